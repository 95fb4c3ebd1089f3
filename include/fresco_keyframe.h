/* Key-frame selection on the device (reference: src/keyframe_selection.py get_keyframe_ind, which runs
 * resize_image -> cv2.GaussianBlur -> numpy2tensor(...).cuda() -> F.mse_loss(...).cpu() once per frame of the video).
 *
 * These entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its
 * stream convention, but they are named keyframe_* and declared here: the surface of fresco_hip.h is pinned to its
 * fresco_* names.  Moving them there as fresco_keyframe_* is a follow-up that also updates that pin.
 * As everywhere in the library nothing is allocated inside: the caller holds the resize tables and the workspace.
 *
 * All arithmetic is integer or fixed-order fp32 on uint8 frames (n, H, W, 3): same inputs give the same bits.
 *
 *   keyframe_resize_table_bytes: the size of the coverage tables of a geometry (H0, W0) -> (H, W); 0 for one the resize
 *     refuses.
 *   keyframe_resize_table   : writes them to HOST memory (no HIP call): OpenCV's computeResizeAreaTab per axis, computed in
 *     double and stored as float -- per output index the partial-left, full and partial-right entries over a cell width of
 *     min(scale, size - start), scale = 1 / (dsize / ssize).  32-bit words: x.ofs[W + 1] | x.si[W0 + 2 W] |
 *     x.alpha[W0 + 2 W] | y.ofs[H + 1] | y.si[H0 + 2 H] | y.alpha[H0 + 2 H]; entries ofs[d] .. ofs[d + 1] - 1 belong to
 *     output index d.  The caller copies them to the device once per geometry and keeps them.
 *   keyframe_resize_area_u8 : src (n, H0, W0, 3) -> dst (n, H, W, 3), OpenCV's INTER_AREA for 8-bit images where no side is
 *     enlarged; `table` is the device copy of the tables.  Both scale factors integer (within DBL_EPSILON, as cv::resize
 *     tests it): the integer sum over the box, (s + 2) >> 2 for a 2 x 2 box, otherwise round-half-even of
 *     float(s) * (1.f / area); the tables are not read.  Otherwise each source row is summed in table order in fp32
 *     (buf += S * alpha), rows are accumulated as sum += beta * buf in fp32, the result is rounded half-even and saturated.
 *     A side of equal sizes is a copy either way.  One launch, one thread per output pixel.  The kernel clamps what it
 *     reads from the tables to the arrays and the frame, so a wrong table gives a wrong picture, not a stray access.
 *   keyframe_workspace_bytes: what keyframe_frame_errors needs for (n, H, W); 0 for sizes the call refuses.
 *   keyframe_frame_errors   : frames (n, H, W, 3), carry (H, W, 3) or NULL -> err[n] (uint64): err[i] = the sum over the
 *     frame of (blur(frame i-1) - blur(frame i))^2 with frame -1 = carry; err[0] = 0 without a carry.  blur is OpenCV's 8-bit
 *     9 x 9 Gaussian at sigma 0 (1.7): weights [4 13 30 51 60 51 30 13 4] / 256, reflect-101 borders, a 16-bit horizontal
 *     pass, a 32-bit vertical pass, (v + 32768) >> 16.  The blurred frames are never stored.  Two launches: per-tile partial
 *     sums into the workspace, then their sum per pair -- integer, so independent of the order of the blocks.
 *
 * FRESCO_EINVAL: a null src / dst / table / frames / err / workspace, non-positive sizes, a table not 4-byte aligned, err
 * or a workspace not 8-byte aligned.  FRESCO_EUNSUPPORTED: a side that would be enlarged or a source side above 2^24
 * (resize), a side below 5 (errors: the reflection would fold twice), n H W 3 >= 2^40 source bytes, n H W >= 2^31 output
 * pixels of the resize.  FRESCO_EWORKSPACE: a short table or workspace.  FRESCO_ELAUNCH: a failed launch
 * (fresco_last_error has the text).  The argument checks all answer before any HIP call.
 */
#ifndef FRESCO_KEYFRAME_H
#define FRESCO_KEYFRAME_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t keyframe_resize_table_bytes(int H0, int W0, int H, int W);
int keyframe_resize_table(int H0, int W0, int H, int W, void* host_table, size_t table_bytes);
int keyframe_resize_area_u8(const uint8_t* src, uint8_t* dst, const void* table, size_t table_bytes, int n, int H0, int W0,
                            int H, int W, void* stream);
size_t keyframe_workspace_bytes(int n, int H, int W);
int keyframe_frame_errors(const uint8_t* frames, const uint8_t* carry /* may be NULL */, uint64_t* err, void* workspace,
                          size_t workspace_bytes, int n, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_KEYFRAME_H */
