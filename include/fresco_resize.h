/* resize_image where it enlarges (reference: src/utils.py resize_image -- cv2.resize with INTER_LANCZOS4 when the short side
 * is below the resolution, and INTER_AREA on a geometry whose rounding to multiples of 64 enlarges a side, where OpenCV
 * leaves the area rule for a two-tap one).  fresco_keyframe.h has the case where no side is enlarged.
 *
 * These entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its
 * stream convention; they are named frame_resize_* and declared here because the surfaces of fresco_hip.h and
 * fresco_keyframe.h are pinned to their names (the follow-up of DESIGN.md section 15 moves all of them).  Nothing is
 * allocated inside: the caller holds the tap table.
 *
 * All arithmetic on the device is integer on uint8 frames (n, H, W, 3): same inputs give the same bits, in any order of
 * the blocks.  Per axis inv = dsize / ssize and scale = 1 / inv in double, as cv::resize forms them.
 *
 *   method FRAME_RESIZE_LANCZOS4: output index d samples at fx = (float)((d + 0.5) * scale - 0.5), s = floor(fx), phase
 *     fx - s in float; eight taps s - 3 .. s + 4, replicated at the borders; coefficients of interpolateLanczos4 (the unit
 *     tap for a phase below FLT_EPSILON; otherwise (cs[i][0] sin y0 + cs[i][1] cos y0) / y_i^2 from double angles, summed
 *     and normalised in float), each rounded half-even to 11 fractional bits with no renormalisation.  A pixel is
 *     sum_j beta_j (sum_i alpha_i src[y_j][x_i]) in 32-bit integers, then clamp((v + 2^21) >> 22, 0, 255).
 *   method FRAME_RESIZE_LINEAR_AREA: what INTER_AREA does when a side is enlarged, on both axes: s = floor(d * scale),
 *     fx = (float)((d + 1) - (s + 1) * inv), 0 if not positive, else its fraction; s is clamped to the axis with fx = 0;
 *     taps s and s + 1 with (1.f - fx, fx) * 2048 rounded half-even; h = a0 S[s] + a1 S[s + 1] in 32-bit integers and
 *     out = sat_u8((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2).  An axis of equal sizes is a copy.
 *
 *   frame_resize_table_bytes: the size of the tap table of a geometry and method; 0 for one the resize refuses.
 *   frame_resize_table   : writes it to HOST memory (no HIP call): x.first[W] (int32: the first tap's source index,
 *     unclamped) | x.coef[W][K] (int16) | y.first[H] | y.coef[H][K], K = 8 or 2.  The caller copies it to the device once
 *     per geometry and method and keeps it.
 *   frame_resize_u8      : src (n, H0, W0, 3) -> dst (n, H, W, 3); `table` is the device copy.  One launch, one workgroup
 *     per 32 x 32 output tile: the tile's source window goes to LDS as bytes at clamped coordinates, the horizontal pass
 *     runs once per window row into 32-bit LDS words, the vertical pass reads those.  The kernel clamps every tap to its
 *     window and the window to the frame, so a wrong table gives a wrong picture, not a stray access.  src needs no
 *     alignment.
 *
 * FRESCO_EINVAL: a null src / dst / table, non-positive sizes, an unknown method, a table not 4-byte aligned.
 * FRESCO_EUNSUPPORTED: an axis with ssize > 2 dsize (resize_image never asks for one; the bound keeps the LDS window
 * fixed), a source side above 2^24, n H0 W0 3 >= 2^40 source bytes, n H W >= 2^31 output pixels, more than 2^23 tiles in
 * one call.  FRESCO_EWORKSPACE: a short table.  FRESCO_ELAUNCH: a failed launch (fresco_last_error has the text).  The
 * argument checks all answer before any HIP call.
 */
#ifndef FRESCO_RESIZE_H
#define FRESCO_RESIZE_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#define FRAME_RESIZE_LANCZOS4 0
#define FRAME_RESIZE_LINEAR_AREA 1

#ifdef __cplusplus
extern "C" {
#endif

size_t frame_resize_table_bytes(int H0, int W0, int H, int W, int method);
int frame_resize_table(int H0, int W0, int H, int W, int method, void* host_table, size_t table_bytes);
int frame_resize_u8(const uint8_t* src, uint8_t* dst, const void* table, size_t table_bytes, int n, int H0, int W0, int H,
                    int W, int method, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_RESIZE_H */
