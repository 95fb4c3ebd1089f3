/* C ABI of libfresco_canny.so: the Canny edge detector behind the ControlNet condition `controlnet_type: canny`
 * (fresco_amd/csrc/canny.hip).  A library of its own next to libfresco_hip.so, like libfresco_egnet.so: same conventions --
 * plain device pointers, sizes, a hipStream_t as void*, the FRESCO_E* return codes and dtype codes of fresco_hip.h, nothing
 * allocated inside.  It also exports fresco_version / fresco_last_error of its own build. */
#ifndef FRESCO_CANNY_H
#define FRESCO_CANNY_H
#include "fresco_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * OpenCV's generic Canny(src, low, high, apertureSize = 3, L2gradient = false) on 8-bit 3-channel frames, batched
 * (reference: src/ControlNet/annotator/canny/__init__.py; DESIGN.md section 14 has the rules).  All integer: same inputs give
 * the same bits.
 *   fresco_canny_workspace_bytes: what fresco_canny_hysteresis needs for (n, H, W); 0 for sizes the calls refuse.
 *   fresco_canny_classify  : frames (n, H, W, 3) uint8 -> cls (n, H, W) uint8: 0 (no edge), 1 (weak: a local maximum of
 *     the gradient magnitude above `low`), 2 (strong: above `high` as well).  3 x 3 Sobel per channel with replicated
 *     borders, |dx| + |dy|, the channel of the largest magnitude (the first on ties), zero magnitude outside the frame,
 *     non-maximum suppression along the quantised gradient direction.  low > high: the two are swapped.  One launch.
 *   fresco_canny_hysteresis: cls -> out (n, H, W) uint8: 255 on every class 1 / 2 pixel whose 8-connected component of
 *     class 1 / 2 pixels holds a class 2 pixel, else 0 (a class byte >= 3 counts as 0; frames are independent).  cond,
 *     when given: the ControlNet condition (n, 3, H, W) of cond_dtype (FRESCO_F16 / FRESCO_BF16 / FRESCO_F32),
 *     ((out / 255) * 2 - 1) * 0.5 + 0.5 in fp32 in that order, rounded once -- what fresco_hed_fuse writes.  Union-find
 *     labelling in four launches whatever the picture; no host loop, no read-back, no synchronisation.
 * FRESCO_EINVAL: null frames / cls / out / workspace, non-positive n / H / W, a workspace not 4-byte aligned or a cond not
 * aligned to its element, an unknown cond_dtype with a non-null cond.  FRESCO_EUNSUPPORTED: n H W >= 2^31.
 * FRESCO_EWORKSPACE: a short workspace.  All before any launch.
 * ------------------------------------------------------------------------------------------ */
size_t fresco_canny_workspace_bytes(int n, int H, int W);
int fresco_canny_classify(const uint8_t* frames, uint8_t* cls, int n, int H, int W, int low, int high, void* stream);
int fresco_canny_hysteresis(const uint8_t* cls, uint8_t* out, void* cond /* may be NULL */, int cond_dtype, void* workspace,
                            size_t workspace_bytes, int n, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_CANNY_H */
