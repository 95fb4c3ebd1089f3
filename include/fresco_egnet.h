/* C ABI of libfresco_egnet.so: the kernels of the EGNet saliency detector that are no convolutions (fresco_amd/csrc/egnet.hip).
 * A library of its own next to libfresco_hip.so (whose surface is one exported function per operation of fresco_hip.h, as
 * tests/test_capi_surface_cpu.py pins it): same conventions -- plain device pointers, sizes, a hipStream_t as void*, the
 * FRESCO_E* return codes of fresco_hip.h, nothing allocated inside.  It also exports fresco_version / fresco_last_error of its own
 * build (the launch error of ITS last failed launch). */
#ifndef FRESCO_EGNET_H
#define FRESCO_EGNET_H
#include "fresco_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The EGNet saliency detector behind the background smoothing (src/EGNet/model.py, resnet.py; called by
 * src/utils.py::get_saliency).  DESIGN.md section 13.  The network's convolutions are fresco_fn_gemm / fresco_fn_conv7_rgb
 * calls (BatchNorm folded into weights and bias); these are the pieces around them.  Planes and range_flag as in section (l)
 * of fresco_hip.h.
 * Same inputs give bit-identical outputs (no float atomics).
 *   fresco_egnet_input     : frames (n, H, W, 3) uint8 -> cv2sod's tensor as NHWC fp32 rows (n, H / 2, W / 2, 3): channel c
 *     minus (104.00699, 116.66877, 122.67892)[c], then the mean of each 2 x 2 block = F.interpolate(scale_factor=0.5,
 *     bilinear); the block sum is exact and (sum / 4 - mean) is rounded to fp32 once; an odd last row / column is dropped.
 *   fresco_egnet_pool      : MaxPool2d(3, stride 2, padding 1, ceil_mode=True) on x (n, H, W, 64) fp32 NHWC -> the planes
 *     of the pooled map, (n, OH, OW, 64), and its fp32 values where `out` is given; OH follows PyTorch's rule (ceil, minus
 *     one where the last window would start beyond the input and its left padding).
 *   fresco_egnet_resize_add: F.interpolate(x, (H, W), bilinear, align_corners=True) on x (n, h, w, C) fp32 NHWC [+ addend
 *     (n, H, W, C)] [ReLU] -> out fp32 and / or the planes, C % 32 == 0, C <= 512.  The source position d (h - 1) / (H - 1)
 *     is a quotient and a remainder of integers (exact taps, the weight rounded once); h == H and w == W copies x exactly.
 *   fresco_egnet_saliency  : logit (n, h, w) fp32 -> align_corners=True resize to (Hs, Ws), 1 / (1 + expf(-x)), k x k box
 *     sum with replicate padding (added in row order), clamp to [0, 1], 1 - x: out (n, 1, Hs, Ws) fp32; logit_out
 *     (n, Hs, Ws) (optional): the resized logit.  k odd, <= 15.
 * FRESCO_EUNSUPPORTED: C outside the above, H or W < 2 (input), k even or > 15, n H W >= 2^31, a resized side > 32768.  FRESCO_EINVAL: null pointers,
 * non-positive sizes or scale, fp32 rows read in 16-byte pieces not 16-byte aligned, planes not 8-byte aligned.  All before
 * any launch.
 * ------------------------------------------------------------------------------------------ */
int fresco_egnet_input(const uint8_t* frames, float* out, int n, int H, int W, void* stream);
int fresco_egnet_pool(const float* x, float* out /* may be NULL */, void* out_hi, void* out_lo, int n, int H, int W, int C,
                      float split_scale, int32_t* range_flag, void* stream);
int fresco_egnet_resize_add(const float* x, const float* addend /* may be NULL */, float* out /* may be NULL */,
                            void* out_hi /* may be NULL */, void* out_lo, int n, int h, int w, int H, int W, int C, int relu,
                            float split_scale, int32_t* range_flag, void* stream);
int fresco_egnet_saliency(const float* logit, float* out, float* logit_out /* may be NULL */, int n, int h, int w, int Hs,
                          int Ws, int k, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* FRESCO_EGNET_H */
