/* The MiDaS depth annotator of the ControlNet condition (`controlnet_type: depth`; reference:
 * src/ControlNet/annotator/midas/__init__.py around DPTDepthModel(backbone="vitb_rn50_384")).  DESIGN.md section 16.
 *
 * These entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its
 * stream convention; like the keyframe_* functions they are declared beside fresco_hip.h, whose surface is pinned to its
 * fresco_* names.  The network's linear layers and convolutions are fresco_fn_gemm calls, its attention is
 * fresco_attn_f32, its resizes fresco_egnet_resize_add; these are the pieces around them.  "Planes" are the (hi, lo) fp16
 * operands of fresco_fn_gemm: x * split_scale = hi + lo, saturating beyond +-65000; a producer that had to saturate ORs 1
 * into *range_flag (may be NULL).  Activations are NHWC fp32 rows.  No float atomics: same inputs give the same bits.
 *
 *   midas_input     : frames (n, H, W, 3) uint8 -> x / 127.5 - 1 as fp32 NHWC (n, H, W, 3), what midas_stem_conv reads.
 *   midas_stem_conv : StdConv2dSame(3, 64, 7, stride 2) at even sizes: "same" padding = 2 before, 3 after.  The kernel and
 *     the weight layout of fresco_fn_conv7_rgb with the window origin at -2: x (n, H, W, 3) fp32, w_hi / w_lo the (64, 224)
 *     planes of the (standardised) weight -> out (n, H / 2, W / 2, 64) fp32.
 *   midas_groupnorm_workspace_bytes / midas_groupnorm_stats: GroupNorm(32, C) statistics of x (n, P, C) fp32, C in
 *     {64, 128, 256, 512, 1024}: per (image, group) the mean and 1 / sqrt(biased variance + eps) over P pixels x C / 32
 *     channels, (n, 32) each.  Workgroups of 256 pixels leave fp64 partial sums in the workspace, a second launch adds
 *     them in chunk order: a fixed order whatever the grid.
 *   midas_groupnorm_apply: y = (x - mean) rstd gamma + beta [ReLU] [+ residual, ReLU] on x (n, H, W, C).  Writes y fp32
 *     (n, H, W, C) and / or the planes; pixel (r, c) of image i goes to plane row (i plane_h + r) plane_w + c, plane_h >= H,
 *     plane_w >= W: with plane_h = H + 1, plane_w = W + 1 into a zero-filled buffer the planes carry the far-side zero
 *     border that a "same" 3 x 3 stride-2 convolution (0 before, 1 after) reads as fresco_fn_gemm's pad = 0.
 *   midas_pool      : MaxPool2dSame(3, stride 2) at even sizes (0 before, 1 after, padding never wins) on x (n, H, W, 64)
 *     fp32 -> out fp32 (n, H / 2, W / 2, 64) (may be NULL) and the planes.
 *   midas_layernorm : nn.LayerNorm(C) on (M, C) fp32 rows, C % 4 == 0, C <= 1024 (the transformer's 768): the mean, then
 *     the biased variance of the centred values, one wave per row -> y fp32 and / or planes (row stride C).
 *   midas_tokens    : out (n, L, C) = [cls | grid (n, L - 1, C)] + pos (L, C), C % 4 == 0.
 *   midas_head_merge: attention output (heads * n, L, 64), batch = head * n + image -> rows (n * L, heads * 64) as fp32
 *     (may be NULL) and / or planes.
 *   midas_rowbias_gelu: GELU(x[m] + rowbias[m / rows_per_img]) (erf form) on (M, C) fp32 rows, C % 4 == 0 -> fp32 and / or
 *     planes: ProjectReadout's concatenated cls token as a per-image bias row.
 *   midas_tail_workspace_bytes / midas_tail: depth (n, H, W) fp32 -> depth_image (n, H, W) uint8 =
 *     trunc(clip((d - min) / (max - min) * 255)), min / max per frame; normal_image (n, H, W, 3) uint8 from the 3 x 3 Sobel
 *     derivatives of the depth (BORDER_REFLECT_101), both zeroed where the normalised depth is below bg_th, the vector
 *     (gx, gy, a) normalised, trunc(clip(v * 127.5 + 127.5)); cond (optional, (n, 3, H, W) of cond_dtype): the ControlNet
 *     condition of the depth image as fresco_hed_fuse writes it.  A constant frame (max == min) gives a zero depth image
 *     and the flat normal (127, 127, 255).  Two launches (per-frame partial min / max, then the maps).  H, W >= 2.
 *
 * FRESCO_EINVAL: null pointers, non-positive sizes or scale, rows read in 16-byte pieces not 16-byte aligned, planes not
 * 8-byte aligned.  FRESCO_EUNSUPPORTED: odd H or W where "same" padding is one-sided, C outside the lists, n H W >= 2^31.
 * FRESCO_EWORKSPACE: a short workspace.  All before any launch.
 */
#ifndef FRESCO_MIDAS_H
#define FRESCO_MIDAS_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int midas_input(const uint8_t* frames, float* out, int n, int H, int W, void* stream);
int midas_stem_conv(const float* x, const void* w_hi, const void* w_lo, float* out, int n, int H, int W, int32_t* range_flag,
                    void* stream);
size_t midas_groupnorm_workspace_bytes(int n, int P, int C);
int midas_groupnorm_stats(const float* x, float* mean, float* rstd, void* workspace, size_t workspace_bytes, int n, int P,
                          int C, float eps, void* stream);
int midas_groupnorm_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                          const float* residual /* may be NULL */, float* y /* may be NULL */, void* out_hi /* may be NULL */,
                          void* out_lo, int n, int H, int W, int C, int plane_h, int plane_w, int relu, float split_scale,
                          int32_t* range_flag, void* stream);
int midas_pool(const float* x, float* out /* may be NULL */, void* out_hi, void* out_lo, int n, int H, int W, int C,
               float split_scale, int32_t* range_flag, void* stream);
int midas_layernorm(const float* x, const float* gamma, const float* beta, float* y /* may be NULL */,
                    void* out_hi /* may be NULL */, void* out_lo, int64_t M, int C, float eps, float split_scale,
                    int32_t* range_flag, void* stream);
int midas_tokens(const float* grid, const float* cls, const float* pos, float* out, int n, int L, int C, void* stream);
int midas_head_merge(const float* x, float* out /* may be NULL */, void* out_hi /* may be NULL */, void* out_lo, int n,
                     int L, int heads, float split_scale, int32_t* range_flag, void* stream);
int midas_rowbias_gelu(const float* x, const float* rowbias, float* out /* may be NULL */, void* out_hi /* may be NULL */,
                       void* out_lo, int64_t M, int C, int rows_per_img, float split_scale, int32_t* range_flag,
                       void* stream);
size_t midas_tail_workspace_bytes(int n, int H, int W);
int midas_tail(const float* depth, uint8_t* depth_image, uint8_t* normal_image, void* cond /* may be NULL */, int cond_dtype,
               void* workspace, size_t workspace_bytes, int n, int H, int W, float a, float bg_th, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_MIDAS_H */
