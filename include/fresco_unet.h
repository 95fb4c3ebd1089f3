/* What a UNet ResnetBlock2D of fp16 and bf16 pipelines needs beside vae_conv (diffusers 0.19.3 ResnetBlock2D as the SD-1.5 UNet and
 * ControlNet configure it: 32 groups, swish, time_embedding_norm "default").  DESIGN.md section 19.
 *
 * These entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its
 * stream convention; like the vae_* functions they are declared beside fresco_hip.h, whose surface is pinned to its
 * fresco_* names.  No atomics, fixed summation orders: same inputs give the same bits.
 *
 *   unet_groupnorm_workspace_bytes / unet_groupnorm : y = [SiLU] GroupNorm(32, C, eps)(x + addend) on x (n, P, C) fp16 NHWC
 *     rows -> y fp16 in the same layout.  addend (optional, may be NULL): fp32 (n, C), one term per image and channel, added
 *     in fp32 before the statistics and before the normalisation (the time embedding of the block's second norm).  gamma and
 *     beta are fp32 (C).  C is any multiple of 64 from 64 to 2560: a group is C / 32 channels, an even number.  Statistics
 *     are fp64 sums in a fixed order; the normalisation is fp32 with one rounding to fp16.  Two forms, chosen by the shape
 *     alone (unet.hip's header comment): where the plane of one image's smallest 16-byte aligned run of whole groups fits
 *     in LDS, one launch that reads x once; otherwise partial sums per 64 pixels, a finish step, and the apply pass.  The
 *     workspace size is never 0 for a shape unet_groupnorm accepts (0: a shape it refuses).  With UNET_ELEM_BF16 in the
 *     `silu` word (below) x and y are bf16 and the one rounding is to bf16; nothing else changes.
 *   unet_temb : out[i, co] = bias[co] + conv_bias[co] + sum_k SiLU(temb[i, k]) W[co, k]: time_emb_proj(SiLU(temb)) with the
 *     bias of the block's first convolution folded in: the addend of the second norm.  temb fp16 (n, K), W fp16 (cout, K)
 *     row-major, bias and conv_bias fp32 (cout), out fp32 (n, cout).  SiLU and the sums are fp32.  n <= 64, K % 8 == 0; the
 *     weights are read once for all n rows.  unet_temb_dt: the same with temb and W of `dtype`, FRESCO_F16 or FRESCO_BF16.
 *
 * FRESCO_EINVAL: null pointers (addend excepted), non-positive sizes, a negative or NaN eps, pointers not aligned to what
 * is read in 16-byte pieces.  FRESCO_EUNSUPPORTED: C outside the list, K % 8, n > 64 (unet_temb) or > 65535, a pixel count
 * that does not fit 31 bits (pixels are indexed in int32, element offsets in int64).  FRESCO_EWORKSPACE: a short workspace.
 * All before any HIP call.
 */
#ifndef FRESCO_UNET_H
#define FRESCO_UNET_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* unet_groupnorm's `silu` argument is a word of flags: bit 0 applies SiLU; UNET_ELEM_BF16 makes x and y bf16 instead of fp16
 * (addend, gamma and beta stay fp32, the statistics fp64; the workspace and the form depend on the shape alone, both types
 * being 2 bytes wide); any other bit is FRESCO_EINVAL.  The value equals VAE_ELEM_BF16 of fresco_vae.h. */
#define UNET_ELEM_BF16 0x100

size_t unet_groupnorm_workspace_bytes(int n, int P, int C);
int unet_groupnorm(const void* x, const float* addend /* may be NULL */, const float* gamma, const float* beta, void* y,
                   void* workspace, size_t workspace_bytes, int n, int P, int C, float eps, int silu, void* stream);
/* 1: the shape takes the one-launch LDS form, 0: the three-launch form, -1: a shape unet_groupnorm refuses */
int unet_groupnorm_lds_form(int n, int P, int C);
int unet_temb(const void* temb, const void* weight, const float* bias, const float* conv_bias, float* out, int n, int K,
              int cout, void* stream);
/* unet_temb with the type of temb and weight as an argument: dtype FRESCO_F16 (what unet_temb passes) or FRESCO_BF16; bias,
 * conv_bias and out stay fp32.  Any other code: FRESCO_EINVAL; every other check answers as unet_temb's. */
int unet_temb_dt(const void* temb, const void* weight, const float* bias, const float* conv_bias, float* out, int n, int K,
                 int cout, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_UNET_H */
