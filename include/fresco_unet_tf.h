/* What a UNet Transformer2DModel of fp16 pipelines needs beside unet_groupnorm and vae_conv (diffusers 0.19.3
 * Transformer2DModel / BasicTransformerBlock as the SD-1.5 UNet and ControlNet configure them: LayerNorm, GEGLU
 * feed-forward).  DESIGN.md section 20.
 *
 * These entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its
 * stream convention; like the other unet_* functions they are declared beside fresco_hip.h, whose surface is pinned to its
 * fresco_* names.  No atomics, fixed summation orders: same inputs give the same bits.
 *
 *   unet_layernorm : y = LayerNorm(C, eps)(x [+ r]) * gamma + beta on rows of C fp16 values.  x (rows, C) with row stride ldx
 *     (elements); r (optional, may be NULL) in the same shape with row stride ldr; y fp16 with row stride ldy; sum_out
 *     (optional, may be NULL) fp16 with row stride ld_sum receives x + r rounded once: the residual stream the next add
 *     reads.  gamma and beta are fp32 (C).  C % 8 == 0, 64 <= C <= 2560; every stride is a multiple of 8 and >= C.  Rows are
 *     read once, in 16-byte pieces.  Statistics are fp64 sums in a fixed order; the normalisation is fp32 from the fp32 sum
 *     x + r (not from the rounded sum_out), with one rounding to fp16.  One launch.
 *   unet_geglu : out[m, c] = (sum_k x[m, k] Wv[c, k] + bv[c]) * gelu(sum_k x[m, k] Wg[c, k] + bg[c]), the exact (erf) GELU.
 *     x (M, K) fp16 dense rows; out (M, inner) fp16 with row stride ldo.  w is ONE packed (2 inner, K) fp16 matrix whose rows
 *     go in blocks of 64: the 32 value rows of channels 32 b .. 32 b + 31, then their 32 gate rows; bias is fp32 (2 inner)
 *     in the same order.  fp32 accumulation, the product in fp32, one rounding.  K % 32 == 0, inner % 32 == 0.  M counts the
 *     rows of all images together.  The (M, 2 inner) projection is never written.
 *
 * FRESCO_EINVAL: null pointers (r and sum_out excepted), non-positive sizes, a negative or NaN eps, a stride below the row
 * or not a multiple of 8 (ldo: of 4), pointers not aligned to what is read or written in pieces (16 bytes; out of
 * unet_geglu: 8).  FRESCO_EUNSUPPORTED: C outside the range or C % 8, K % 32, inner % 32, a row count that does not fit 31
 * bits.  All before any HIP call.
 */
#ifndef FRESCO_UNET_TF_H
#define FRESCO_UNET_TF_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int unet_layernorm(const void* x, int64_t ldx, const void* r /* may be NULL */, int64_t ldr, const float* gamma,
                   const float* beta, void* y, int64_t ldy, void* sum_out /* may be NULL */, int64_t ld_sum, int64_t rows, int C,
                   float eps, void* stream);
int unet_geglu(const void* x, const void* w, const float* bias, void* out, int64_t M, int K, int inner, int64_t ldo,
               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_UNET_TF_H */
