/* Flash attention at head dim 160, the head dim of the SD-1.5 UNet's and ControlNet's 1280-wide transformer blocks (8 heads):
 * what the plain attention processor (fresco_amd/unet_attention.py) needs beside fresco_linear, fresco_attn_fwd and vae_conv.
 * DESIGN.md section 21.
 *
 * The entry point lives in libfresco_hip.so and shares its error codes (fresco_hip.h), its last-error string and its stream
 * convention; like the other unet_* functions it is declared beside fresco_hip.h, whose surface is pinned to its fresco_*
 * names.  No atomics, a fixed summation order: same inputs give the same bits.
 *
 *   unet_attention : out[b, i, h*D + d] = sum_j softmax_j(scale * q[b, i, h, :] . k[b, j, h, :]) * v[b, j, h, d],  D = 160.
 *     q (B, Lq, H*D) with row stride q_ld (elements); k and v (B, Lk, H*D) with the common row stride kv_ld; out (B, Lq, H*D)
 *     with row stride out_ld.  Row b*L + i of a tensor starts (b*L + i) * ld elements after its pointer, so q | k | v may be
 *     column slices of one (rows, 3 H D) buffer and k | v of a (rows, 2 H D) one.  Any Lq >= 1 and Lk >= 1.  fp32 scores from
 *     the fp16 MFMA, the scale and the softmax in fp32, P rounded to fp16 for P.V, fp32 accumulators, one rounding of the
 *     output.  Nothing is read past a tensor's last row; rows past Lq are not stored.  One launch, no workspace.
 *
 * FRESCO_EINVAL: a null pointer, a non-positive size, scale <= 0 (or NaN), a row stride below H*D or not a multiple of 8, a
 * pointer not aligned to 16 bytes, a dtype code that names no element type.  FRESCO_EUNSUPPORTED: D != 160, a dtype other
 * than FRESCO_F16 (bf16 is not built), B above 65535, Lq above 32 * 65535, kv_ld of 2^22 elements or more.  All before any HIP call.
 */
#ifndef FRESCO_UNET_ATTN_H
#define FRESCO_UNET_ATTN_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int unet_attention(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out, int64_t out_ld, int B,
                   int H, int Lq, int Lk, int D, float scale, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_UNET_ATTN_H */
