/* What the CLIP text model of fp16 pipelines (pipe.text_encoder; fresco_amd/text_encoder.py) needs beside unet_layernorm
 * (fresco_unet_tf.h) and vae_conv (fresco_vae.h): the token + position embedding, a causal attention at head dim 64 and the
 * projection with CLIP's quick-GELU.  DESIGN.md section 24.
 *
 * The entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its stream
 * convention (`stream` is a hipStream_t, null for the default stream; nothing synchronises); they are declared beside
 * fresco_hip.h, whose surface is pinned to its fresco_* names.  fp16 only.  No atomics, a fixed summation order: same inputs
 * give the same bits.  Every argument check answers before any HIP call.
 *
 *   clip_embed : out[b, t, :] = tok[ids[b, t], :] + pos[t, :], fp16 + fp16 rounded once.  tok (vocab, C) and pos (>= L, C)
 *     dense fp16, read where they live; ids (B, L) int64, dense; out (B, L, C) dense fp16.  C a multiple of 8: rows move in
 *     16-byte pieces.  An id outside [0, vocab) reads nothing from the table; its output row is NaN.
 *     FRESCO_EINVAL: a null pointer, a non-positive size, tok / pos / out not aligned to 16 bytes, ids not aligned to 8.
 *     FRESCO_EUNSUPPORTED: C not a multiple of 8, B * L of 2^31 or more.
 *
 *   clip_attention : out[b, i, h*D + d] = sum_{j <= i} softmax_j(scale * q[b, i, h, :] . k[b, j, h, :]) * v[b, j, h, d],
 *     D = 64, 1 <= L <= 128.  q, k and v are (B, L, H*D) with the common row stride qkv_ld (elements): row b*L + i starts
 *     (b*L + i) * qkv_ld elements after the pointer, so they may be the column slices of one (B L, 3 H D) q | k | v buffer;
 *     out (B, L, H*D) with row stride out_ld.  The mask is a selection on the fp32 scores (-inf before the row maximum), so
 *     the rows of the result do not depend on what later keys and values hold, as long as those are finite.  fp32 scores
 *     from the fp16 MFMA, scale and softmax in fp32, P rounded to fp16 for P.V, fp32 accumulators, one rounding of the
 *     output.  Nothing is read past row L of a sequence.  One launch, no workspace.  No key-padding mask.
 *     FRESCO_EINVAL: a null pointer, a non-positive size, scale <= 0 (or NaN), a row stride below H*D or not a multiple of 8,
 *     a pointer not aligned to 16 bytes, a dtype code that names no element type.  FRESCO_EUNSUPPORTED: D != 64, L above 128,
 *     a dtype other than FRESCO_F16, B or H above 65535.
 *
 *   clip_fc1 : out = quick_gelu(x W^T + bias), quick_gelu(g) = g * sigmoid(1.702 g).  x (M, K) dense fp16, W (N, K) dense
 *     fp16, bias fp32 (N), out (M, N) fp16 with row stride ldo.  Bias, sigmoid and product in fp32, one rounding; the
 *     pre-activation is never written.  Any M >= 1; K a multiple of 32, N a multiple of 64.
 *     FRESCO_EINVAL: a null pointer, a non-positive size, ldo below N or not a multiple of 4, x / w / bias not aligned to 16
 *     bytes, out not aligned to 8.  FRESCO_EUNSUPPORTED: K % 32, N % 64, M of 2^31 or more, N of 2^30 or more.
 */
#ifndef FRESCO_TEXT_H
#define FRESCO_TEXT_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int clip_embed(const void* tok, const void* pos, const int64_t* ids, void* out, int B, int L, int C, int vocab, void* stream);

int clip_attention(const void* q, const void* k, const void* v, int64_t qkv_ld, void* out, int64_t out_ld, int B, int H, int L,
                   int D, float scale, int dtype, void* stream);

int clip_fc1(const void* x, const void* w, const float* bias, void* out, int64_t M, int K, int N, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_TEXT_H */
