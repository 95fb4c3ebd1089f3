/* What is left of a fp16 UNet2DConditionModel and ControlNetModel (diffusers 0.19.3, SD-1.5) around their resnets,
 * transformer blocks and attention: Downsample2D, the two ends, the time-embedding MLP and the ControlNet's condition
 * embedding.  DESIGN.md section 23.  Upsample2D, conv_in / conv_out and the zero convolutions are vae_conv's forms
 * (fresco_vae.h) and need nothing here.
 *
 * These entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its
 * stream convention; they are declared beside fresco_hip.h, whose surface is pinned to its fresco_* names.  Activations are
 * fp16 NHWC rows between layers; accumulation is fp32 in a fixed order.  No atomics, no split-K: same inputs, same bits.
 *
 *   unet_conv3 : Conv2d(cin, cout, 3, stride, padding 1) [+ SiLU]:
 *       out[n, yo, xo, co] = act(bias[co] + sum_{ky, kx, ci} x[n, stride yo + ky - 1, stride xo + kx - 1, ci] W[co, (ky, kx, ci)]),
 *     a source row outside 0 .. H - 1 or a source column outside 0 .. W - 1 reads zero.  stride 1 or 2; act UNET_ACT_NONE or
 *     UNET_ACT_SILU.  x (n, H, W, cin) fp16 NHWC, cin % 32 == 0; W (cout, 9 cin) fp16 row-major with k = (ky, kx, ci); bias
 *     fp32; out (n, Ho, Wo, cout) fp16 NHWC, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, any H, W >= 1.  Plain fp16
 *     operands on v_mfma_f32_32x32x16_f16, fp32 accumulators; bias and SiLU in fp32, one rounding.  Any cout (a ragged last
 *     column tile reads zero weights and stores nothing beyond cout).
 *   unet_input : x (n, c, H, W) fp16 NCHW -> out (n, H, W, cpad) fp16 NHWC, channels c .. cpad - 1 zero (1 <= c <= cpad,
 *     cpad % 8 == 0, 8 <= cpad <= 64).  Exact.  The 4-channel latents and the 3-channel condition image.
 *   unet_time_linear : out (n, cout) fp16 = round16(bias + f(src) W^T), n <= 64, K % 8 == 0; W (cout, K) fp16, bias fp32.
 *     src_kind UNET_SRC_TIMESTEPS: src fp32 (n), f = Timesteps(K, flip_sin_to_cos=True, downscale_freq_shift=0):
 *       f[k] = cos(t w_k) for k < K / 2, f[K / 2 + i] = sin(t w_i), w_i = exp(-ln(10000) i / (K / 2)), computed in fp32 and
 *       rounded to fp16; sin_out (optional, fp16 (n, K)) receives f.
 *     src_kind UNET_SRC_SILU_ROWS: src fp16 (n, K), f = SiLU in fp32; sin_out must be NULL.
 *     TimestepEmbedding (linear_1, SiLU, linear_2) is two calls.
 *
 * FRESCO_EINVAL: null pointers, non-positive sizes, cpad or c outside unet_input's rule, rows read in 16-byte pieces not
 * 16-byte aligned (x, w, bias of unet_conv3; out of unet_input; w, fp16 src and sin_out of unet_time_linear), out of
 * unet_conv3 not 8-byte aligned.  FRESCO_EUNSUPPORTED: a stride outside {1, 2}, an act or src_kind outside its list,
 * cin % 32, more than 65535 images, n > 64 or K % 8 in unet_time_linear, sin_out with UNET_SRC_SILU_ROWS, a pixel count or a
 * workgroup count that does not fit 31 bits.  All before any HIP call.
 */
#ifndef FRESCO_UNET_SHELL_H
#define FRESCO_UNET_SHELL_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_ACT_NONE 0
#define UNET_ACT_SILU 1
#define UNET_SRC_TIMESTEPS 0
#define UNET_SRC_SILU_ROWS 1

int unet_conv3(const void* x, const void* w, const float* bias, void* out, int n, int H, int W, int cin, int cout, int stride,
               int act, void* stream);
int unet_input(const void* x, void* out, int n, int c, int H, int W, int cpad, void* stream);
int unet_time_linear(const void* src, int src_kind, const void* w, const float* bias, void* out, void* sin_out /* may be NULL */,
                     int n, int K, int cout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_UNET_SHELL_H */
