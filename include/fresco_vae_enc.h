/* The VAE encoder of fp16 pipelines (diffusers AutoencoderKL.encode of the SD-1.5 VAE; reference call sites:
 * src/pipe_FRESCO.py:47 and :160, src/diffusion_hacked.py:874).  DESIGN.md section 18.
 *
 * The encoder's resnets, its mid block, GroupNorm and its stride-1 convolutions are the decoder's entry points
 * (fresco_vae.h); these four are what the decoder lacks.  They live in libfresco_hip.so and share its error codes
 * (fresco_hip.h), its last-error string and its stream convention.  Activations are fp16 NHWC rows between layers;
 * accumulation is fp32.  No float atomics, no split-K across workgroups: same inputs give the same bits.
 *
 *   vaeenc_input     : image (n, 3, H, W) fp16 NCHW -> out (n, H, W, cpad) fp16 NHWC, channels 3 .. cpad - 1 zero
 *     (cpad % 8 == 0, 8 <= cpad <= 64): what encoder.conv_in reads through vae_conv with its weights padded to cpad input
 *     channels.
 *   vaeenc_conv_down : Downsample2D(padding=0), i.e. Conv2d(cin, cout, 3, stride 2, padding 0) behind F.pad(x, (0, 1, 0, 1)):
 *       out[n, yo, xo, co] = bias[co] + sum_{ky, kx, ci} x[n, 2 yo + ky, 2 xo + kx, ci] W[co, (ky, kx, ci)],
 *     a source row of index H or a source column of index W reads zero; nothing is padded on the top or left.  Ho = H / 2,
 *     Wo = W / 2 (integer division) for any H, W >= 2: at an odd H the pad row is never reached.  x (n, H, W, cin) fp16 NHWC,
 *     cin % 32 == 0; W (cout, 9 cin) fp16 row-major with k = (ky, kx, ci); bias fp32; out (n, Ho, Wo, cout) fp16 NHWC.  Plain
 *     fp16 operands on v_mfma_f32_32x32x16_f16, fp32 accumulators, one rounding.  Any cout (a ragged last column tile reads
 *     zero weights and stores nothing beyond cout).
 *   vaeenc_moments   : h (n hh ww, 8) fp32 rows -- encoder.conv_out's result from vae_conv with VAE_OUT_F32, so that nothing
 *     is rounded between conv_out and quant_conv -- -> quant_conv (1 x 1, 8 -> 8: weight (8, 8) and bias (8) fp32, computed in
 *     fp32) -> params (n, 8, hh, ww) fp16 NCHW, rounded once: the tensor DiagonalGaussianDistribution is built from.
 *   vaeenc_sample    : params (n, 8, hh, ww) fp16 (mean = channels 0 - 3, logvar = channels 4 - 7), noise (n, 4, hh, ww) fp16
 *     -> out (n, 4, hh, ww) fp16 = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), computed in fp32 from the
 *     fp16 inputs and rounded ONCE.  The module computes the same expression as a chain of fp16 tensor operations (clamp,
 *     0.5 *, exp, * noise, + mean, * scale), each rounded to fp16: one rounding of the fp32 value is at least as close to
 *     the exact value as that chain, and is not bit-equal to it.
 *
 * FRESCO_EINVAL: null pointers, non-positive sizes, cpad outside its rule, a NaN scale, rows read in 16-byte pieces not
 * 16-byte aligned (x, w, bias of vaeenc_conv_down; out of vaeenc_input; h of vaeenc_moments), out of vaeenc_conv_down not
 * 8-byte aligned.  FRESCO_EUNSUPPORTED: H or W below 2 or cin % 32 in vaeenc_conv_down, more than 65535 images there, a
 * pixel count or a workgroup count that does not fit 31 bits (pixels are indexed in int32, element offsets in int64).  All
 * before any HIP call.
 */
#ifndef FRESCO_VAE_ENC_H
#define FRESCO_VAE_ENC_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int vaeenc_input(const void* image, void* out, int n, int H, int W, int cpad, void* stream);
int vaeenc_conv_down(const void* x, const void* w, const float* bias, void* out, int n, int H, int W, int cin, int cout,
                     void* stream);
int vaeenc_moments(const float* h, const float* weight, const float* bias, void* params, int n, int hh, int ww, void* stream);
int vaeenc_sample(const void* params, const void* noise, void* out, int n, int hh, int ww, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_VAE_ENC_H */
