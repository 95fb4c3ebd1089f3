/* The VAE decoder of fp16 pipelines (diffusers AutoencoderKL.decode of the SD-1.5 VAE; reference call sites:
 * src/pipe_FRESCO.py:44-47, run_fresco.py:251).  DESIGN.md section 17.
 *
 * These entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its
 * stream convention; like the keyframe_* and midas_* functions they are declared beside fresco_hip.h, whose surface is
 * pinned to its fresco_* names.  Activations are fp16 NHWC rows between layers; accumulation is fp32, statistics fp64.
 * No float atomics, no split-K across workgroups: same inputs give the same bits.
 *
 *   vae_input : latents z (n, 4, h, w) fp16 NCHW -> post_quant_conv (1 x 1, 4 -> 4: weight (4, 4) and bias (4) fp32, computed
 *     in fp32) -> out (n, h, w, cpad) fp16 NHWC, channels 4 .. cpad - 1 zero (cpad % 8 == 0, 8 <= cpad <= 64): what conv_in
 *     reads with its weights padded to cpad input channels.
 *   vae_conv  : out = [residual +] sum_k A[., k] W[co, k] + bias, plain fp16 operands on v_mfma_f32_32x32x16_f16, fp32
 *     accumulators.  W is (cout, K) fp16 row-major, K = ksize * ksize * cin with k = (ky, kx, ci); image i uses
 *     w + i * w_img_stride (elements; 0 = one matrix for all images).
 *       ksize 3: A is the implicit im2col of x (n, Hs, Ws, cin), stride 1, zero padding 1; out has H x W pixels per image.
 *         up2 = 0: Hs = H, Ws = W.  up2 = 1 (H, W even): Hs = H / 2, Ws = W / 2 and tap (y, x) of the upsampled plane reads
 *         source pixel (y >> 1, x >> 1), the zero border decided in upsampled coordinates: conv(nearest 2x upsample(x)).
 *       ksize 1: A is x, H * W rows of cin per image (a linear layer: H = rows, W = 1); image i reads x + i * x_img_stride
 *         (elements; 0 = the same rows for every image).  ksize 3 needs x_img_stride = Hs * Ws * cin.
 *     out_kind VAE_OUT_F16: fp16 rows of stride ldo >= cout, pixel-major (NHWC); residual (optional) is fp16 in the same
 *       layout.  VAE_OUT_F32: fp32 rows of stride ldo (the attention scores).  VAE_OUT_F16_NCHW: (n, cout, H, W) fp16 (the
 *       image; ldo = cout).  bias (optional, fp32): per output channel, or with bias_rows = 1 (ksize 1) per row of the image.
 *     cin % 32 == 0; any cout (a ragged last column tile reads zero weights and stores nothing beyond cout).
 *     With VAE_ELEM_BF16 OR-ed into out_kind, x, W and residual are bf16 on v_mfma_f32_32x32x16_bf16 and the 16-bit outputs
 *     bf16 (the UNet's resnet blocks of bf16 pipelines); bias and VAE_OUT_F32 stay fp32.
 *   vae_groupnorm_workspace_bytes / vae_groupnorm : GroupNorm(32, C, eps) [+ SiLU] on x (n, P, C) fp16, C in {128, 256, 512}
 *     -> y fp16.  Statistics as midas_groupnorm_stats: fp64 partial sums per workgroup of 256 pixels, a second launch adds
 *     them in chunk order; the third launch applies in fp32.
 *   vae_softmax : p[r, c] = softmax_c(scale * s[r, c]) for c < Lk, 0 for Lk <= c < ld_out; s fp32 rows of stride ld_in, p
 *     fp16 rows of stride ld_out; the row maximum is subtracted first, the sum is fp32.  scale > 0.
 *
 * FRESCO_EINVAL: null pointers, non-positive sizes, strides smaller than a row, rows read in 16-byte pieces not 16-byte
 * aligned, an option outside its form (up2 or a ksize-3 x_img_stride that is not the plane; bias_rows with ksize 3; a
 * residual with another out_kind).  FRESCO_EUNSUPPORTED: ksize outside {1, 3}, cin % 32, odd H or W with up2, C outside
 * the list, more than 65535 images, a pixel count or a workgroup count that does not fit 31 bits (pixels are indexed in
 * int32, element offsets in int64).  FRESCO_EWORKSPACE: a short workspace.  All before any HIP call.
 */
#ifndef FRESCO_VAE_H
#define FRESCO_VAE_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VAE_OUT_F16 0
#define VAE_OUT_F32 1
#define VAE_OUT_F16_NCHW 2
/* OR-ed into vae_conv's out_kind: x, w and residual are bf16 instead of fp16, on v_mfma_f32_32x32x16_bf16, and VAE_OUT_F16 /
 * VAE_OUT_F16_NCHW then mean bf16 output ("16-bit, the operands' type"); bias stays fp32 and VAE_OUT_F32 stays fp32.  Strides
 * are in elements of 2 bytes either way.  Every check answers as without the bit; any other bit is FRESCO_EINVAL.  Only
 * vae_conv takes it: the other vae_* functions are fp16. */
#define VAE_ELEM_BF16 0x100

int vae_input(const void* z, const float* weight, const float* bias, void* out, int n, int h, int w, int cpad, void* stream);
int vae_conv(const void* x, int64_t x_img_stride, const void* w, int64_t w_img_stride, const float* bias /* may be NULL */,
             const void* residual /* may be NULL */, void* out, int n, int H, int W, int cin, int cout, int ksize, int up2,
             int out_kind, int bias_rows, int64_t ldo, void* stream);
size_t vae_groupnorm_workspace_bytes(int n, int P, int C);
int vae_groupnorm(const void* x, const float* gamma, const float* beta, void* y, void* workspace, size_t workspace_bytes, int n,
                  int P, int C, float eps, int silu, void* stream);
int vae_softmax(const float* s, void* p, int64_t rows, int Lk, int64_t ld_in, int64_t ld_out, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_VAE_H */
