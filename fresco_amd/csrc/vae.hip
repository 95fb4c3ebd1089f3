// The VAE decoder of fp16 pipelines (diffusers AutoencoderKL.decode, SD-1.5 VAE): include/fresco_vae.h, DESIGN.md section 17.
//
//   vae_input_kernel       latents NCHW fp16 -> post_quant_conv (4 -> 4, fp32) -> fp16 NHWC rows padded to conv_in's K chunk
//   vae_conv_kernel<9>     3 x 3, stride 1, pad 1 implicit-GEMM convolution, optionally through a nearest 2x upsample
//   vae_conv_kernel<1>     1 x 1 / linear form; per-image weight matrices (Q K^T, P V) and a per-row bias (V^T) as options
//   gn_stats_kernel<half_t> / gn_finish_kernel (groupnorm_stats.h, shared with midas.hip) / vae_gn_apply_kernel
//                          GroupNorm(32) [+ SiLU], fp64 statistics
//   vae_softmax_kernel     fp32 scores -> fp16 probabilities, one workgroup per row
//
// vae_conv_kernel (its text: vae_conv_body.h, a template over the element type; this file launches the fp16 form, net_bf16.hip
// the bf16 form that vae_conv's VAE_ELEM_BF16 flag selects): conv_tile.h's fp16 implicit-GEMM tile (operands, wave layout, weight ring, XCD deal, epilogue map) with the
// tile's pixels held as an input WINDOW.  The fp16 NHWC result leaves as 8-byte stores, the NCHW image as stores that run
// along x.  LDS (dynamic, 40 KiB):
//   * two slots of 12 KiB for the input WINDOW of the tile, 32 channels deep: 3 x 3: the 10 x 18 pixels around the
//     8 x 16 tile (180 rows of 64 bytes, fetched ONCE per chunk and read by all nine taps: tap (ky, kx) of tile pixel
//     (ty, tx) is window row (ty + ky) 18 + tx + kx); 1 x 1: the tile's 128 rows.  Pixels outside the image and rows past
//     the problem come from the zero page.  up2 changes only the window's source addresses.
//   * conv_tile.h's two weight slots of 8 KiB.
// Everything arrives by LDS-DMA (lds_dma.h).  Step s: every wave waits for its own copies (all of them: vmcnt(0)), barrier
// -- step s is in LDS and step s - 1 has been read -- then the weights of step s + 1 and, at a chunk's first tap, the
// next chunk's window are issued into the other slots and fly under the MFMAs of step s.  A window row's four 16-byte
// pieces sit at piece ^ swizzle(row): flownet.hip's (py + 2 (P >> 2)) & 3 for the 18-wide window, the GEMM rows' map at 1 x 1.
#include "common.h"
#include "lds_dma.h"
#include "conv_tile.h"
#include "vae_conv_body.h"
#include "groupnorm_stats.h"
#include "../../include/fresco_vae.h"

namespace fresco {

constexpr int VA_GROUPS = GN_GROUPS;
constexpr int VC_LDS = 2 * VC_A_BYTES + 2 * CT_B_BYTES;



// One thread per latent pixel.
__global__ __launch_bounds__(256) void vae_input_kernel(const half_t* __restrict__ z, const float* __restrict__ wq,
                                                        const float* __restrict__ bq, half_t* __restrict__ out, int n, int hw,
                                                        int cpad) {
    const int64_t total = (int64_t)n * hw;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t img = idx / hw, p = idx - img * hw;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (float)z[(img * 4 + c) * hw + p];
        half8_t o8;
#pragma unroll
        for (int e = 0; e < 8; ++e) o8[e] = (half_t)0.f;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float s = bq[o];
#pragma unroll
            for (int c = 0; c < 4; ++c) s += wq[o * 4 + c] * v[c];
            o8[o] = (half_t)s;
        }
        ct_store_padded_row(out + idx * cpad, o8, cpad);
    }
}

// One thread per (pixel, eight channels); grid (blocks, n).  C is a power of two, so item idx of an image is its elements
// 8 idx .. 8 idx + 7, channel 8 (idx & (C / 8 - 1)): shifts, no division (the first version divided int64 indices three
// times per item and ran at a fifth of this one's rate).
__global__ __launch_bounds__(256) void vae_gn_apply_kernel(const half_t* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, half_t* __restrict__ y,
                                                           int64_t per_img, int C, int lcpg, int silu) {
    const int img = blockIdx.y;
    const half_t* xi = x + (int64_t)img * per_img * 8;
    half_t* yi = y + (int64_t)img * per_img * 8;
    const float* mi = mean + img * VA_GROUPS;
    const float* ri = rstd + img * VA_GROUPS;
    const int qmask = (C >> 3) - 1;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < per_img; idx += (int64_t)gridDim.x * 256) {
        const int c = ((int)idx & qmask) * 8;
        const half8_t v8 = *reinterpret_cast<const half8_t*>(xi + idx * 8);
        const floatx4 g0 = *reinterpret_cast<const floatx4*>(gamma + c), g1 = *reinterpret_cast<const floatx4*>(gamma + c + 4);
        const floatx4 b0 = *reinterpret_cast<const floatx4*>(beta + c), b1 = *reinterpret_cast<const floatx4*>(beta + c + 4);
        half8_t o8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int g = (c + e) >> lcpg;
            float v = ((float)v8[e] - mi[g]) * ri[g] * (e < 4 ? g0[e & 3] : g1[e & 3]) + (e < 4 ? b0[e & 3] : b1[e & 3]);
            if (silu) v = v / (1.f + expf(-v));
            o8[e] = (half_t)v;
        }
        *reinterpret_cast<half8_t*>(yi + idx * 8) = o8;
    }
}

__device__ __forceinline__ float block_max_256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// One workgroup per row: the maximum, the fp32 sum of exp(scale (s - max)), then the fp16 quotients (and the zero tail).
__global__ __launch_bounds__(256) void vae_softmax_kernel(const float* __restrict__ s, half_t* __restrict__ p, int Lk,
                                                          int64_t ld_in, int64_t ld_out, float scale) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const float* sr = s + (int64_t)blockIdx.x * ld_in;
    half_t* pr = p + (int64_t)blockIdx.x * ld_out;
    float m = -INFINITY;
    for (int c = tid; c < Lk; c += 256) m = fmaxf(m, sr[c]);
    m = block_max_256(m, red);
    float sum = 0.f;
    for (int c = tid; c < Lk; c += 256) sum += expf((sr[c] - m) * scale);
    sum = block_sum_256(sum, red);
    for (int c = tid; c < ld_out; c += 256) pr[c] = c < Lk ? (half_t)(expf((sr[c] - m) * scale) / sum) : (half_t)0.f;
}

static inline bool va_gn_channels(int C) { return C == 128 || C == 256 || C == 512; }

}  // namespace fresco

using namespace fresco;

extern "C" int vae_input(const void* z, const float* weight, const float* bias, void* out, int n, int h, int w, int cpad,
                         void* stream) {
    if (!z || !weight || !bias || !out || n <= 0 || h <= 0 || w <= 0) return FRESCO_EINVAL;
    if (cpad < 8 || cpad > 64 || cpad % 8) return FRESCO_EINVAL;
    if (!aligned_to(z, 2) || !aligned_to(weight, 4) || !aligned_to(bias, 4) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    if ((int64_t)n * h * w >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(vae_input_kernel, dim3(stream_blocks((int64_t)n * h * w)), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t*>(z), weight, bias, static_cast<half_t*>(out), n, h * w, cpad);
    return check_launch();
}

extern "C" int vae_conv(const void* x, int64_t x_img_stride, const void* w, int64_t w_img_stride, const float* bias,
                        const void* residual, void* out, int n, int H, int W, int cin, int cout, int ksize, int up2,
                        int out_kind, int bias_rows, int64_t ldo, void* stream) {
    if (!x || !w || !out || n <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0) return FRESCO_EINVAL;
    const bool bf16 = (out_kind & VAE_ELEM_BF16) != 0;  // the operands' type; what is left is the output kind, checked as ever
    out_kind &= ~VAE_ELEM_BF16;
    if (out_kind != VAE_OUT_F16 && out_kind != VAE_OUT_F32 && out_kind != VAE_OUT_F16_NCHW) return FRESCO_EINVAL;
    if (ksize != 1 && ksize != 3) return FRESCO_EUNSUPPORTED;
    if (!ct_supported(n, H, W, cin) || (up2 && (H % 2 || W % 2))) return FRESCO_EUNSUPPORTED;
    up2 = up2 ? 1 : 0;
    bias_rows = bias_rows ? 1 : 0;
    const int Hs = H >> up2, Ws = W >> up2;
    if (ksize == 1 && up2) return FRESCO_EINVAL;
    if (ksize == 3 && (bias_rows || x_img_stride != (int64_t)Hs * Ws * cin)) return FRESCO_EINVAL;
    if (x_img_stride < 0 || w_img_stride < 0 || x_img_stride % 8 || w_img_stride % 8) return FRESCO_EINVAL;
    if (residual && out_kind != VAE_OUT_F16) return FRESCO_EINVAL;
    if (ldo < cout || (out_kind == VAE_OUT_F16_NCHW && ldo != cout)) return FRESCO_EINVAL;
    if (!aligned_to(x, 16) || !aligned_to(w, 16) || !aligned_to(bias, 16) || !aligned_to(residual, 8)) return FRESCO_EINVAL;
    if (!aligned_to(out, out_kind == VAE_OUT_F32 ? 4 : 8)) return FRESCO_EINVAL;
    VaeConv a;
    a.x = x;
    a.w = w;
    a.bias = bias;
    a.res = residual;
    a.out = out;
    a.x_img_stride = x_img_stride;
    a.w_img_stride = w_img_stride;
    a.ldo = ldo;
    a.n = n;
    a.H = H;
    a.W = W;
    a.Hs = Hs;
    a.Ws = Ws;
    a.rows = H * W;
    a.cin = cin;
    a.cout = cout;
    a.up2 = up2;
    a.out_kind = out_kind;
    a.bias_rows = bias_rows;
    a.tiles_x = ksize == 3 ? ct_tiles_x(W) : 1;
    a.tiles_per_img = ksize == 3 ? ct_plane_tiles(H, W) : (int)(((int64_t)a.rows + CT_BM - 1) / CT_BM);
    const unsigned grid = ct_grid(n, a.tiles_per_img, cout);
    if (!grid) return FRESCO_EUNSUPPORTED;
    if (bf16) return vae_conv_launch_bf16(a, ksize, grid, as_stream(stream));
    if (ksize == 3)
        hipLaunchKernelGGL((vae_conv_kernel<9, half_t>), dim3(grid), dim3(256), VC_LDS, as_stream(stream), a);
    else
        hipLaunchKernelGGL((vae_conv_kernel<1, half_t>), dim3(grid), dim3(256), VC_LDS, as_stream(stream), a);
    return check_launch();
}

extern "C" size_t vae_groupnorm_workspace_bytes(int n, int P, int C) {
    if (n <= 0 || P <= 0 || !va_gn_channels(C)) return 0;
    return gn_workspace_bytes(n, P, true);
}

extern "C" int vae_groupnorm(const void* x, const float* gamma, const float* beta, void* y, void* workspace,
                             size_t workspace_bytes, int n, int P, int C, float eps, int silu, void* stream) {
    if (!x || !gamma || !beta || !y || !workspace || n <= 0 || P <= 0 || C <= 0 || !(eps >= 0.f)) return FRESCO_EINVAL;
    if (!va_gn_channels(C)) return FRESCO_EUNSUPPORTED;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(y, 16) || !aligned_to(workspace, 8) || !aligned_to(gamma, 16) || !aligned_to(beta, 16))
        return FRESCO_EINVAL;
    if (workspace_bytes < vae_groupnorm_workspace_bytes(n, P, C)) return FRESCO_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    float *mean = nullptr, *rstd = nullptr;  // (in the workspace, behind the partial sums)
    if (int rc = gn_statistics(static_cast<const half_t*>(x), workspace, mean, rstd, n, P, C, eps, st)) return rc;
    const int64_t per_img = (int64_t)P * (C / 8);
    const int lcpg = C == 128 ? 2 : (C == 256 ? 3 : 4);  // log2(C / 32)
    hipLaunchKernelGGL(vae_gn_apply_kernel, dim3(stream_blocks(per_img), n), dim3(256), 0, st, static_cast<const half_t*>(x), mean,
                       rstd, gamma, beta, static_cast<half_t*>(y), per_img, C, lcpg, silu ? 1 : 0);
    return check_launch();
}

extern "C" int vae_softmax(const float* s, void* p, int64_t rows, int Lk, int64_t ld_in, int64_t ld_out, float scale,
                           void* stream) {
    if (!s || !p || rows <= 0 || Lk <= 0 || ld_in < Lk || ld_out < Lk || !(scale > 0.f)) return FRESCO_EINVAL;
    if (!aligned_to(s, 4) || !aligned_to(p, 2)) return FRESCO_EINVAL;
    if (rows >= (int64_t)1 << 31 || ld_out >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(vae_softmax_kernel, dim3((unsigned)rows), dim3(256), 0, as_stream(stream), s, static_cast<half_t*>(p), Lk,
                       ld_in, ld_out, scale);
    return check_launch();
}
