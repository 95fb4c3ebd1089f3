// The VAE decoder of fp16 pipelines (diffusers AutoencoderKL.decode, SD-1.5 VAE): include/fresco_vae.h, DESIGN.md section 17.
//
//   vae_input_kernel       latents NCHW fp16 -> post_quant_conv (4 -> 4, fp32) -> fp16 NHWC rows padded to conv_in's K chunk
//   vae_conv_kernel<9>     3 x 3, stride 1, pad 1 implicit-GEMM convolution, optionally through a nearest 2x upsample
//   vae_conv_kernel<1>     1 x 1 / linear form; per-image weight matrices (Q K^T, P V) and a per-row bias (V^T) as options
//   gn_stats_kernel<half_t> / gn_finish_kernel (groupnorm_stats.h, shared with midas.hip) / vae_gn_apply_kernel
//                          GroupNorm(32) [+ SiLU], fp64 statistics
//   vae_softmax_kernel     fp32 scores -> fp16 probabilities, one workgroup per row
//
// vae_conv_kernel: conv_tile.h's fp16 implicit-GEMM tile (operands, wave layout, weight ring, XCD deal, epilogue map) with the
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
#include "groupnorm_stats.h"
#include "../../include/fresco_vae.h"

namespace fresco {

constexpr int VA_GROUPS = GN_GROUPS;
constexpr int VC_WW = CT_TW + 2, VC_NPOS = (CT_TH + 2) * VC_WW;
constexpr int VC_A_BYTES = 12 * 1024;  // 12 pieces of 64 lanes x 16 bytes = 192 window rows of 64 bytes (180 used)
constexpr int VC_LDS = 2 * VC_A_BYTES + 2 * CT_B_BYTES;

struct VaeConv {
    const half_t* x;
    const half_t* w;
    const float* bias;
    const half_t* res;
    void* out;
    int64_t x_img_stride, w_img_stride, ldo;
    int n, H, W, Hs, Ws, rows;  // rows = H W, the output pixels per image
    int cin, cout, up2, out_kind, bias_rows;
    int tiles_x, tiles_per_img;
};

template <int TAPS>
__device__ __forceinline__ int vc_swizzle(int P) {
    return TAPS == 9 ? ((P / VC_WW + 2 * (P >> 2)) & 3) : ((P >> 2) & 3);
}

template <int TAPS>
__global__ __launch_bounds__(256) void vae_conv_kernel(const VaeConv a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int APW = TAPS == 9 ? 3 : 2;  // window pieces per wave
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const CtTile t = ct_deal(a.n, a.tiles_per_img);
    const int img = t.img, t_in = t.t_in;
    const int co0 = t.col_tile * CT_BN;
    const int ty0 = TAPS == 9 ? (t_in / a.tiles_x) * CT_TH : 0;
    const int tx0 = TAPS == 9 ? (t_in % a.tiles_x) * CT_TW : 0;
    const int m0 = t_in * CT_BM;
    const uint32_t lds0 = lds_addr(smem);
    const char* zp = reinterpret_cast<const char*>(ct_zero_page);

    // ---- DMA sources: a lane owns LDS piece (slot & 3) of window row slot >> 2 and fetches source piece (slot & 3) ^ swizzle(row)
    const char* a_src[APW];
#pragma unroll
    for (int p = 0; p < APW; ++p) {
        const int slot = (wave * APW + p) * 64 + lane;
        const int P = slot >> 2;
        const int pc = (slot & 3) ^ vc_swizzle<TAPS>(P);
        bool ok;
        int64_t off;
        if (TAPS == 9) {
            const int wy = P / VC_WW, wx = P - wy * VC_WW;
            const int y = ty0 + wy - 1, x = tx0 + wx - 1;
            ok = P < VC_NPOS && y >= 0 && y < a.H && x >= 0 && x < a.W;
            off = ((int64_t)(y >> a.up2) * a.Ws + (x >> a.up2)) * a.cin;
        } else {
            ok = P < CT_BM && m0 + P < a.rows;
            off = (int64_t)(m0 + P) * a.cin;
        }
        a_src[p] = ok ? reinterpret_cast<const char*>(a.x + (int64_t)img * a.x_img_stride + off + pc * 8) : nullptr;
    }
    const char* b_src[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int R, pc;
        ct_gemm_slot(wave, p, lane, R, pc);
        b_src[p] = ct_weight_src(a.w + (int64_t)img * a.w_img_stride, co0, R, pc, a.cout, TAPS * a.cin);
    }
    auto issue_a = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < APW; ++p)
            lds_dma16(a_src[p] ? static_cast<const void*>(a_src[p] + (int64_t)chunk * (CT_BK * 2)) : static_cast<const void*>(zp),
                      lds0 + (uint32_t)((chunk & 1) * VC_A_BYTES + (wave * APW + p) * 1024));
    };
    const uint32_t lds_b = lds0 + 2 * VC_A_BYTES;

    const int nbv = ct_live_blocks(a.cout, co0, wn);
    floatx16 acc[2][2] = {};  // [channel block j][pixel block i]

    const int chunks = a.cin / CT_BK, steps = chunks * TAPS;
    const int wsw = (l31 >> 2) & 3;
    issue_a(0);
    ct_issue_weights(b_src, 0, 0, lds_b, wave);
    int chunk = 0, tap = 0;
    for (int s = 0; s < steps; ++s) {
        dma_wait_barrier<0>();
        if (s + 1 < steps) {
            const int t1 = tap + 1 == TAPS ? 0 : tap + 1, c1 = tap + 1 == TAPS ? chunk + 1 : chunk;
            ct_issue_weights(b_src, s + 1, t1 * a.cin + c1 * CT_BK, lds_b, wave);
            if (tap == 0 && chunk + 1 < chunks) issue_a(chunk + 1);
        }
        const int ky = tap / 3, kx = tap - ky * 3;
        const char* pa = smem + (chunk & 1) * VC_A_BYTES;
        const char* pb = smem + 2 * VC_A_BYTES + (s & 1) * CT_B_BYTES + (wn * 64 + l31) * 64;
        int aoff[2], asw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = ct_row(wm, i, l31);
            const int P = TAPS == 9 ? ((r >> 4) + ky) * VC_WW + (r & 15) + kx : r;
            aoff[i] = P * 64;
            asw[i] = vc_swizzle<TAPS>(P);
        }
#pragma unroll
        for (int ks = 0; ks < CT_BK / 16; ++ks) {
            const int piece = ks * 2 + hi;
            half8_t px[2], wt[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) px[i] = *reinterpret_cast<const half8_t*>(pa + aoff[i] + ((piece ^ asw[i]) * 16));
#pragma unroll
            for (int j = 0; j < 2; ++j) wt[j] = *reinterpret_cast<const half8_t*>(pb + j * 32 * 64 + ((piece ^ wsw) * 16));
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j < nbv) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[j], px[i], acc[j][i], 0, 0, 0);
                }
        }
        if (++tap == TAPS) {
            tap = 0;
            ++chunk;
        }
    }

    // ---- epilogue (conv_tile.h's map).  Every address and every residual is read before the first store.
    int64_t opix[2];   // pixel index over all images, -1: outside the problem
    int orow[2];       // the pixel's index inside its image
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = ct_row(wm, i, l31);
        if (TAPS == 9) {
            const int y = ty0 + (r >> 4), x = tx0 + (r & 15);
            orow[i] = y * a.W + x;
            opix[i] = (y < a.H && x < a.W) ? (int64_t)img * a.rows + orow[i] : -1;
        } else {
            orow[i] = m0 + r;
            opix[i] = orow[i] < a.rows ? (int64_t)img * a.rows + orow[i] : -1;
        }
    }
    const bool vec = a.out_kind == VAE_OUT_F16 && !(a.cout & 3) && !(a.ldo & 3);
    if (vec) {
        half_t* out = static_cast<half_t*>(a.out);
        half4_t rs[2][2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = ct_channel(co0, wn, j, hi, 4 * g);
                    half4_t z4 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
                    rs[j][i][g] = (a.res && opix[i] >= 0 && co < a.cout)
                                      ? *reinterpret_cast<const half4_t*>(a.res + opix[i] * a.ldo + co)
                                      : z4;
                }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = ct_channel(co0, wn, j, hi, 4 * g);
                if (co >= a.cout) continue;
                floatx4 bv = {0.f, 0.f, 0.f, 0.f};
                if (a.bias && !a.bias_rows) bv = *reinterpret_cast<const floatx4*>(a.bias + co);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (opix[i] < 0) continue;
                    const float br = (a.bias && a.bias_rows) ? a.bias[orow[i]] : 0.f;
                    half4_t o4;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        o4[e] = (half_t)(acc[j][i][4 * g + e] + (bv[e] + br) + (float)rs[j][i][g][e]);
                    *reinterpret_cast<half4_t*>(out + opix[i] * a.ldo + co) = o4;
                }
            }
    } else {
        // ragged channel counts, fp32 rows and the NCHW image: one element per store
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (opix[i] < 0) continue;
                const float br = (a.bias && a.bias_rows) ? a.bias[orow[i]] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct_channel(co0, wn, j, hi, r);
                    if (co >= a.cout) continue;
                    float v = acc[j][i][r] + ((a.bias && !a.bias_rows) ? a.bias[co] : 0.f) + br;
                    if (a.out_kind == VAE_OUT_F32) {
                        static_cast<float*>(a.out)[opix[i] * a.ldo + co] = v;
                    } else if (a.out_kind == VAE_OUT_F16_NCHW) {
                        static_cast<half_t*>(a.out)[((int64_t)img * a.cout + co) * a.rows + orow[i]] = (half_t)v;
                    } else {
                        if (a.res) v += (float)a.res[opix[i] * a.ldo + co];
                        static_cast<half_t*>(a.out)[opix[i] * a.ldo + co] = (half_t)v;
                    }
                }
            }
    }
}

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
    a.x = static_cast<const half_t*>(x);
    a.w = static_cast<const half_t*>(w);
    a.bias = bias;
    a.res = static_cast<const half_t*>(residual);
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
    if (ksize == 3)
        hipLaunchKernelGGL(vae_conv_kernel<9>, dim3(grid), dim3(256), VC_LDS, as_stream(stream), a);
    else
        hipLaunchKernelGGL(vae_conv_kernel<1>, dim3(grid), dim3(256), VC_LDS, as_stream(stream), a);
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
