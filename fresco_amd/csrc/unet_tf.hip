// What a UNet Transformer2DModel of fp16 pipelines needs beside unet_groupnorm and vae_conv: include/fresco_unet_tf.h,
// DESIGN.md section 20.
//
//   unet_ln_kernel<NP>   y = LayerNorm(C, eps)(x [+ r]) gamma + beta, and optionally sum_out = x + r: one launch, rows read once
//   unet_geglu_kernel    out = (x Wv^T + bv) * gelu(x Wg^T + bg) on conv_tile.h's tile: the (M, 2 inner) projection is never
//                        written
//
// unet_ln_kernel.  256 threads = four waves; ONE WAVE PER ROW, and a wave walks rows gw, gw + waves, ... of the grid (at most
// UL_MAX_BLOCKS workgroups), so gamma and beta (fp32: twice a row's bytes) are loaded once per wave and stay in registers.
// A row is C / 8 <= 320 pieces of 16 bytes; lane l owns pieces l, l + 64, ..: NP = ceil(C / 512) of them (1 .. 5; at C = 320
// the 40 pieces are fewer than the lanes, at 1280 the 160 are 2.5 per lane).  x [+ r] is summed in fp32 ONCE and kept: 8 NP
// registers.  SUMMATION ORDER (fixed; no atomics): a lane adds its values to one fp64 (sum, sum of squares) in piece order
// and element order; the 64 lanes are folded by an xor butterfly (32, 16, .., 1), whose two partners add the same two
// numbers, so every lane ends with the same bits.  mean and rstd as unet.hip's ug_mean_rstd; the normalisation is fp32 from
// the fp32 sum, one rounding to fp16; sum_out is that fp32 sum rounded once.
//
// unet_geglu_kernel.  vae_conv_kernel<1>'s main loop (vae.hip) on conv_tile.h's tile with the rows flat: the tile's 128 rows
// are rows m0 .. m0 + 127 of ALL images' tokens.  LDS (static, 32 KiB): two slots of 8 KiB for the tile's 128 rows of x, 32
// columns deep, and conv_tile.h's two weight slots of 8 KiB; the same ring (step s: wait, barrier, issue step s + 1, MFMAs).
// WEIGHT ORDER: the packed (2 inner, K) matrix goes in blocks of 64 rows, the 32 value rows of channels 32 b .. 32 b + 31
// and then their 32 gate rows (unet_transformer.py's pack_geglu_weight), the bias likewise.  A wave's channel block j = 0 is
// then the values and j = 1 the gates of the SAME 32 channels: acc[0][i][r] and acc[1][i][r] of one lane are a pair, and the
// epilogue computes (v + bv) * gelu(g + bg) in fp32, rounds ONCE, and stores four consecutive channels as 8 bytes.  A
// 128-row column tile of packed weights is 64 output channels; 2 inner is a multiple of 64, so a wave's pair block is live
// or dead as a whole.  The GELU is the exact one, 0.5 g (1 + erf(g / sqrt 2)).
// No split-K, no atomics: same inputs, same bits.
#include "common.h"
#include "lds_dma.h"
#include "conv_tile.h"
#include "../../include/fresco_unet_tf.h"

namespace fresco {

constexpr int UL_THREADS = 256;
constexpr int UL_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups
constexpr int UL_CMIN = 64, UL_CMAX = 2560;
constexpr int UF_A_BYTES = 8 * 1024;  // the tile's 128 rows of 64 bytes
constexpr int UF_LDS = 2 * UF_A_BYTES + 2 * CT_B_BYTES;

struct UlArgs {
    const half_t* x;
    const half_t* r;
    const float* gamma;
    const float* beta;
    half_t* y;
    half_t* sum_out;
    int64_t ldx, ldr, ldy, lds;
    int rows, C;
    float eps;
};

__device__ __forceinline__ double ul_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (min(ceil(rows / 4), UL_MAX_BLOCKS)); wave gw of the grid: rows gw, gw + waves, ...
template <int NP>
__global__ __launch_bounds__(UL_THREADS) void unet_ln_kernel(const UlArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int npieces = a.C >> 3;
    const int waves = gridDim.x * (UL_THREADS / 64);
    floatx4 ga[NP][2], be[NP][2];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = lane + 64 * i;
        const floatx4 z = {0.f, 0.f, 0.f, 0.f};
        ga[i][0] = ga[i][1] = be[i][0] = be[i][1] = z;
        if (p < npieces) {
            ga[i][0] = *reinterpret_cast<const floatx4*>(a.gamma + p * 8);
            ga[i][1] = *reinterpret_cast<const floatx4*>(a.gamma + p * 8 + 4);
            be[i][0] = *reinterpret_cast<const floatx4*>(a.beta + p * 8);
            be[i][1] = *reinterpret_cast<const floatx4*>(a.beta + p * 8 + 4);
        }
    }
    for (int64_t row = blockIdx.x * (UL_THREADS / 64) + wave; row < a.rows; row += waves) {
        float v[NP][8];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = lane + 64 * i;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
            if (p < npieces) {
                const half8_t x8 = *reinterpret_cast<const half8_t*>(a.x + row * a.ldx + p * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] = (float)x8[e];
                if (a.r) {
                    const half8_t r8 = *reinterpret_cast<const half8_t*>(a.r + row * a.ldr + p * 8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[i][e] += (float)r8[e];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) {   // (pieces >= npieces hold zeros: they add nothing)
                const double d = (double)v[i][e];
                s1 += d;
                s2 += d * d;
            }
        s1 = ul_wave_sum(s1);
        s2 = ul_wave_sum(s2);
        const double m = s1 / (double)a.C;
        double var = s2 / (double)a.C - m * m;
        var = var > 0.0 ? var : 0.0;
        const float mean = (float)m, rstd = (float)(1.0 / sqrt(var + (double)a.eps));
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = lane + 64 * i;
            if (p >= npieces) continue;
            half8_t o8;
#pragma unroll
            for (int e = 0; e < 8; ++e) o8[e] = (half_t)((v[i][e] - mean) * rstd * ga[i][e >> 2][e & 3] + be[i][e >> 2][e & 3]);
            *reinterpret_cast<half8_t*>(a.y + row * a.ldy + p * 8) = o8;
            if (a.sum_out) {
                half8_t s8;
#pragma unroll
                for (int e = 0; e < 8; ++e) s8[e] = (half_t)v[i][e];
                *reinterpret_cast<half8_t*>(a.sum_out + row * a.lds + p * 8) = s8;
            }
        }
    }
}

struct UfArgs {
    const half_t* x;
    const half_t* w;
    const float* bias;
    half_t* out;
    int64_t ldo;
    int M, K, inner, tiles;
};

__device__ __forceinline__ float uf_gelu(float g) { return 0.5f * g * (1.f + erff(g * 0.70710678118654752f)); }

__global__ __launch_bounds__(256) void unet_geglu_kernel(const UfArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[UF_LDS];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const CtTile t = ct_deal(1, a.tiles);
    const int co0 = t.col_tile * CT_BN;  // the first PACKED weight row of the column tile
    const int m0 = t.t_in * CT_BM;
    const int cout = 2 * a.inner;
    const uint32_t lds0 = lds_addr(smem);
    const char* zp = reinterpret_cast<const char*>(ct_zero_page);

    // ---- DMA sources: a lane owns LDS piece (slot & 3) of tile row slot >> 2 and fetches source piece (slot & 3) ^ swizzle(row)
    const char* a_src[2];
    const char* b_src[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int R, pc;
        ct_gemm_slot(wave, p, lane, R, pc);
        a_src[p] = (int64_t)m0 + R < a.M ? reinterpret_cast<const char*>(a.x + ((int64_t)m0 + R) * a.K + pc * 8) : nullptr;
        b_src[p] = ct_weight_src(a.w, co0, R, pc, cout, a.K);
    }
    auto issue_a = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            lds_dma16(a_src[p] ? static_cast<const void*>(a_src[p] + (int64_t)chunk * (CT_BK * 2)) : static_cast<const void*>(zp),
                      lds0 + (uint32_t)((chunk & 1) * UF_A_BYTES + (wave * 2 + p) * 1024));
    };
    const uint32_t lds_b = lds0 + 2 * UF_A_BYTES;

    const int nbv = ct_live_blocks(cout, co0, wn);  // 0 or 2: cout is a multiple of 64
    floatx16 acc[2][2] = {};  // [0: value, 1: gate][row block i]

    const int steps = a.K / CT_BK;
    const int wsw = (l31 >> 2) & 3;
    issue_a(0);
    ct_issue_weights(b_src, 0, 0, lds_b, wave);
    for (int s = 0; s < steps; ++s) {
        dma_wait_barrier<0>();
        if (s + 1 < steps) {
            ct_issue_weights(b_src, s + 1, (s + 1) * CT_BK, lds_b, wave);
            issue_a(s + 1);
        }
        const char* pa = smem + (s & 1) * UF_A_BYTES;
        const char* pb = smem + 2 * UF_A_BYTES + (s & 1) * CT_B_BYTES + (wn * 64 + l31) * 64;
        int aoff[2], asw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = ct_row(wm, i, l31);
            aoff[i] = r * 64;
            asw[i] = (r >> 2) & 3;
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
    }

    // ---- epilogue: registers 4 g .. 4 g + 3 of block 0 / block 1 are the values / gates of four consecutive channels
    if (nbv == 0) return;
    const int oc0 = (co0 + wn * 64) >> 1;  // this wave's first output channel
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int pk = ct_channel(co0, wn, 0, hi, 4 * g);  // the packed row of the value; its gate is 32 rows on
        const int oc = oc0 + 8 * g + 4 * hi;
        const floatx4 bv = *reinterpret_cast<const floatx4*>(a.bias + pk);
        const floatx4 bg = *reinterpret_cast<const floatx4*>(a.bias + pk + 32);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t row = (int64_t)m0 + ct_row(wm, i, l31);
            if (row >= a.M) continue;
            half4_t o4;
#pragma unroll
            for (int e = 0; e < 4; ++e) o4[e] = (half_t)((acc[0][i][4 * g + e] + bv[e]) * uf_gelu(acc[1][i][4 * g + e] + bg[e]));
            *reinterpret_cast<half4_t*>(a.out + row * a.ldo + oc) = o4;
        }
    }
}

}  // namespace fresco

using namespace fresco;

extern "C" int unet_layernorm(const void* x, int64_t ldx, const void* r, int64_t ldr, const float* gamma, const float* beta,
                              void* y, int64_t ldy, void* sum_out, int64_t ld_sum, int64_t rows, int C, float eps, void* stream) {
    if (!x || !gamma || !beta || !y || rows <= 0 || C <= 0 || !(eps >= 0.f)) return FRESCO_EINVAL;
    if (C % 8 || C < UL_CMIN || C > UL_CMAX || rows >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (ldx < C || ldx % 8 || ldy < C || ldy % 8) return FRESCO_EINVAL;
    if (r && (ldr < C || ldr % 8)) return FRESCO_EINVAL;
    if (sum_out && (ld_sum < C || ld_sum % 8)) return FRESCO_EINVAL;
    if (!aligned_to(x, 16) || !aligned_to(r, 16) || !aligned_to(y, 16) || !aligned_to(sum_out, 16) || !aligned_to(gamma, 16) ||
        !aligned_to(beta, 16))
        return FRESCO_EINVAL;
    UlArgs a;
    a.x = static_cast<const half_t*>(x);
    a.r = static_cast<const half_t*>(r);
    a.gamma = gamma;
    a.beta = beta;
    a.y = static_cast<half_t*>(y);
    a.sum_out = static_cast<half_t*>(sum_out);
    a.ldx = ldx;
    a.ldr = ldr;
    a.ldy = ldy;
    a.lds = ld_sum;
    a.rows = (int)rows;
    a.C = C;
    a.eps = eps;
    const int64_t blocks = (rows + UL_THREADS / 64 - 1) / (UL_THREADS / 64);
    const dim3 grid((unsigned)(blocks < UL_MAX_BLOCKS ? blocks : UL_MAX_BLOCKS));
    const int np = (C / 8 + 63) / 64;
    hipStream_t st = as_stream(stream);
    switch (np) {
        case 1: hipLaunchKernelGGL(unet_ln_kernel<1>, grid, dim3(UL_THREADS), 0, st, a); break;
        case 2: hipLaunchKernelGGL(unet_ln_kernel<2>, grid, dim3(UL_THREADS), 0, st, a); break;
        case 3: hipLaunchKernelGGL(unet_ln_kernel<3>, grid, dim3(UL_THREADS), 0, st, a); break;
        case 4: hipLaunchKernelGGL(unet_ln_kernel<4>, grid, dim3(UL_THREADS), 0, st, a); break;
        default: hipLaunchKernelGGL(unet_ln_kernel<5>, grid, dim3(UL_THREADS), 0, st, a); break;
    }
    return check_launch();
}

extern "C" int unet_geglu(const void* x, const void* w, const float* bias, void* out, int64_t M, int K, int inner, int64_t ldo,
                          void* stream) {
    if (!x || !w || !bias || !out || M <= 0 || K <= 0 || inner <= 0) return FRESCO_EINVAL;
    if (K % CT_BK || inner % 32 || M >= (int64_t)1 << 31 || inner >= 1 << 29) return FRESCO_EUNSUPPORTED;
    if (ldo < inner || ldo % 4) return FRESCO_EINVAL;
    if (!aligned_to(x, 16) || !aligned_to(w, 16) || !aligned_to(bias, 16) || !aligned_to(out, 8)) return FRESCO_EINVAL;
    UfArgs a;
    a.x = static_cast<const half_t*>(x);
    a.w = static_cast<const half_t*>(w);
    a.bias = bias;
    a.out = static_cast<half_t*>(out);
    a.ldo = ldo;
    a.M = (int)M;
    a.K = K;
    a.inner = inner;
    a.tiles = (int)((M + CT_BM - 1) / CT_BM);
    const unsigned grid = ct_grid(1, a.tiles, 2 * inner);
    if (!grid) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(unet_geglu_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a);
    return check_launch();
}
