// vae_conv_kernel<TAPS, T> (vae.hip's header comment describes it) as ONE text for both 16-bit element types: vae.hip
// instantiates and launches vae_conv_kernel<TAPS, half_t>, net_bf16.hip vae_conv_kernel<TAPS, bf16_t>.
// On gfx950 v_mfma_f32_32x32x16_f16 and v_mfma_f32_32x32x16_bf16 share operand and accumulator lane maps and both types
// have 2-byte elements, so the window, the swizzles, the LDS-DMA and the packed weight image are byte-identical: what the
// type changes is the fragment types, the MFMA (Elem<T>::mfma32x32x16) and every conversion of the epilogue (one rounding to
// nearest even at the store in both).  VAE_OUT_F16 and VAE_OUT_F16_NCHW mean "16-bit, the operands' type".
//
// The kernel itself is the template, NOT a wrapper around a forceinline body: with a body taken by reference hipcc scheduled
// the fp16 kernels differently (same register counts, another instruction order), and conv_tile.h records what a factored
// MFMA step cost.  As a template the fp16 instantiations have the instruction streams they had when this text stood in
// vae.hip, line for line (DESIGN.md section 19 records the comparison).
#pragma once
#include "common.h"
#include "lds_dma.h"
#include "conv_tile.h"
#include "../../include/fresco_vae.h"

namespace fresco {

constexpr int VC_WW = CT_TW + 2, VC_NPOS = (CT_TH + 2) * VC_WW;

struct VaeConv {
    const void* x;    // T
    const void* w;    // T
    const float* bias;
    const void* res;  // T
    void* out;        // T or float
    int64_t x_img_stride, w_img_stride, ldo;
    int n, H, W, Hs, Ws, rows;  // rows = H W, the output pixels per image
    int cin, cout, up2, out_kind, bias_rows;
    int tiles_x, tiles_per_img;
};

template <int TAPS>
__device__ __forceinline__ int vc_swizzle(int P) {
    return TAPS == 9 ? ((P / VC_WW + 2 * (P >> 2)) & 3) : ((P >> 2) & 3);
}

template <int TAPS, typename T>
__global__ __launch_bounds__(256) void vae_conv_kernel(const VaeConv a) {
    typedef typename Elem<T>::x4 T4;
    typedef typename Elem<T>::x8 T8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int APW = TAPS == 9 ? 3 : 2;  // window pieces per wave
    const T* ax = static_cast<const T*>(a.x);
    const T* ares = static_cast<const T*>(a.res);
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
        a_src[p] = ok ? reinterpret_cast<const char*>(ax + (int64_t)img * a.x_img_stride + off + pc * 8) : nullptr;
    }
    const char* b_src[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int R, pc;
        ct_gemm_slot(wave, p, lane, R, pc);
        b_src[p] = ct_weight_src(static_cast<const T*>(a.w) + (int64_t)img * a.w_img_stride, co0, R, pc, a.cout, TAPS * a.cin);
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
            T8 px[2], wt[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) px[i] = *reinterpret_cast<const T8*>(pa + aoff[i] + ((piece ^ asw[i]) * 16));
#pragma unroll
            for (int j = 0; j < 2; ++j) wt[j] = *reinterpret_cast<const T8*>(pb + j * 32 * 64 + ((piece ^ wsw) * 16));
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j < nbv) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[j][i] = Elem<T>::mfma32x32x16(wt[j], px[i], acc[j][i]);
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
        T* out = static_cast<T*>(a.out);
        T4 rs[2][2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = ct_channel(co0, wn, j, hi, 4 * g);
                    T4 z4 = {(T)0.f, (T)0.f, (T)0.f, (T)0.f};
                    rs[j][i][g] = (ares && opix[i] >= 0 && co < a.cout) ? *reinterpret_cast<const T4*>(ares + opix[i] * a.ldo + co)
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
                    T4 o4;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        o4[e] = Elem<T>::from_float(acc[j][i][4 * g + e] + (bv[e] + br) + (float)rs[j][i][g][e]);
                    *reinterpret_cast<T4*>(out + opix[i] * a.ldo + co) = o4;
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
                        static_cast<T*>(a.out)[((int64_t)img * a.cout + co) * a.rows + orow[i]] = Elem<T>::from_float(v);
                    } else {
                        if (ares) v += (float)ares[opix[i] * a.ldo + co];
                        static_cast<T*>(a.out)[opix[i] * a.ldo + co] = Elem<T>::from_float(v);
                    }
                }
            }
    }
}

// net_bf16.hip: vae_conv's launch for bf16 operands.  `a` is filled and checked by vae_conv (vae.hip), grid = ct_grid(..).
int vae_conv_launch_bf16(const VaeConv& a, int ksize, unsigned grid, hipStream_t st);

}  // namespace fresco
