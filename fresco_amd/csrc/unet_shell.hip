// What is left of a fp16 UNet and ControlNet around their resnets, transformers and attention: the down samplers, the two
// ends, the time-embedding MLP and the ControlNet's condition embedding.  include/fresco_unet_shell.h, DESIGN.md section 23.
//
//   unet_conv3_kernel<STRIDE, ACT>  3 x 3, zero padding 1 on all four sides, stride 1 or 2, [SiLU]
//   unet_input_kernel               (n, c, H, W) fp16 NCHW -> fp16 NHWC rows padded to the convolution's K chunk
//   unet_time_linear_kernel<TILES>  out = round16(bias + W f(src)): f the sinusoid of fp32 timesteps, or SiLU of fp16 rows
//
// unet_conv3_kernel is vaeenc_conv_down_kernel (vae_enc.hip) with the plane's pad on every side: conv_tile.h's fp16
// implicit-GEMM tile (operands, wave layout, weight ring, XCD deal, epilogue map) on 8 x 16 output pixels, the nine taps
// inner, and NO window: every (chunk, tap) step gathers its own 128 pixel rows by LDS-DMA, source pixel
// (STRIDE yo + ky - 1, STRIDE xo + kx - 1).  LDS (dynamic, 32 KiB):
//   * two slots of 8 KiB for the pixels of one step: 128 rows of 64 bytes in tile order (row r = pixel (r >> 4, r & 15)),
//     swizzled as GEMM rows;
//   * conv_tile.h's two weight slots of 8 KiB.
// Step s: every wave waits for its own copies (vmcnt(0)), barrier -- step s is in LDS and step s - 1 has been read -- then
// the pixels and weights of step s + 1 are issued into the other slots and fly under the MFMAs of step s.
// THE PAD.  A lane keeps the address of tap (0, 0) of its output pixel, i.e. source pixel (STRIDE yo - 1, STRIDE xo - 1):
// for the first row or column of a plane that lies BEFORE the plane, for pixel (0, 0) of image 0 before the buffer.  It is
// an address to add tap offsets to and is never dereferenced by itself: a 9-bit mask per lane (bit ky 3 + kx set where
// source row 0 <= STRIDE yo + ky - 1 < H and column 0 <= STRIDE xo + kx - 1 < W; all clear for tile pixels past the
// plane) selects between that address + the tap's offset and the zero page, a select on the source address with no branch
// in the loop.  Any tap can be outside: at H = W = 1 every tap but the centre is.
// Bias and SiLU are applied to the fp32 accumulator; the result is rounded to fp16 once.  No split-K, no atomics.
//
// unet_time_linear_kernel is unet_temb_kernel's scheme (unet.hip): 256 threads = four waves = four output channels, K in
// chunks of 512, a lane holds 8 weights of its channel, f(src) of 16 images x 512 k stands in LDS as fp32 (32 KiB, static);
// a lane adds its 8 products in k order into one fp32 accumulator per image, chunks in order, then a butterfly over the
// 64 lanes.
#include "common.h"
#include "lds_dma.h"
#include "conv_tile.h"
#include "../../include/fresco_unet_shell.h"

namespace fresco {

constexpr int UC_A_BYTES = 8 * 1024;  // 128 pixel rows of 64 bytes
constexpr int UC_LDS = 2 * UC_A_BYTES + 2 * CT_B_BYTES;  // 32 KiB
constexpr int UL_KC = 512, UL_IT = 16, UL_NMAX = 64;

struct UnetConv3 {
    const half_t* x;
    const half_t* w;
    const float* bias;
    half_t* out;
    int n, H, W, Ho, Wo, cin, cout;
    int tiles_x, tiles_per_img;
};

template <int STRIDE, int ACT>
__global__ __launch_bounds__(256) void unet_conv3_kernel(const UnetConv3 a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const CtTile t = ct_deal(a.n, a.tiles_per_img);
    const int img = t.img, co0 = t.col_tile * CT_BN;
    const int ty0 = (t.t_in / a.tiles_x) * CT_TH, tx0 = (t.t_in % a.tiles_x) * CT_TW;
    const uint32_t lds0 = lds_addr(smem);
    const char* zp = reinterpret_cast<const char*>(ct_zero_page);

    // ---- DMA sources, pixel rows laid out as the weight rows are (ct_gemm_slot).
    // a_src: tap (0, 0) of the row's output pixel, chunk 0 -- possibly before the plane or the buffer, see THE PAD: only ever
    // used behind a_ok; a_ok: bit t set where tap t of that pixel is inside the plane.
    const char* a_src[2];
    int a_ok[2];
    const char* b_src[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int R, pc;
        ct_gemm_slot(wave, p, lane, R, pc);
        const int yo = ty0 + (R >> 4), xo = tx0 + (R & 15);
        const int ys = STRIDE * yo - 1, xs = STRIDE * xo - 1;  // source pixel of tap (0, 0)
        int rows_ok = 0, cols_ok = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (ys + k >= 0 && ys + k < a.H) rows_ok |= 0x007 << (3 * k);
            if (xs + k >= 0 && xs + k < a.W) cols_ok |= 0x049 << k;
        }
        a_ok[p] = (yo < a.Ho && xo < a.Wo) ? (rows_ok & cols_ok) : 0;
        const int64_t pix = ((int64_t)img * a.H + ys) * a.W + xs;  // -W - 1 at the first pixel of the buffer
        a_src[p] = reinterpret_cast<const char*>(a.x) + (pix * a.cin + pc * 8) * 2;
        b_src[p] = ct_weight_src(a.w, co0, R, pc, a.cout, 9 * a.cin);
    }
    // step (chunk, tap): pixels at a_off bytes from the lane's tap-(0, 0) address, weights at column k0
    auto issue = [&](int s, int tap, int64_t a_off, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            lds_dma16((a_ok[p] >> tap) & 1 ? static_cast<const void*>(a_src[p] + a_off) : static_cast<const void*>(zp),
                      lds0 + (uint32_t)((s & 1) * UC_A_BYTES + (wave * 2 + p) * 1024));
        ct_issue_weights(b_src, s, k0, lds0 + 2 * UC_A_BYTES, wave);
    };

    const int nbv = ct_live_blocks(a.cout, co0, wn);
    floatx16 acc[2][2] = {};  // [channel block j][pixel block i]

    const int chunks = a.cin / CT_BK, steps = chunks * 9;
    const int sw = (l31 >> 2) & 3;  // rows wm 64 + i 32 + l31 and wn 64 + j 32 + l31 share it
    issue(0, 0, 0, 0);
    int chunk = 0, tap = 0;
    for (int s = 0; s < steps; ++s) {
        dma_wait_barrier<0>();
        if (s + 1 < steps) {
            const int t1 = tap + 1 == 9 ? 0 : tap + 1, c1 = tap + 1 == 9 ? chunk + 1 : chunk;
            const int ky = t1 / 3, kx = t1 - ky * 3;
            issue(s + 1, t1, (((int64_t)ky * a.W + kx) * a.cin + c1 * CT_BK) * 2, t1 * a.cin + c1 * CT_BK);
        }
        const char* pa = smem + (s & 1) * UC_A_BYTES + (wm * 64 + l31) * 64;
        const char* pb = smem + 2 * UC_A_BYTES + (s & 1) * CT_B_BYTES + (wn * 64 + l31) * 64;
#pragma unroll
        for (int ks = 0; ks < CT_BK / 16; ++ks) {
            const int piece = ((ks * 2 + hi) ^ sw) * 16;
            half8_t px[2], wt[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) px[i] = *reinterpret_cast<const half8_t*>(pa + i * 32 * 64 + piece);
#pragma unroll
            for (int j = 0; j < 2; ++j) wt[j] = *reinterpret_cast<const half8_t*>(pb + j * 32 * 64 + piece);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j < nbv) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[j], px[i], acc[j][i], 0, 0, 0);
                }
        }
        if (++tap == 9) {
            tap = 0;
            ++chunk;
        }
    }

    // ---- epilogue (conv_tile.h's map).  Every address is computed before the first store.
    auto finish = [&](float v) __attribute__((always_inline)) { return ACT ? v / (1.f + expf(-v)) : v; };
    int64_t opix[2];  // pixel index over all images, -1: outside the plane
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = ct_row(wm, i, l31);
        const int yo = ty0 + (r >> 4), xo = tx0 + (r & 15);
        opix[i] = (yo < a.Ho && xo < a.Wo) ? ((int64_t)img * a.Ho + yo) * a.Wo + xo : -1;
    }
    if (!(a.cout & 3)) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = ct_channel(co0, wn, j, hi, 4 * g);
                if (co >= a.cout) continue;
                const floatx4 bv = *reinterpret_cast<const floatx4*>(a.bias + co);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (opix[i] < 0) continue;
                    half4_t o4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o4[e] = (half_t)finish(acc[j][i][4 * g + e] + bv[e]);
                    *reinterpret_cast<half4_t*>(a.out + opix[i] * a.cout + co) = o4;
                }
            }
    } else {
        // a channel count that is no multiple of four: one element per store
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (opix[i] < 0) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct_channel(co0, wn, j, hi, r);
                    if (co < a.cout) a.out[opix[i] * a.cout + co] = (half_t)finish(acc[j][i][r] + a.bias[co]);
                }
            }
    }
}

// One thread per pixel: its cpad / 8 pieces, channels >= c zero.
__global__ __launch_bounds__(256) void unet_input_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int n, int c,
                                                         int hw, int cpad) {
    const int64_t total = (int64_t)n * hw;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx / hw, p = idx - i * hw;
        for (int c0 = 0; c0 < cpad; c0 += 8) {
            half8_t o8;
#pragma unroll
            for (int e = 0; e < 8; ++e) o8[e] = c0 + e < c ? x[(i * c + c0 + e) * hw + p] : (half_t)0.f;
            *reinterpret_cast<half8_t*>(out + idx * cpad + c0) = o8;
        }
    }
}

// cos(x), or sin(x) with want_sin, of an fp32 argument.  The library's cosf / sinf keep a table in scratch memory for large
// arguments; here x is reduced by multiples of pi / 2 in fp64 (exact to well below an fp32 ulp for |x| < 2^30: the timesteps'
// arguments stay below a few thousand) and the remainder in [-pi / 4, pi / 4] goes through the two minimax polynomials of
// the Cephes single-precision library (sinf.c, cosf.c: errors below one fp32 ulp on that interval).
__device__ __forceinline__ float ul_cos_sin(float x, bool want_sin) {
    const double xd = (double)x;
    const double nd = rint(xd * 0.63661977236758134308);
    const float r = (float)fma(-nd, 1.57079632679489661923, xd);
    const int q = ((int)(long long)nd + (want_sin ? 0 : 1)) & 3;   // cos(x) = sin(x + pi / 2)
    const float z = r * r;
    const float s = r + r * z * (-1.6666654611e-1f + z * (8.3321608736e-3f + z * -1.9515295891e-4f));
    const float c = 1.f - 0.5f * z + z * z * (4.166664568298827e-2f + z * (-1.388731625493765e-3f + z * 2.443315711809948e-5f));
    const float v = (q & 1) ? c : s;
    return (q & 2) ? -v : v;
}

// grid (ceil(cout / 4)); wave w: output channel 4 blockIdx.x + w.  TILES = ceil(n / 16): images >= n are zero rows in LDS.
// KIND 0 (UNET_SRC_TIMESTEPS): src fp32 (n); column k < K / 2 is cos(t w_k), column K / 2 + i is sin(t w_i),
// w_i = exp(-ln(10000) i / (K / 2)), in fp32, rounded to fp16; workgroup 0 also writes them to sin_out where that is given.
// KIND 1 (UNET_SRC_SILU_ROWS): src fp16 (n, K); SiLU in fp32.
template <int TILES, int KIND>
__global__ __launch_bounds__(256) void unet_time_linear_kernel(const void* __restrict__ src, const half_t* __restrict__ w,
                                                               const float* __restrict__ bias, half_t* __restrict__ out,
                                                               half_t* __restrict__ sin_out, int n, int K, int cout) {
    __shared__ __attribute__((aligned(16))) float s[UL_IT][UL_KC];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int co = blockIdx.x * 4 + wave;
    const bool has = co < cout;
    const int half_k = K >> 1;
    float acc[TILES * UL_IT];
#pragma unroll
    for (int i = 0; i < TILES * UL_IT; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < K; k0 += UL_KC) {
        float wf[8];
        {
            const int k = k0 + lane * 8;  // (K % 8 == 0: a piece is inside the row or outside it)
            half8_t w8;
#pragma unroll
            for (int e = 0; e < 8; ++e) w8[e] = (half_t)0.f;
            if (has && k < K) w8 = *reinterpret_cast<const half8_t*>(w + (int64_t)co * K + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[e] = (float)w8[e];
        }
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            __syncthreads();
            if (KIND == UNET_SRC_TIMESTEPS) {
                // one element per thread and pass: the fp64 reduction of ul_cos_sin is kept out of an unrolled loop
#pragma unroll 1
                for (int idx = tid; idx < UL_IT * UL_KC; idx += 256) {
                    const int i = idx >> 9, kk = idx & (UL_KC - 1), gi = t * UL_IT + i, k = k0 + kk;
                    float v = 0.f;
                    if (gi < n && k < K) {
                        const int fi = k < half_k ? k : k - half_k;
                        const float arg = static_cast<const float*>(src)[gi] * expf((-9.210340371976184f * (float)fi) / (float)half_k);
                        const half_t h = (half_t)ul_cos_sin(arg, k >= half_k);
                        if (sin_out && blockIdx.x == 0) sin_out[(int64_t)gi * K + k] = h;
                        v = (float)h;
                    }
                    s[i][kk] = v;
                }
            } else {
                for (int idx = tid; idx < UL_IT * (UL_KC / 8); idx += 256) {
                    const int i = idx >> 6, kk = (idx & 63) * 8, gi = t * UL_IT + i;
                    half8_t t8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) t8[e] = (half_t)0.f;
                    if (gi < n && k0 + kk < K)
                        t8 = *reinterpret_cast<const half8_t*>(static_cast<const half_t*>(src) + (int64_t)gi * K + k0 + kk);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = (float)t8[e];
                        s[i][kk + e] = v / (1.f + expf(-v));
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < UL_IT; ++i) {
                const floatx4 p0 = *reinterpret_cast<const floatx4*>(&s[i][lane * 8]);
                const floatx4 p1 = *reinterpret_cast<const floatx4*>(&s[i][lane * 8 + 4]);
                float v = acc[t * UL_IT + i];
#pragma unroll
                for (int e = 0; e < 4; ++e) v += p0[e] * wf[e];
#pragma unroll
                for (int e = 0; e < 4; ++e) v += p1[e] * wf[4 + e];
                acc[t * UL_IT + i] = v;
            }
        }
    }
    const float b = has ? bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < TILES * UL_IT; ++i) {
        const float v = wave_sum(acc[i]);
        if (lane == 0 && has && i < n) out[(int64_t)i * cout + co] = (half_t)(v + b);
    }
}

template <int STRIDE, int ACT>
static int uc_launch(const UnetConv3& a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((unet_conv3_kernel<STRIDE, ACT>), dim3(grid), dim3(256), UC_LDS, st, a);  // 32 KiB of dynamic LDS
    return check_launch();
}

template <int KIND>
static int ul_launch(const void* src, const half_t* w, const float* bias, half_t* out, half_t* sin_out, int n, int K, int cout,
                     hipStream_t st) {
    auto kern = n <= UL_IT ? unet_time_linear_kernel<1, KIND>
                           : (n <= 2 * UL_IT ? unet_time_linear_kernel<2, KIND>
                                             : (n <= 3 * UL_IT ? unet_time_linear_kernel<3, KIND> : unet_time_linear_kernel<4, KIND>));
    hipLaunchKernelGGL(kern, dim3((cout + 3) / 4), dim3(256), 0, st, src, w, bias, out, sin_out, n, K, cout);
    return check_launch();
}

}  // namespace fresco

using namespace fresco;

extern "C" int unet_conv3(const void* x, const void* w, const float* bias, void* out, int n, int H, int W, int cin, int cout,
                          int stride, int act, void* stream) {
    if (!x || !w || !bias || !out || n <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0) return FRESCO_EINVAL;
    if (!aligned_to(x, 16) || !aligned_to(w, 16) || !aligned_to(bias, 16) || !aligned_to(out, 8)) return FRESCO_EINVAL;
    if ((stride != 1 && stride != 2) || (act != UNET_ACT_NONE && act != UNET_ACT_SILU)) return FRESCO_EUNSUPPORTED;
    if (!ct_supported(n, H, W, cin)) return FRESCO_EUNSUPPORTED;
    UnetConv3 a;
    a.x = static_cast<const half_t*>(x);
    a.w = static_cast<const half_t*>(w);
    a.bias = bias;
    a.out = static_cast<half_t*>(out);
    a.n = n;
    a.H = H;
    a.W = W;
    a.Ho = (H - 1) / stride + 1;
    a.Wo = (W - 1) / stride + 1;
    a.cin = cin;
    a.cout = cout;
    a.tiles_x = ct_tiles_x(a.Wo);
    a.tiles_per_img = ct_plane_tiles(a.Ho, a.Wo);
    const unsigned grid = ct_grid(n, a.tiles_per_img, cout);
    if (!grid) return FRESCO_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    if (stride == 1) return act ? uc_launch<1, 1>(a, grid, st) : uc_launch<1, 0>(a, grid, st);
    return act ? uc_launch<2, 1>(a, grid, st) : uc_launch<2, 0>(a, grid, st);
}

extern "C" int unet_input(const void* x, void* out, int n, int c, int H, int W, int cpad, void* stream) {
    if (!x || !out || n <= 0 || c <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (cpad < 8 || cpad > 64 || cpad % 8 || c > cpad) return FRESCO_EINVAL;
    if (!aligned_to(x, 2) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    if ((int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(unet_input_kernel, dim3(stream_blocks((int64_t)n * H * W)), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t*>(x), static_cast<half_t*>(out), n, c, H * W, cpad);
    return check_launch();
}

extern "C" int unet_time_linear(const void* src, int src_kind, const void* w, const float* bias, void* out, void* sin_out, int n,
                                int K, int cout, void* stream) {
    if (!src || !w || !bias || !out || n <= 0 || K <= 0 || cout <= 0) return FRESCO_EINVAL;
    if (src_kind != UNET_SRC_TIMESTEPS && src_kind != UNET_SRC_SILU_ROWS) return FRESCO_EUNSUPPORTED;
    if (n > UL_NMAX || K % 8) return FRESCO_EUNSUPPORTED;
    if (sin_out && src_kind != UNET_SRC_TIMESTEPS) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(src, src_kind == UNET_SRC_TIMESTEPS ? 4 : 16) || !aligned_to(w, 16) || !aligned_to(bias, 4) ||
        !aligned_to(out, 2) || !aligned_to(sin_out, 16))
        return FRESCO_EINVAL;
    hipStream_t st = as_stream(stream);
    const half_t* wh = static_cast<const half_t*>(w);
    half_t* oh = static_cast<half_t*>(out);
    half_t* sh = static_cast<half_t*>(sin_out);
    if (src_kind == UNET_SRC_TIMESTEPS) return ul_launch<UNET_SRC_TIMESTEPS>(src, wh, bias, oh, sh, n, K, cout, st);
    return ul_launch<UNET_SRC_SILU_ROWS>(src, wh, bias, oh, sh, n, K, cout, st);
}
