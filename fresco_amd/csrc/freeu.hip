// FreeU (src/free_lunch_utils.py) for the decoder's up blocks: the skip-connection filter in closed form and the backbone
// scaling fused with the channel concat.  DESIGN.md section 11.
//
// Fourier_filter(x, threshold = 1, scale = s) (free_lunch_utils.py:25-52) multiplies the four shifted FFT bins
// [H/2-1, H/2] x [W/2-1, W/2] by s: these are the frequencies (u, v) in {-1, 0}^2 for even and odd sizes alike.  The real
// part of the inverse transform is then a rank-7 correction of the input, with theta_h = 2 pi h / H, phi_w = 2 pi w / W
// and sums over the plane:
//   y[h,w] = x[h,w] + (s-1)/(H W) ( S0 + S1 cos theta_h + S2 sin theta_h + S3 cos phi_w + S4 sin phi_w
//                                  + S5 cos(theta_h + phi_w) + S6 sin(theta_h + phi_w) )
//   S0 = sum x, S1 = sum x cos theta, S2 = sum x sin theta, S3 = sum x cos phi, S4 = sum x sin phi,
//   S5 = sum x cos(theta + phi), S6 = sum x sin(theta + phi)
// No FFT: seven sums and one correction per element.  fp32 arithmetic for fp16 / bf16 / fp32 storage, one rounding at the
// store; every sum is reduced in a fixed tree (lane partials, xor butterfly within the wave, waves through LDS in a fixed
// order), no float atomics: the same input gives the same bits on every run.
//
// The backbone half (free_lunch_utils.py:127-147): m = mean over channels, per sample min / max of m,
// hidden[:, :n_scaled] *= (b - 1) (m - min) / (max - min) + 1, in place, and optionally hidden -> cat[:, :C] in the same
// pass.  A constant mean map gives max == min and 0 / 0, as in the reference: the scaled channels become non-finite.
// That quirk is reproduced, not repaired (a sample whose channel mean is the same at every pixel does not occur in a
// denoising run).
#include "common.h"

namespace fresco {

// V consecutive elements moved as one access (16 bytes for V * sizeof(T) == 16)
template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

template <typename T, int V>
__device__ __forceinline__ void load_pack(const T* p, float* f) {
    const Pack<T, V> k = *reinterpret_cast<const Pack<T, V>*>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] = (float)k.v[j];
}

template <typename T, int V>
__device__ __forceinline__ void store_pack(T* p, const float* f) {
    Pack<T, V> k;
#pragma unroll
    for (int j = 0; j < V; ++j) k.v[j] = (T)f[j];
    *reinterpret_cast<Pack<T, V>*>(p) = k;
}

// ---------------------------------------------------------------------------------------------------------------
// Fourier filter
// ---------------------------------------------------------------------------------------------------------------
// cos / sin of the row and column angles, once per workgroup: tab = cos theta[H] | sin theta[H] | cos phi[W] | sin phi[W]
__device__ __forceinline__ void freeu_build_tables(float* tab, int H, int W) {
    for (int j = threadIdx.x; j < H + W; j += blockDim.x) {
        const bool row = j < H;
        const int k = row ? j : j - H, n = row ? H : W;
        float s, c;
        sincospif((float)(2 * k) / (float)n, &s, &c);
        float* t = row ? tab : tab + 2 * H;
        t[k] = c;
        t[n + k] = s;
    }
}

struct FreeuSums {
    float s[7];
};

// V consecutive elements of a plane, the first at linear index i0: their share of the seven sums.  The (theta + phi)
// products come from angle addition.
template <int V>
__device__ __forceinline__ void freeu_accumulate(FreeuSums& a, const float* x, int i0, int H, int W, const float* tab) {
    int h = i0 / W, w = i0 - h * W;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float ch = tab[h], sh = tab[H + h], cw = tab[2 * H + w], sw = tab[2 * H + W + w];
        const float v = x[j];
        a.s[0] += v;
        a.s[1] = fmaf(v, ch, a.s[1]);
        a.s[2] = fmaf(v, sh, a.s[2]);
        a.s[3] = fmaf(v, cw, a.s[3]);
        a.s[4] = fmaf(v, sw, a.s[4]);
        a.s[5] = fmaf(v, ch * cw - sh * sw, a.s[5]);
        a.s[6] = fmaf(v, sh * cw + ch * sw, a.s[6]);
        if (++w == W) {
            w = 0;
            ++h;
        }
    }
}

// y = x + coef (S0 + S1 ch + S2 sh + cw (S3 + S5 ch + S6 sh) + sw (S4 - S5 sh + S6 ch)), the closed form regrouped by column
template <int V>
__device__ __forceinline__ void freeu_correct(const FreeuSums& a, float coef, float* x, int i0, int H, int W,
                                              const float* tab) {
    int h = i0 / W, w = i0 - h * W;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float ch = tab[h], sh = tab[H + h], cw = tab[2 * H + w], sw = tab[2 * H + W + w];
        const float r0 = fmaf(a.s[2], sh, fmaf(a.s[1], ch, a.s[0]));
        const float rc = fmaf(a.s[6], sh, fmaf(a.s[5], ch, a.s[3]));
        const float rs = fmaf(a.s[6], ch, fmaf(-a.s[5], sh, a.s[4]));
        x[j] = fmaf(coef, fmaf(sw, rs, fmaf(cw, rc, r0)), x[j]);
        if (++w == W) {
            w = 0;
            ++h;
        }
    }
}

// Planes of at most 16 * TPP elements, held in 16 registers per thread between the sum pass and the apply pass: one
// global read, one write.  TPP = 64: one wave per plane, four planes per workgroup (H W <= 1024); TPP = 256: one
// workgroup per plane (H W <= 4096).  V = 16 bytes of elements when H W % V == 0 and the pointers allow, else 1.
// Dynamic LDS: the tables, then 28 floats for the cross-wave step.
template <typename T, int V, int TPP>
__global__ __launch_bounds__(256) void freeu_fourier_reg_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                                 int64_t out_bs, int nplanes, int C, int H, int W,
                                                                 float coef) {
    extern __shared__ __attribute__((aligned(16))) float freeu_lds[];
    float* tab = freeu_lds;
    float* red = freeu_lds + 2 * (H + W);
    freeu_build_tables(tab, H, W);
    __syncthreads();
    constexpr int NK = 16 / V;
    const int HW = H * W;
    const int plane = blockIdx.x * (256 / TPP) + threadIdx.x / TPP;
    const int tl = threadIdx.x % TPP;
    const bool live = plane < nplanes;  // wave-uniform
    if (TPP == 64 && !live) return;
    const T* xp = x + (int64_t)plane * HW;
    T* op = out + (int64_t)(plane / C) * out_bs + (int64_t)(plane % C) * HW;
    float v[16];
    FreeuSums a;
#pragma unroll
    for (int j = 0; j < 7; ++j) a.s[j] = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int i0 = (k * TPP + tl) * V;
        if (i0 < HW) {
            load_pack<T, V>(xp + i0, v + k * V);
            freeu_accumulate<V>(a, v + k * V, i0, H, W, tab);
        }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) a.s[j] = wave_sum(a.s[j]);
    if (TPP == 256) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int j = 0; j < 7; ++j) red[j * 4 + wave] = a.s[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 7; ++j) a.s[j] = (red[j * 4] + red[j * 4 + 1]) + (red[j * 4 + 2] + red[j * 4 + 3]);
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int i0 = (k * TPP + tl) * V;
        if (i0 < HW) {
            freeu_correct<V>(a, coef, v + k * V, i0, H, W, tab);
            store_pack<T, V>(op + i0, v + k * V);
        }
    }
}

// Larger planes: one workgroup per plane, the plane read twice (the second read comes from L2).
template <typename T, int V>
__global__ __launch_bounds__(256) void freeu_fourier_two_pass_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                                      int64_t out_bs, int C, int H, int W, float coef) {
    extern __shared__ __attribute__((aligned(16))) float freeu_lds[];
    float* tab = freeu_lds;
    float* red = freeu_lds + 2 * (H + W);
    freeu_build_tables(tab, H, W);
    __syncthreads();
    const int HW = H * W;
    const int plane = blockIdx.x;
    const T* xp = x + (int64_t)plane * HW;
    T* op = out + (int64_t)(plane / C) * out_bs + (int64_t)(plane % C) * HW;
    FreeuSums a;
#pragma unroll
    for (int j = 0; j < 7; ++j) a.s[j] = 0.f;
    for (int i0 = threadIdx.x * V; i0 < HW; i0 += 256 * V) {
        float v[V];
        load_pack<T, V>(xp + i0, v);
        freeu_accumulate<V>(a, v, i0, H, W, tab);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) a.s[j] = wave_sum(a.s[j]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 7; ++j) red[j * 4 + wave] = a.s[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 7; ++j) a.s[j] = (red[j * 4] + red[j * 4 + 1]) + (red[j * 4 + 2] + red[j * 4 + 3]);
    for (int i0 = threadIdx.x * V; i0 < HW; i0 += 256 * V) {
        float v[V];
        load_pack<T, V>(xp + i0, v);
        freeu_correct<V>(a, coef, v, i0, H, W, tab);
        store_pack<T, V>(op + i0, v);
    }
}

// scale == 1: the filter is the identity (the reference returns x up to its FFT noise): a strided copy, no sums.
// grid (blocks over one sample's C H W elements, B)
template <typename T, int V>
__global__ __launch_bounds__(256) void freeu_copy_kernel(const T* __restrict__ x, T* __restrict__ out, int64_t out_bs,
                                                          int64_t chw) {
    const T* xp = x + (int64_t)blockIdx.y * chw;
    T* op = out + (int64_t)blockIdx.y * out_bs;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < chw; i += (int64_t)gridDim.x * 256 * V)
        *reinterpret_cast<Pack<T, V>*>(op + i) = *reinterpret_cast<const Pack<T, V>*>(xp + i);
}

// ---------------------------------------------------------------------------------------------------------------
// Backbone
// ---------------------------------------------------------------------------------------------------------------
// A workgroup of 256 threads is laid out as (channel lane cy, pixel lane px): px = t % LPX runs along packs of V pixels,
// cy = t / LPX along channels, LPX = 1 << lpx_log2 the smallest power of two that covers the plane (at most 256).

// Channel sums, split over channel ranges so that the smallest site still fills the chip.  grid (pixel tiles, splits, B);
// partial (B, splits, HW) fp32.  Each thread sums its channels in order, the channel lanes are then added in order
// through LDS.
template <typename T, int V>
__global__ __launch_bounds__(256) void freeu_chan_partial_kernel(const T* __restrict__ hidden,
                                                                  float* __restrict__ partial, int C, int HW,
                                                                  int lpx_log2, int cps) {
    __shared__ __attribute__((aligned(16))) float sh[256 * V];
    const int LPX = 1 << lpx_log2, CY = 256 >> lpx_log2;
    const int px = threadIdx.x & (LPX - 1), cy = threadIdx.x >> lpx_log2;
    const int p0 = (blockIdx.x * LPX + px) * V;
    const int c0 = blockIdx.y * cps, c1 = min(C, c0 + cps);
    const T* hp = hidden + (int64_t)blockIdx.z * C * HW + p0;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (p0 < HW) {
#pragma unroll 4
        for (int c = c0 + cy; c < c1; c += CY) {
            float v[V];
            load_pack<T, V>(hp + (int64_t)c * HW, v);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) sh[threadIdx.x * V + j] = acc[j];
    __syncthreads();
    float* pp = partial + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * HW;
    for (int q = threadIdx.x; q < LPX * V; q += 256) {
        float s = sh[q];
        for (int k = 1; k < CY; ++k) s += sh[k * LPX * V + q];
        const int p = blockIdx.x * LPX * V + q;
        if (p < HW) pp[p] = s;
    }
}

// One workgroup of 1024 threads per sample: adds the partials in split order, divides by C, writes the mean map (B, HW)
// and the sample's min and max (B, 2).
__global__ __launch_bounds__(1024) void freeu_minmax_kernel(const float* __restrict__ partial, float* __restrict__ mean,
                                                             float* __restrict__ minmax, int splits, int C, int HW) {
    __shared__ float red[32];
    const float* pp = partial + (int64_t)blockIdx.x * splits * HW;
    float* mp = mean + (int64_t)blockIdx.x * HW;
    float lo = INFINITY, hi = -INFINITY;
    for (int p = threadIdx.x; p < HW; p += 1024) {
        float s = pp[p];
#pragma unroll 4
        for (int k = 1; k < splits; ++k) s += pp[(int64_t)k * HW + p];
        const float m = s / (float)C;
        mp[p] = m;
        lo = fminf(lo, m);
        hi = fmaxf(hi, m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave] = lo;
        red[16 + wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) {
            lo = fminf(lo, red[k]);
            hi = fmaxf(hi, red[16 + k]);
        }
        minmax[2 * blockIdx.x] = lo;
        minmax[2 * blockIdx.x + 1] = hi;
    }
}

// hidden[:, :n_scaled] *= f in place (and into cat[:, :n_scaled]); hidden[:, n_scaled:] -> cat only.  The factor follows
// the reference's operation order, f = (b - 1) * ((m - min) / (max - min)) + 1, no contraction; it is formed once per
// thread and reused over CPT channels.  grid (pixel tiles, channel groups of CY * CPT, B); with cat == NULL the grid
// covers the scaled channels only.
constexpr int FREEU_CPT = 4;
template <typename T, int V>
__global__ __launch_bounds__(256) void freeu_scale_cat_kernel(T* __restrict__ hidden, T* __restrict__ cat,
                                                               int64_t cat_bs, const float* __restrict__ mean,
                                                               const float* __restrict__ minmax, int C, int n_scaled,
                                                               int c_end, int HW, int lpx_log2, float bm1) {
    const int LPX = 1 << lpx_log2, CY = 256 >> lpx_log2;
    const int px = threadIdx.x & (LPX - 1), cy = threadIdx.x >> lpx_log2;
    const int p0 = (blockIdx.x * LPX + px) * V;
    if (p0 >= HW) return;
    const int b = blockIdx.z;
    const int cbase = blockIdx.y * CY * FREEU_CPT + cy;
    float f[V];
    if (cbase < n_scaled) {
        const float lo = minmax[2 * b], hi = minmax[2 * b + 1];
        const float range = hi - lo;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float hm = __fdiv_rn(__fsub_rn(mean[(int64_t)b * HW + p0 + j], lo), range);
            f[j] = __fadd_rn(__fmul_rn(bm1, hm), 1.f);
        }
    }
    T* hp = hidden + (int64_t)b * C * HW + p0;
    T* cp = cat ? cat + (int64_t)b * cat_bs + p0 : nullptr;
#pragma unroll
    for (int k = 0; k < FREEU_CPT; ++k) {
        const int c = cbase + k * CY;
        if (c >= c_end) break;
        float v[V];
        load_pack<T, V>(hp + (int64_t)c * HW, v);
        if (c < n_scaled) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = __fmul_rn(v[j], f[j]);
            store_pack<T, V>(hp + (int64_t)c * HW, v);
        }
        if (cp) store_pack<T, V>(cp + (int64_t)c * HW, v);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

// smallest l <= 8 with (V << l) >= HW
static inline int freeu_lpx_log2(int HW, int V) {
    int l = 0;
    while (l < 8 && ((int64_t)V << l) < HW) ++l;
    return l;
}

struct FreeuPlan {
    int lpx_log2, tiles, splits, cps;
};

// Channel splits of freeu_chan_partial: enough workgroups for two per CU at the smallest site, no split shorter than one
// pass of the channel lanes, at most 40 (freeu_minmax reads every split from one workgroup per sample).
static FreeuPlan freeu_plan(int B, int C, int HW, int V) {
    FreeuPlan p;
    p.lpx_log2 = freeu_lpx_log2(HW, V);
    const int64_t per_tile = (int64_t)V << p.lpx_log2;
    p.tiles = (int)((HW + per_tile - 1) / per_tile);
    const int CY = 256 >> p.lpx_log2;
    const int64_t bt = (int64_t)B * p.tiles;
    int64_t want = (512 + bt - 1) / bt;
    const int64_t most = (C + CY - 1) / CY;
    if (want > most) want = most;
    if (want > 40) want = 40;
    if (want < 1) want = 1;
    p.cps = (int)((C + want - 1) / want);
    p.splits = (C + p.cps - 1) / p.cps;
    return p;
}

struct FreeuWorkspace {
    size_t partial, mean, minmax, total;  // byte offsets and the size
};

static FreeuWorkspace freeu_workspace(int B, int C, int HW) {
    int splits = 1;
    for (int V : {1, 4, 8}) {
        const int n = freeu_plan(B, C, HW, V).splits;
        if (n > splits) splits = n;
    }
    FreeuWorkspace w;
    w.partial = 0;
    w.mean = align_up((size_t)B * splits * HW * sizeof(float), 256);
    w.minmax = w.mean + align_up((size_t)B * HW * sizeof(float), 256);
    w.total = w.minmax + align_up((size_t)B * 2 * sizeof(float), 256);
    return w;
}

constexpr int FREEU_MAX_SIDES = 8192;  // H + W: the tables take 8 (H + W) bytes of the 64 KiB of LDS a launch gets unasked

template <typename T>
static int freeu_fourier_launch(const T* x, T* out, int64_t out_bs, int B, int C, int H, int W, float scale,
                                hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int HW = H * W;
    const int64_t chw = (int64_t)C * HW;
    const bool wide = aligned_to(x, 16) && aligned_to(out, 16) && HW % VEC == 0 && out_bs % VEC == 0;
    if (scale == 1.0f) {
        const bool wide_copy = aligned_to(x, 16) && aligned_to(out, 16) && chw % VEC == 0 && out_bs % VEC == 0;
        const int64_t per_block = 256 * (wide_copy ? VEC : 1);
        const int64_t need = (chw + per_block - 1) / per_block;
        const int blocks = need < 2048 ? (int)need : 2048;
        if (wide_copy)
            hipLaunchKernelGGL((freeu_copy_kernel<T, VEC>), dim3(blocks, B), dim3(256), 0, st, x, out, out_bs, chw);
        else
            hipLaunchKernelGGL((freeu_copy_kernel<T, 1>), dim3(blocks, B), dim3(256), 0, st, x, out, out_bs, chw);
        return check_launch();
    }
    const int nplanes = B * C;
    const float coef = (scale - 1.0f) / (float)HW;
    const size_t lds = (size_t)(2 * (H + W) + 28) * sizeof(float);
    if (HW <= 1024) {
        const dim3 grid((nplanes + 3) / 4);
        if (wide)
            hipLaunchKernelGGL((freeu_fourier_reg_kernel<T, VEC, 64>), grid, dim3(256), lds, st, x, out, out_bs, nplanes, C,
                               H, W, coef);
        else
            hipLaunchKernelGGL((freeu_fourier_reg_kernel<T, 1, 64>), grid, dim3(256), lds, st, x, out, out_bs, nplanes, C,
                               H, W, coef);
    } else if (HW <= 4096) {
        if (wide)
            hipLaunchKernelGGL((freeu_fourier_reg_kernel<T, VEC, 256>), dim3(nplanes), dim3(256), lds, st, x, out, out_bs,
                               nplanes, C, H, W, coef);
        else
            hipLaunchKernelGGL((freeu_fourier_reg_kernel<T, 1, 256>), dim3(nplanes), dim3(256), lds, st, x, out, out_bs,
                               nplanes, C, H, W, coef);
    } else {
        if (wide)
            hipLaunchKernelGGL((freeu_fourier_two_pass_kernel<T, VEC>), dim3(nplanes), dim3(256), lds, st, x, out, out_bs,
                               C, H, W, coef);
        else
            hipLaunchKernelGGL((freeu_fourier_two_pass_kernel<T, 1>), dim3(nplanes), dim3(256), lds, st, x, out, out_bs, C,
                               H, W, coef);
    }
    return check_launch();
}

template <typename T, int V>
static void freeu_backbone_kernels(T* hidden, T* cat, int64_t cat_bs, int B, int C, int n_scaled, int HW, float b,
                                   char* ws, const FreeuWorkspace& lay, hipStream_t st) {
    const FreeuPlan p = freeu_plan(B, C, HW, V);
    float* partial = reinterpret_cast<float*>(ws + lay.partial);
    float* mean = reinterpret_cast<float*>(ws + lay.mean);
    float* minmax = reinterpret_cast<float*>(ws + lay.minmax);
    hipLaunchKernelGGL((freeu_chan_partial_kernel<T, V>), dim3(p.tiles, p.splits, B), dim3(256), 0, st, hidden, partial,
                       C, HW, p.lpx_log2, p.cps);
    hipLaunchKernelGGL(freeu_minmax_kernel, dim3(B), dim3(1024), 0, st, partial, mean, minmax, p.splits, C, HW);
    const int c_end = cat ? C : n_scaled;
    if (c_end > 0) {
        const int per_group = (256 >> p.lpx_log2) * FREEU_CPT;
        hipLaunchKernelGGL((freeu_scale_cat_kernel<T, V>), dim3(p.tiles, (c_end + per_group - 1) / per_group, B), dim3(256),
                           0, st, hidden, cat, cat_bs, mean, minmax, C, n_scaled, c_end, HW, p.lpx_log2, b - 1.0f);
    }
}

template <typename T>
static int freeu_backbone_launch(T* hidden, T* cat, int64_t cat_bs, int B, int C, int n_scaled, int HW, float b, char* ws,
                                 const FreeuWorkspace& lay, hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const bool wide = aligned_to(hidden, 16) && HW % VEC == 0 && (!cat || (aligned_to(cat, 16) && cat_bs % VEC == 0));
    if (wide)
        freeu_backbone_kernels<T, VEC>(hidden, cat, cat_bs, B, C, n_scaled, HW, b, ws, lay, st);
    else
        freeu_backbone_kernels<T, 1>(hidden, cat, cat_bs, B, C, n_scaled, HW, b, ws, lay, st);
    return check_launch();
}

static inline size_t freeu_elem_size(int dtype) {
    return dtype == FRESCO_F32 ? 4 : (dtype == FRESCO_F16 || dtype == FRESCO_BF16) ? 2 : 0;
}

}  // namespace fresco

using namespace fresco;

extern "C" size_t fresco_freeu_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H < 2 || W < 2 || (int64_t)H * W > (1 << 26) || B > 65535) return 0;
    return freeu_workspace(B, C, H * W).total;
}

extern "C" int fresco_freeu_fourier(const void* x, void* out, int64_t out_batch_stride, int B, int C, int H, int W,
                                    float scale, int dtype, void* stream) {
    const size_t es = freeu_elem_size(dtype);
    if (!x || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || es == 0) return FRESCO_EINVAL;
    if (H < 2 || W < 2 || H + W > FREEU_MAX_SIDES) return FRESCO_EUNSUPPORTED;
    if ((int64_t)B * C > INT32_MAX - 4 || B > 65535) return FRESCO_EUNSUPPORTED;
    if (out_batch_stride < (int64_t)C * H * W) return FRESCO_EINVAL;
    if (!aligned_to(x, es) || !aligned_to(out, es)) return FRESCO_EINVAL;
    hipStream_t st = as_stream(stream);
    if (dtype == FRESCO_F16)
        return freeu_fourier_launch(static_cast<const half_t*>(x), static_cast<half_t*>(out), out_batch_stride, B, C, H,
                                    W, scale, st);
    if (dtype == FRESCO_BF16)
        return freeu_fourier_launch(static_cast<const bf16_t*>(x), static_cast<bf16_t*>(out), out_batch_stride, B, C, H,
                                    W, scale, st);
    return freeu_fourier_launch(static_cast<const float*>(x), static_cast<float*>(out), out_batch_stride, B, C, H, W,
                                scale, st);
}

extern "C" int fresco_freeu_backbone(void* hidden, void* cat, int64_t cat_batch_stride, int B, int C, int n_scaled, int H,
                                     int W, float b, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    const size_t es = freeu_elem_size(dtype);
    if (!hidden || !workspace || B <= 0 || C <= 0 || H <= 0 || W <= 0 || es == 0) return FRESCO_EINVAL;
    if (n_scaled < 0 || n_scaled > C) return FRESCO_EINVAL;
    if (H < 2 || W < 2 || (int64_t)H * W > (1 << 26) || B > 65535) return FRESCO_EUNSUPPORTED;
    const int HW = H * W;
    if (cat && (cat == hidden || cat_batch_stride < (int64_t)C * HW)) return FRESCO_EINVAL;
    if (!aligned_to(hidden, es) || !aligned_to(cat, es) || !aligned_to(workspace, 16)) return FRESCO_EINVAL;
    const FreeuWorkspace lay = freeu_workspace(B, C, HW);
    if (workspace_bytes < lay.total) return FRESCO_EWORKSPACE;
    if ((C + FREEU_CPT - 1) / FREEU_CPT > 65535) return FRESCO_EUNSUPPORTED;  // grid.y of the scaling pass at its narrowest
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    if (dtype == FRESCO_F16)
        return freeu_backbone_launch(static_cast<half_t*>(hidden), static_cast<half_t*>(cat), cat_batch_stride, B, C,
                                     n_scaled, HW, b, ws, lay, st);
    if (dtype == FRESCO_BF16)
        return freeu_backbone_launch(static_cast<bf16_t*>(hidden), static_cast<bf16_t*>(cat), cat_batch_stride, B, C,
                                     n_scaled, HW, b, ws, lay, st);
    return freeu_backbone_launch(static_cast<float*>(hidden), static_cast<float*>(cat), cat_batch_stride, B, C, n_scaled,
                                 HW, b, ws, lay, st);
}
