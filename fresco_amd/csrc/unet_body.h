// unet.hip's GroupNorm and time-embedding kernels (unet.hip's header comment describes them) as ONE text for both 16-bit
// element types, templates over the element type T: unet.hip instantiates and launches the half_t forms, net_bf16.hip the
// bf16_t forms.  x, y (GroupNorm) and temb, W (unet_temb) are T; the addend, gamma, beta, biases and unet_temb's output are
// fp32, the statistics fp64, for both types.  Slabs, planes and pieces are counted in BYTES and both types have 2-byte
// elements, so the plan (unet.hip's ug_plan), the grids, the LDS sizes and the summation order do not depend on T.
// (The kernels are the templates themselves, not wrappers around forceinline bodies: taken by reference, the LDS-form body
// compiled to 182 registers instead of 80.  As templates the fp16 instantiations are instruction for instruction what they
// were when this text stood in unet.hip: DESIGN.md section 19.)
#pragma once
#include "common.h"

namespace fresco {

constexpr int UG_GROUPS = 32;
constexpr int UG_THREADS = 512;
constexpr int UG_ROWS = 64;                       // pixels per workgroup of the three-launch form
constexpr int UT_KC = 512, UT_IT = 16, UT_NMAX = 64;

struct UgArgs {
    const void* x;  // T
    const float* addend;
    const float* gamma;
    const float* beta;
    void* y;        // T
    double* part;
    float* mean;
    float* rstd;
    int P, C, cpg, ncols, sc, ngroups, chunks, silu;
    float eps;
};

struct UgLane {
    float ad[8], ga[8], be[8];
};

__device__ __forceinline__ void ug_load8(const float* p, float (&o)[8]) {
    const floatx4 a = *reinterpret_cast<const floatx4*>(p), b = *reinterpret_cast<const floatx4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o[e] = a[e];
        o[4 + e] = b[e];
    }
}

template <typename T8>
__device__ __forceinline__ void ug_accumulate(const T8 v, const float (&ad)[8], double (&a1)[4], double (&a2)[4]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const double d = (double)((float)v[e] + ad[e]);
        a1[e >> 1] += d;
        a2[e >> 1] += d * d;
    }
}

template <typename T>
__device__ __forceinline__ typename Elem<T>::x8 ug_normalise(const typename Elem<T>::x8 v, const UgLane& L, const float (&mu)[4],
                                                             const float (&rs)[4], int silu) {
    typename Elem<T>::x8 o8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float o = (((float)v[e] + L.ad[e]) - mu[e >> 1]) * rs[e >> 1] * L.ga[e] + L.be[e];
        if (silu) o = o / (1.f + expf(-o));
        o8[e] = Elem<T>::from_float(o);
    }
    return o8;
}

// The pair sums of all 512 threads -> g1[g], g2[g] for the workgroup's groups g < ngroups (header comment: SUMMATION ORDER).
// Thread slot * ncols + col holds pairs 4 col .. 4 col + 3 of its columns; rs = row slots in use; cpg2 = pairs per group.
// Entry (slot, j) of s1 / s2 is s * width + j, width = 4 ncols <= 1280; every step writes only entries that no other thread
// of that step reads.
__device__ __forceinline__ void ug_reduce(const double (&a1)[4], const double (&a2)[4], double* s1, double* s2, double* g1,
                                          double* g2, int ncols, int rs, int cpg2, int ngroups) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s1[tid * 4 + k] = a1[k];
        s2[tid * 4 + k] = a2[k];
    }
    __syncthreads();
    const int width = ncols * 4;
    int S = 1;
    while (S < 16 && 2 * S * width <= UG_THREADS) S *= 2;
    // (1a) thread (sub, j): slots sub, sub + S, ... -> entry (sub, j), the first it read
    for (int t = tid; t < S * width; t += UG_THREADS) {
        const int sub = t / width, j = t - sub * width;
        double t1 = 0.0, t2 = 0.0;
        for (int sl = sub; sl < rs; sl += S) {
            t1 += s1[sl * width + j];
            t2 += s2[sl * width + j];
        }
        s1[t] = t1;
        s2[t] = t2;
    }
    __syncthreads();
    // (1b) thread j: the S sub-ranges -> entry (0, j)
    if (S > 1 && tid < width) {
        double t1 = 0.0, t2 = 0.0;
        for (int sub = 0; sub < S; ++sub) {
            t1 += s1[sub * width + tid];
            t2 += s2[sub * width + tid];
        }
        s1[tid] = t1;
        s2[tid] = t2;
    }
    __syncthreads();
    // (2a) thread (g, share): pairs g cpg2 + share, + 8, ... of group g -> entry width + 8 g + share (behind the live ones)
    if (tid < ngroups * 8) {
        const int g = tid >> 3, share = tid & 7;
        double t1 = 0.0, t2 = 0.0;
        for (int p = share; p < cpg2; p += 8) {
            t1 += s1[g * cpg2 + p];
            t2 += s2[g * cpg2 + p];
        }
        s1[width + tid] = t1;
        s2[width + tid] = t2;
    }
    __syncthreads();
    // (2b) thread g: its eight shares
    if (tid < ngroups) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            t1 += s1[width + tid * 8 + r];
            t2 += s2[width + tid * 8 + r];
        }
        g1[tid] = t1;
        g2[tid] = t2;
    }
    __syncthreads();
}

__device__ __forceinline__ void ug_mean_rstd(double t1, double t2, double count, float eps, float& mean, float& rstd) {
    const double m = t1 / count;
    double var = t2 / count - m * m;
    var = var > 0.0 ? var : 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// grid (32 / G slabs, n); dynamic LDS: the slab's plane, P x ncols pieces of 16 bytes.
template <typename T>
__global__ __launch_bounds__(UG_THREADS) void unet_gn_lds_kernel_t(const UgArgs a) {
    typedef typename Elem<T>::x8 T8;
    extern __shared__ __attribute__((aligned(16))) char ug_plane[];
    __shared__ double s1[UG_THREADS * 4], s2[UG_THREADS * 4], g1[UG_GROUPS], g2[UG_GROUPS];
    __shared__ float smean[UG_GROUPS], srstd[UG_GROUPS];
    T8* plane = reinterpret_cast<T8*>(ug_plane);
    const T* ax = static_cast<const T*>(a.x);
    T* ay = static_cast<T*>(a.y);
    const int tid = threadIdx.x, ncols = a.ncols, rs = UG_THREADS / ncols;
    const int col = tid % ncols, slot = tid / ncols;
    const int img = blockIdx.y, c0 = blockIdx.x * a.sc + col * 8;
    const bool active = slot < rs;
    UgLane L;
#pragma unroll
    for (int e = 0; e < 8; ++e) L.ad[e] = 0.f;
    if (a.addend) ug_load8(a.addend + (int64_t)img * a.C + c0, L.ad);
    ug_load8(a.gamma + c0, L.ga);
    ug_load8(a.beta + c0, L.be);
    const int64_t base = (int64_t)img * a.P * a.C + c0;
    double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
#pragma unroll 8
        for (int r = slot; r < a.P; r += rs) {
            const T8 v = *reinterpret_cast<const T8*>(ax + base + (int64_t)r * a.C);
            plane[r * ncols + col] = v;
            ug_accumulate(v, L.ad, a1, a2);
        }
    }
    ug_reduce(a1, a2, s1, s2, g1, g2, ncols, rs, a.cpg >> 1, a.ngroups);
    if (tid < a.ngroups) ug_mean_rstd(g1[tid], g2[tid], (double)a.P * a.cpg, a.eps, smean[tid], srstd[tid]);
    __syncthreads();
    if (!active) return;
    float mu[4], rsd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int g = (col * 8 + 2 * k) / a.cpg;
        mu[k] = smean[g];
        rsd[k] = srstd[g];
    }
#pragma unroll 4
    for (int r = slot; r < a.P; r += rs)
        *reinterpret_cast<T8*>(ay + base + (int64_t)r * a.C) = ug_normalise<T>(plane[r * ncols + col], L, mu, rsd, a.silu);
}

// grid (chunks, n): rows [chunk UG_ROWS, ..) of one image, whole rows (ncols = C / 8).
template <typename T>
__global__ __launch_bounds__(UG_THREADS) void unet_gn_stats_kernel_t(const UgArgs a) {
    typedef typename Elem<T>::x8 T8;
    __shared__ double s1[UG_THREADS * 4], s2[UG_THREADS * 4], g1[UG_GROUPS], g2[UG_GROUPS];
    const T* ax = static_cast<const T*>(a.x);
    const int tid = threadIdx.x, ncols = a.ncols, rs = UG_THREADS / ncols;
    const int col = tid % ncols, slot = tid / ncols;
    const int img = blockIdx.y, chunk = blockIdx.x, c0 = col * 8;
    const int r0 = chunk * UG_ROWS, r1 = min(r0 + UG_ROWS, a.P);
    float ad[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) ad[e] = 0.f;
    if (a.addend) ug_load8(a.addend + (int64_t)img * a.C + c0, ad);
    const int64_t base = (int64_t)img * a.P * a.C + c0;
    double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[4] = {0.0, 0.0, 0.0, 0.0};
    if (slot < rs) {
#pragma unroll 4
        for (int r = r0 + slot; r < r1; r += rs)
            ug_accumulate(*reinterpret_cast<const T8*>(ax + base + (int64_t)r * a.C), ad, a1, a2);
    }
    ug_reduce(a1, a2, s1, s2, g1, g2, ncols, rs, a.cpg >> 1, UG_GROUPS);
    if (tid < UG_GROUPS) {
        double* o = a.part + (((int64_t)img * a.chunks + chunk) * UG_GROUPS + tid) * 2;
        o[0] = g1[tid];
        o[1] = g2[tid];
    }
}

// one thread per (image, group): the chunks' partial sums in chunk order.  (No element type in it: T only names the twin, so
// that each file that includes this header emits its own kernel and the library links without a duplicate symbol.)
template <typename T>
__global__ __launch_bounds__(256) void unet_gn_finish_kernel_t(const double* __restrict__ part, float* __restrict__ mean,
                                                               float* __restrict__ rstd, int n, int chunks, double count,
                                                               float eps) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * UG_GROUPS) return;
    const int img = idx / UG_GROUPS, g = idx - img * UG_GROUPS;
    double t1 = 0.0, t2 = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double* o = part + (((int64_t)img * chunks + c) * UG_GROUPS + g) * 2;
        t1 += o[0];
        t2 += o[1];
    }
    ug_mean_rstd(t1, t2, count, eps, mean[idx], rstd[idx]);
}

// grid (chunks, n), the statistics pass's rows and columns.
template <typename T>
__global__ __launch_bounds__(UG_THREADS) void unet_gn_apply_kernel_t(const UgArgs a) {
    typedef typename Elem<T>::x8 T8;
    const T* ax = static_cast<const T*>(a.x);
    T* ay = static_cast<T*>(a.y);
    const int tid = threadIdx.x, ncols = a.ncols, rs = UG_THREADS / ncols;
    const int col = tid % ncols, slot = tid / ncols;
    if (slot >= rs) return;
    const int img = blockIdx.y, c0 = col * 8;
    const int r0 = blockIdx.x * UG_ROWS, r1 = min(r0 + UG_ROWS, a.P);
    UgLane L;
#pragma unroll
    for (int e = 0; e < 8; ++e) L.ad[e] = 0.f;
    if (a.addend) ug_load8(a.addend + (int64_t)img * a.C + c0, L.ad);
    ug_load8(a.gamma + c0, L.ga);
    ug_load8(a.beta + c0, L.be);
    float mu[4], rsd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int g = (c0 + 2 * k) / a.cpg;
        mu[k] = a.mean[img * UG_GROUPS + g];
        rsd[k] = a.rstd[img * UG_GROUPS + g];
    }
    const int64_t base = (int64_t)img * a.P * a.C + c0;
#pragma unroll 4
    for (int r = r0 + slot; r < r1; r += rs) {
        const int64_t off = base + (int64_t)r * a.C;
        *reinterpret_cast<T8*>(ay + off) = ug_normalise<T>(*reinterpret_cast<const T8*>(ax + off), L, mu, rsd, a.silu);
    }
}

// grid (ceil(cout / 4)); wave w: output channel 4 blockIdx.x + w.  TILES = ceil(n / 16): images >= n are zero rows in LDS.
template <int TILES, typename T>
__global__ __launch_bounds__(256) void unet_temb_kernel_t(const T* __restrict__ temb, const T* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ cbias,
                                                          float* __restrict__ out, int n, int K, int cout) {
    typedef typename Elem<T>::x8 T8;
    __shared__ __attribute__((aligned(16))) float s[UT_IT][UT_KC];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int co = blockIdx.x * 4 + wave;
    const bool has = co < cout;
    float acc[TILES * UT_IT];
#pragma unroll
    for (int i = 0; i < TILES * UT_IT; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < K; k0 += UT_KC) {
        float wf[8];
        {
            const int k = k0 + lane * 8;  // (K % 8 == 0: a piece is inside the row or outside it)
            T8 w8;
#pragma unroll
            for (int e = 0; e < 8; ++e) w8[e] = (T)0.f;
            if (has && k < K) w8 = *reinterpret_cast<const T8*>(w + (int64_t)co * K + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[e] = (float)w8[e];
        }
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            __syncthreads();
            for (int idx = tid; idx < UT_IT * (UT_KC / 8); idx += 256) {
                const int i = idx >> 6, kk = (idx & 63) * 8, gi = t * UT_IT + i;
                T8 t8;
#pragma unroll
                for (int e = 0; e < 8; ++e) t8[e] = (T)0.f;
                if (gi < n && k0 + kk < K) t8 = *reinterpret_cast<const T8*>(temb + (int64_t)gi * K + k0 + kk);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = (float)t8[e];
                    s[i][kk + e] = v / (1.f + expf(-v));
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < UT_IT; ++i) {
                const floatx4 p0 = *reinterpret_cast<const floatx4*>(&s[i][lane * 8]);
                const floatx4 p1 = *reinterpret_cast<const floatx4*>(&s[i][lane * 8 + 4]);
                float v = acc[t * UT_IT + i];
#pragma unroll
                for (int e = 0; e < 4; ++e) v += p0[e] * wf[e];
#pragma unroll
                for (int e = 0; e < 4; ++e) v += p1[e] * wf[4 + e];
                acc[t * UT_IT + i] = v;
            }
        }
    }
    const float b = has ? bias[co] + cbias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < TILES * UT_IT; ++i) {
        const float v = wave_sum(acc[i]);
        if (lane == 0 && has && i < n) out[(int64_t)i * cout + co] = v + b;
    }
}

// net_bf16.hip: the launches of unet_groupnorm and unet_temb for bf16 operands.  unet.hip has checked the arguments, made the
// plan and filled `a`.  lds_form: grid (slabs, n) with `plane` bytes of dynamic LDS, which goes through allow_dyn_lds where
// `plane_needs_leave` says that it passes 64 KiB with the static part; otherwise the three launches over (chunks, n).
int unet_groupnorm_launch_bf16(const UgArgs& a, bool lds_form, int slabs, int plane, bool plane_needs_leave, int n, double count,
                               hipStream_t st);
int unet_temb_launch_bf16(const void* temb, const void* weight, const float* bias, const float* conv_bias, float* out, int n, int K,
                          int cout, hipStream_t st);

}  // namespace fresco
