// What a UNet ResnetBlock2D of fp16 pipelines needs beside vae.hip's convolution: include/fresco_unet.h, DESIGN.md section 19.
//
//   unet_gn_lds_kernel      GroupNorm(32) [+ SiLU] of x + addend in ONE launch and ONE read of x: the plane waits in LDS
//   unet_gn_stats_kernel / unet_gn_finish_kernel / unet_gn_apply_kernel
//                           the same in three launches where the plane does not fit: fp64 partial sums per 64 pixels, added
//                           in chunk order, then the apply pass (x is read twice)
//   unet_temb_kernel        out = bias + conv_bias + W SiLU(temb): one wave per output channel, all images at once
//
// WIDTHS.  C is a multiple of 64 (64 .. 2560), so a group is cpg = C / 32 channels, an even number of them: a PAIR of
// channels (2 c, 2 c + 1) never straddles two groups, but a 16-byte piece (8 channels) may: at C = 320 a group is 20 bytes.
// Every thread of the three GroupNorm kernels owns ONE piece COLUMN for its whole life (thread t: column t % ncols, rows
// t / ncols, t / ncols + 512 / ncols, ...; the threads beyond (512 / ncols) ncols idle), so the group of each of its four
// pairs, its addend, gamma and beta are fixed registers, and it keeps one fp64 (sum, sum of squares) per pair.
//
// SUMMATION ORDER (fixed; no atomics): a thread adds its rows in row order; the 512 x 4 pair sums go to LDS (32 KiB,
// static) and are folded in four short steps, each by many threads and each in index order, in place: (1a) per (column,
// pair) the row slots s, s + S, .. of each of S interleaved sub-ranges (S a power of two <= 16), (1b) per (column, pair) the
// S sub-ranges, (2a) per group eight interleaved shares of its pairs, (2b) per group the eight shares.  A single thread
// per sum (the first version) cost 102 + 20 dependent LDS reads at 8 x 8 and left the kernel at 10 us for 5 MB.  The
// three-launch form adds the chunks in chunk order in the finish kernel.
//
// THE LDS FORM.  Global reads must be aligned 16-byte pieces, so a workgroup takes a SLAB: the smallest run of G whole
// groups whose bytes are a multiple of 16 (G = 1, 2 or 4: C = 320: 4 groups = 80 bytes, 640: 2 = 80, 960: 4 = 240,
// 1280: 1 = 80, 1920: 2 = 240, 2560: 1 = 160), of ONE image: grid (32 / G, n).  Its plane is P x 2 G cpg bytes of dynamic
// LDS, written and read back by the same thread (no barrier for it; consecutive threads, consecutive 16 bytes).  The switch:
//   UG_LDS_PLANE_BYTES = 96 KiB: the LDS form runs where P x 2 G cpg <= 96 KiB.
// A CU has 160 KiB; beside the plane stand 32 KiB + 512 bytes + 256 bytes of static LDS (the pair sums, the group sums, mean
// and rstd).  96 KiB leaves the total at 128.75 KiB, holds every plane of the SD-1.5 UNet at 8 x 8, 16 x 16 (all six widths: at
// most 60 KiB) and 32 x 32 at 640 and 1280 (80 KiB), and one workgroup per CU is what any plane above 64 KiB leaves anyway.
// 32 x 32 at 960 and 1920 (240 KiB) and every 64 x 64 plane take the three-launch form.  Planes above 64 KiB - the static
// part go through common.h's allow_dyn_lds.
//
// THE THREE-LAUNCH FORM reads WHOLE rows (ncols = C / 8 <= 320 columns; a slab's 80-byte runs would split cache lines
// between workgroups): grid (chunks of UG_ROWS = 64 pixels, n) for the statistics and for the apply pass.
//
// unet_temb_kernel: 256 threads = four waves = four output channels.  K is walked in chunks of 512: a lane holds 8 weights
// of its channel (one 16-byte load, read ONCE), SiLU(temb) of 16 images x 512 k stands in LDS as fp32 (32 KiB, static) and
// is rebuilt per tile of 16 images under the same weights; a lane adds its 8 products in k order into one fp32 accumulator
// per image (64 registers), chunks in order, then a butterfly over the 64 lanes.
#include "common.h"
#include "../../include/fresco_unet.h"

namespace fresco {

constexpr int UG_GROUPS = 32;
constexpr int UG_THREADS = 512;
constexpr int UG_ROWS = 64;                       // pixels per workgroup of the three-launch form
constexpr int UG_LDS_PLANE_BYTES = 96 * 1024;     // the switch between the two forms (header comment)
constexpr int UG_STATIC_LDS = 2 * UG_THREADS * 4 * 8 + 2 * UG_GROUPS * 8 + 2 * UG_GROUPS * 4;
constexpr int UG_MIN_WORKSPACE = 256;
constexpr int UT_KC = 512, UT_IT = 16, UT_NMAX = 64;

struct UgArgs {
    const half_t* x;
    const float* addend;
    const float* gamma;
    const float* beta;
    half_t* y;
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

__device__ __forceinline__ void ug_accumulate(const half8_t v, const float (&ad)[8], double (&a1)[4], double (&a2)[4]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const double d = (double)((float)v[e] + ad[e]);
        a1[e >> 1] += d;
        a2[e >> 1] += d * d;
    }
}

__device__ __forceinline__ half8_t ug_normalise(const half8_t v, const UgLane& L, const float (&mu)[4], const float (&rs)[4],
                                                int silu) {
    half8_t o8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float o = (((float)v[e] + L.ad[e]) - mu[e >> 1]) * rs[e >> 1] * L.ga[e] + L.be[e];
        if (silu) o = o / (1.f + expf(-o));
        o8[e] = (half_t)o;
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
__global__ __launch_bounds__(UG_THREADS) void unet_gn_lds_kernel(const UgArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ug_plane[];
    __shared__ double s1[UG_THREADS * 4], s2[UG_THREADS * 4], g1[UG_GROUPS], g2[UG_GROUPS];
    __shared__ float smean[UG_GROUPS], srstd[UG_GROUPS];
    half8_t* plane = reinterpret_cast<half8_t*>(ug_plane);
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
            const half8_t v = *reinterpret_cast<const half8_t*>(a.x + base + (int64_t)r * a.C);
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
        *reinterpret_cast<half8_t*>(a.y + base + (int64_t)r * a.C) = ug_normalise(plane[r * ncols + col], L, mu, rsd, a.silu);
}

// grid (chunks, n): rows [chunk UG_ROWS, ..) of one image, whole rows (ncols = C / 8).
__global__ __launch_bounds__(UG_THREADS) void unet_gn_stats_kernel(const UgArgs a) {
    __shared__ double s1[UG_THREADS * 4], s2[UG_THREADS * 4], g1[UG_GROUPS], g2[UG_GROUPS];
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
            ug_accumulate(*reinterpret_cast<const half8_t*>(a.x + base + (int64_t)r * a.C), ad, a1, a2);
    }
    ug_reduce(a1, a2, s1, s2, g1, g2, ncols, rs, a.cpg >> 1, UG_GROUPS);
    if (tid < UG_GROUPS) {
        double* o = a.part + (((int64_t)img * a.chunks + chunk) * UG_GROUPS + tid) * 2;
        o[0] = g1[tid];
        o[1] = g2[tid];
    }
}

__global__ __launch_bounds__(256) void unet_gn_finish_kernel(const double* __restrict__ part, float* __restrict__ mean,
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
__global__ __launch_bounds__(UG_THREADS) void unet_gn_apply_kernel(const UgArgs a) {
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
        *reinterpret_cast<half8_t*>(a.y + off) = ug_normalise(*reinterpret_cast<const half8_t*>(a.x + off), L, mu, rsd, a.silu);
    }
}

// grid (ceil(cout / 4)); wave w: output channel 4 blockIdx.x + w.  TILES = ceil(n / 16): images >= n are zero rows in LDS.
template <int TILES>
__global__ __launch_bounds__(256) void unet_temb_kernel(const half_t* __restrict__ temb, const half_t* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ cbias,
                                                        float* __restrict__ out, int n, int K, int cout) {
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
            for (int idx = tid; idx < UT_IT * (UT_KC / 8); idx += 256) {
                const int i = idx >> 6, kk = (idx & 63) * 8, gi = t * UT_IT + i;
                half8_t t8;
#pragma unroll
                for (int e = 0; e < 8; ++e) t8[e] = (half_t)0.f;
                if (gi < n && k0 + kk < K) t8 = *reinterpret_cast<const half8_t*>(temb + (int64_t)gi * K + k0 + kk);
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

static inline bool ug_channels(int C) { return C >= 64 && C <= 2560 && C % 64 == 0; }

struct UgPlan {
    int cpg, G, sc, chunks;
    bool lds;
    int plane;
};

// the caller has checked n, P > 0 and ug_channels(C)
static inline UgPlan ug_plan(int P, int C) {
    UgPlan p;
    p.cpg = C / UG_GROUPS;
    p.G = p.cpg % 8 == 0 ? 1 : (p.cpg % 4 == 0 ? 2 : 4);  // the fewest groups whose 2 cpg G bytes are a multiple of 16
    p.sc = p.G * p.cpg;
    p.chunks = (P + UG_ROWS - 1) / UG_ROWS;
    const int64_t plane = (int64_t)P * p.sc * 2;
    p.lds = plane <= UG_LDS_PLANE_BYTES;
    p.plane = p.lds ? (int)plane : 0;
    return p;
}

static inline size_t ug_workspace(int n, int P, int C) {
    const UgPlan p = ug_plan(P, C);
    if (p.lds) return UG_MIN_WORKSPACE;
    return (size_t)n * p.chunks * UG_GROUPS * 2 * sizeof(double) + align_up((size_t)n * UG_GROUPS * 2 * sizeof(float), 256);
}

}  // namespace fresco

using namespace fresco;

extern "C" size_t unet_groupnorm_workspace_bytes(int n, int P, int C) {
    if (n <= 0 || P <= 0 || !ug_channels(C)) return 0;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return 0;
    return ug_workspace(n, P, C);
}

extern "C" int unet_groupnorm_lds_form(int n, int P, int C) {
    if (n <= 0 || P <= 0 || !ug_channels(C)) return -1;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return -1;
    return ug_plan(P, C).lds ? 1 : 0;
}

extern "C" int unet_groupnorm(const void* x, const float* addend, const float* gamma, const float* beta, void* y, void* workspace,
                              size_t workspace_bytes, int n, int P, int C, float eps, int silu, void* stream) {
    if (!x || !gamma || !beta || !y || !workspace || n <= 0 || P <= 0 || C <= 0 || !(eps >= 0.f)) return FRESCO_EINVAL;
    if (!ug_channels(C)) return FRESCO_EUNSUPPORTED;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(y, 16) || !aligned_to(workspace, 8) || !aligned_to(gamma, 16) || !aligned_to(beta, 16) ||
        !aligned_to(addend, 16))
        return FRESCO_EINVAL;
    if (workspace_bytes < ug_workspace(n, P, C)) return FRESCO_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const UgPlan p = ug_plan(P, C);
    UgArgs a;
    a.x = static_cast<const half_t*>(x);
    a.addend = addend;
    a.gamma = gamma;
    a.beta = beta;
    a.y = static_cast<half_t*>(y);
    a.part = nullptr;
    a.mean = a.rstd = nullptr;
    a.P = P;
    a.C = C;
    a.cpg = p.cpg;
    a.sc = p.sc;
    a.chunks = p.chunks;
    a.silu = silu ? 1 : 0;
    a.eps = eps;
    if (p.lds) {
        a.ncols = p.sc / 8;
        a.ngroups = p.G;
        if (p.plane + UG_STATIC_LDS > 64 * 1024)
            if (int rc = allow_dyn_lds(unet_gn_lds_kernel, p.plane)) return rc;
        hipLaunchKernelGGL(unet_gn_lds_kernel, dim3(UG_GROUPS / p.G, n), dim3(UG_THREADS), p.plane, st, a);
        return check_launch();
    }
    a.ncols = C / 8;
    a.ngroups = UG_GROUPS;
    a.part = static_cast<double*>(workspace);
    a.mean = reinterpret_cast<float*>(a.part + (size_t)n * p.chunks * UG_GROUPS * 2);
    a.rstd = a.mean + (size_t)n * UG_GROUPS;
    hipLaunchKernelGGL(unet_gn_stats_kernel, dim3(p.chunks, n), dim3(UG_THREADS), 0, st, a);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(unet_gn_finish_kernel, dim3((n * UG_GROUPS + 255) / 256), dim3(256), 0, st, a.part, a.mean, a.rstd, n,
                       p.chunks, (double)P * p.cpg, eps);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(unet_gn_apply_kernel, dim3(p.chunks, n), dim3(UG_THREADS), 0, st, a);
    return check_launch();
}

extern "C" int unet_temb(const void* temb, const void* weight, const float* bias, const float* conv_bias, float* out, int n,
                         int K, int cout, void* stream) {
    if (!temb || !weight || !bias || !conv_bias || !out || n <= 0 || K <= 0 || cout <= 0) return FRESCO_EINVAL;
    if (n > UT_NMAX || K % 8) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(temb, 16) || !aligned_to(weight, 16) || !aligned_to(bias, 4) || !aligned_to(conv_bias, 4) || !aligned_to(out, 4))
        return FRESCO_EINVAL;
    auto kern = n <= UT_IT ? unet_temb_kernel<1> : (n <= 2 * UT_IT ? unet_temb_kernel<2> : (n <= 3 * UT_IT ? unet_temb_kernel<3> : unet_temb_kernel<4>));
    hipLaunchKernelGGL(kern, dim3((cout + 3) / 4), dim3(256), 0, as_stream(stream), static_cast<const half_t*>(temb),
                       static_cast<const half_t*>(weight), bias, conv_bias, out, n, K, cout);
    return check_launch();
}
