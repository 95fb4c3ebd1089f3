// The statistics pass of GroupNorm(32) on NHWC rows of C channels, C a power of two from 64 to 1024: fp64 partial sums per
// (image, 256-pixel chunk, group), added in chunk order -> mean and 1 / sqrt(var + eps) per (image, group).  No atomics:
// same inputs, same bits.  midas.hip (fp32 rows) and vae.hip (fp16 rows) include it; their apply kernels are their own.
//
// LINKAGE: everything here sits in an unnamed namespace, so every file that includes it compiles ITS OWN kernels under ITS OWN
// flags.  That matters: midas.o is built with -ffp-contract=off and vae.o is not, and gn_finish_kernel's
// t2 / count - m * m rounds differently when it is contracted into an fma (gn_stats_kernel's d * d is exact in fp64 for
// fp16 and fp32 inputs, so it does not care).  With external linkage the two files' copies of one name would be merged
// when libfresco_hip.so is linked, and one of the two detectors would silently run the other's arithmetic.
#pragma once
#include "common.h"

namespace fresco {
namespace {

constexpr int GN_GROUPS = 32;
constexpr int GN_ROWS = 256;  // pixels per workgroup of the statistics pass

__device__ __forceinline__ floatx4 gn_load4(const float* p) { return *reinterpret_cast<const floatx4*>(p); }
__device__ __forceinline__ floatx4 gn_load4(const half_t* p) {
    const half4_t v = *reinterpret_cast<const half4_t*>(p);
    return floatx4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// grid (chunks, n).  Thread t owns the four channels 4 (t % Q) .. + 3, Q = C / 4 (a divisor of 256), of the pixels t / Q,
// t / Q + 256 / Q, ... of its chunk, and keeps one fp64 sum pair per HALF of them: two channels never straddle a group
// (C / 32 is even).  Thread g < 32 then adds the 512 halves that belong to group g in index order.
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ x, double* __restrict__ part, int P, int C,
                                                       int chunks) {
    __shared__ double s1[512], s2[512];
    const int Q = C >> 2, tid = threadIdx.x, q = tid % Q, step = 256 / Q;
    const int img = blockIdx.y, chunk = blockIdx.x;
    const int pb = chunk * GN_ROWS, pe = min(pb + GN_ROWS, P);
    double a1[2] = {0.0, 0.0}, a2[2] = {0.0, 0.0};
    for (int p = pb + tid / Q; p < pe; p += step) {
        const floatx4 v = gn_load4(x + ((int64_t)img * P + p) * C + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = (double)v[e];
            a1[e >> 1] += d;
            a2[e >> 1] += d * d;
        }
    }
    s1[tid * 2] = a1[0];
    s1[tid * 2 + 1] = a1[1];
    s2[tid * 2] = a2[0];
    s2[tid * 2 + 1] = a2[1];
    __syncthreads();
    if (tid < GN_GROUPS) {
        const int lcpg = 31 - __clz(C / GN_GROUPS);  // (C is a power of two: the launchers' channel lists)
        double t1 = 0.0, t2 = 0.0;
        for (int e = 0; e < 512; ++e) {
            const int ch = ((e >> 1) & (Q - 1)) * 4 + (e & 1) * 2;
            if ((ch >> lcpg) == tid) {
                t1 += s1[e];
                t2 += s2[e];
            }
        }
        double* o = part + (((int64_t)img * chunks + chunk) * GN_GROUPS + tid) * 2;
        o[0] = t1;
        o[1] = t2;
    }
}

__global__ __launch_bounds__(256) void gn_finish_kernel(const double* __restrict__ part, float* __restrict__ mean,
                                                        float* __restrict__ rstd, int n, int chunks, double count, float eps) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * GN_GROUPS) return;
    const int img = idx / GN_GROUPS, g = idx - img * GN_GROUPS;
    double t1 = 0.0, t2 = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double* o = part + (((int64_t)img * chunks + c) * GN_GROUPS + g) * 2;
        t1 += o[0];
        t2 += o[1];
    }
    const double m = t1 / count;
    double var = t2 / count - m * m;
    var = var > 0.0 ? var : 0.0;
    mean[idx] = (float)m;
    rstd[idx] = (float)(1.0 / sqrt(var + (double)eps));
}

// the partial sums of n images of P pixels, and (own_stats) room for mean and rstd behind them
inline size_t gn_workspace_bytes(int n, int P, bool own_stats) {
    const size_t chunks = ((size_t)P + GN_ROWS - 1) / GN_ROWS;
    const size_t stats = own_stats ? align_up((size_t)n * GN_GROUPS * 2 * sizeof(float), 8) : 0;
    return (size_t)n * chunks * GN_GROUPS * 2 * sizeof(double) + stats;
}

// Both launches on x (n, P, C).  mean / rstd: the caller's (n, 32) arrays, or both nullptr: they are put behind the partial
// sums in the workspace (gn_workspace_bytes(n, P, true)) and handed back.  The caller has checked the arguments: C a power
// of two in 64 .. 1024, n <= 65535, n P < 2^31, x aligned to four elements, the workspace 8-byte aligned and large enough.
template <typename T>
inline int gn_statistics(const T* x, void* workspace, float*& mean, float*& rstd, int n, int P, int C, float eps,
                         hipStream_t st) {
    const int chunks = (P + GN_ROWS - 1) / GN_ROWS;
    double* part = static_cast<double*>(workspace);
    if (!mean) {
        mean = reinterpret_cast<float*>(part + (size_t)n * chunks * GN_GROUPS * 2);
        rstd = mean + (size_t)n * GN_GROUPS;
    }
    hipLaunchKernelGGL(gn_stats_kernel<T>, dim3(chunks, n), dim3(256), 0, st, x, part, P, C, chunks);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(gn_finish_kernel, dim3((n * GN_GROUPS + 255) / 256), dim3(256), 0, st, part, mean, rstd, n, chunks,
                       (double)P * (C / GN_GROUPS), eps);
    return check_launch();
}

}  // namespace
}  // namespace fresco
