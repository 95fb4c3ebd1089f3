// Histogram + Poisson blending of the two Ebsynth propagations of an in-between frame: the per-frame step of FRESCO's
// video_blend.py process_seq (error mask with flow propagation, min-error image, Lab mean / std transfer, gradient-domain
// fusion), written for gfx950 from its description; DESIGN.md section 10 has the semantics kept and the departures.
//
// One frame (fresco_blend_frame, gradient blending on) is 9 launches on the caller's stream, no host synchronisation:
//   memset   the 21 integer statistics
//   prep     BGR -> Lab of both propagations, error mask | warped previous mask, exact uint64 channel sums
//   tables   orthonormal DCT-II matrices C_h, C_h^T, C_w, C_w^T and the path-Laplacian eigenvalues
//   rhs      histogram transfer -> BGR -> Lab again, and the normal-equation right-hand side w^2 (Gx^T gx + Gy^T gy) + im
//   4 GEMMs  x = C_h^T [(C_h R C_w^T) / (1 + w^2 (lam_i + mu_j))] C_w, batched over L, a, b
//   finish   Lab -> BGR
// Without gradient blending the frame is the first three of these (rhs writes the histogram blend's BGR).
//
// Colour conversions and the mask warp are fp64 / non-contracted fp32 (this file builds with -ffp-contract=off) so they
// follow the numpy restatement of tests/blend_model.py operation by operation; the GEMMs use explicit fmaf inside a
// k-step and sum the k-steps in fp64.
#include <cmath>

#include "common.h"
#include "warp_nearest.h"

namespace fresco {
namespace {

constexpr int kBlendMaxSide = 4096;
constexpr int kStats = 21;  // per channel: sum a, a^2, b, b^2, a b, min-error, min-error^2 (Lab bytes)
constexpr int kGemmTile = 64, kGemmK = 16;
constexpr float kTruncGuard = 1.0f / 1024;  // grey levels added before the truncation

// ---------------------------------------------------------------------------------------------------------------------
// OpenCV's documented 8-bit BGR <-> Lab formula (sRGB gamma, D65 white, the 0.008856 / 7.787 / 903.3 branches)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t sat_u8(double v) {
    v = rint(v);
    return uint8_t(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

__device__ __forceinline__ double srgb_to_linear(double c) {
    return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
}

__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }

__device__ __forceinline__ void bgr_to_lab(uint8_t B, uint8_t G, uint8_t R, uint8_t* lab) {
    const double r = srgb_to_linear(R / 255.0), g = srgb_to_linear(G / 255.0), b = srgb_to_linear(B / 255.0);
    const double X = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.950456;
    const double Y = 0.212671 * r + 0.715160 * g + 0.072169 * b;
    const double Z = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.088754;
    const double fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
    const double L = Y > 0.008856 ? 116.0 * cbrt(Y) - 16.0 : 903.3 * Y;
    lab[0] = sat_u8(L * 255.0 / 100.0);
    lab[1] = sat_u8(500.0 * (fx - fy) + 128.0);
    lab[2] = sat_u8(200.0 * (fy - fz) + 128.0);
}

__device__ __forceinline__ double lab_finv(double f) {
    return f <= 7.787 * 0.008856 + 16.0 / 116.0 ? (f - 16.0 / 116.0) / 7.787 : f * f * f;
}

__device__ __forceinline__ double linear_to_srgb(double c) {
    c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
    return c <= 0.0031308 ? 12.92 * c : 1.055 * pow(c, 1.0 / 2.4) - 0.055;
}

__device__ __forceinline__ void lab_to_bgr(uint8_t L8, uint8_t a8, uint8_t b8, uint8_t* bgr) {
    const double li = L8 * 100.0 / 255.0, ai = a8 - 128.0, bi = b8 - 128.0;
    double y, fy;
    if (li <= 903.3 * 0.008856) {
        y = li / 903.3;
        fy = 7.787 * y + 16.0 / 116.0;
    } else {
        fy = (li + 16.0) / 116.0;
        y = fy * fy * fy;
    }
    const double x = lab_finv(fy + ai / 500.0) * 0.950456;
    const double z = lab_finv(fy - bi / 200.0) * 1.088754;
    const double R = 3.240479 * x - 1.53715 * y - 0.498535 * z;
    const double G = -0.969256 * x + 1.875991 * y + 0.041556 * z;
    const double B = 0.055648 * x - 0.204043 * y + 1.057311 * z;
    bgr[0] = sat_u8(linear_to_srgb(B) * 255.0);
    bgr[1] = sat_u8(linear_to_srgb(G) * 255.0);
    bgr[2] = sat_u8(linear_to_srgb(R) * 255.0);
}

__global__ __launch_bounds__(256) void blend_bgr2lab(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) bgr_to_lab(in[3 * i], in[3 * i + 1], in[3 * i + 2], out + 3 * i);
}

__global__ __launch_bounds__(256) void blend_lab2bgr(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) lab_to_bgr(in[3 * i], in[3 * i + 1], in[3 * i + 2], out + 3 * i);
}

// ---------------------------------------------------------------------------------------------------------------------
// prep: Lab of both propagations, the mask, the integer statistics
// ---------------------------------------------------------------------------------------------------------------------
enum PrepMode { kPrepFrame = 0, kPrepHist = 1, kPrepLabOnly = 2 };

struct PrepArgs {
    const uint8_t *a, *b, *min_error;  // BGR; min_error only for kPrepHist
    const float *d1, *d2;              // kPrepFrame
    const uint8_t* prev;               // kPrepFrame, nullable
    const float* flow;                 // (2, h, w), x plane first; with prev
    double weight1;
    int w, h;
    uint8_t *lab_a, *lab_b, *mask;     // mask: written by kPrepFrame
    unsigned long long* stats;         // kStats counters, zeroed before the launch (not kPrepLabOnly)
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256) void blend_prep(PrepArgs p) {
    const int n = p.w * p.h;
    unsigned int acc[kStats];
#pragma unroll
    for (int s = 0; s < kStats; ++s) acc[s] = 0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        uint8_t la[3], lb[3], lm[3];
        bgr_to_lab(p.a[3 * q], p.a[3 * q + 1], p.a[3 * q + 2], la);
        bgr_to_lab(p.b[3 * q], p.b[3 * q + 1], p.b[3 * q + 2], lb);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p.lab_a[3 * q + c] = la[c];
            p.lab_b[3 * q + c] = lb[c];
        }
        if (MODE == kPrepLabOnly) continue;
        if (MODE == kPrepFrame) {
            // video_blend.py g_error_mask: weights and errors compared in double
            const double w1 = p.weight1, w2 = 1.0 - p.weight1;
            uint8_t m;
            if (w1 == 0.0)
                m = 0;
            else if (w2 == 0.0)
                m = 1;
            else
                m = w1 * double(p.d1[q]) < w2 * double(p.d2[q]) ? 0 : 1;
            if (p.prev) m |= warp_nearest(p.prev, p.flow, q % p.w, q / p.w, p.w, p.h);
            p.mask[q] = m;
#pragma unroll
            for (int c = 0; c < 3; ++c) lm[c] = m ? lb[c] : la[c];
        } else {
            bgr_to_lab(p.min_error[3 * q], p.min_error[3 * q + 1], p.min_error[3 * q + 2], lm);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned int A = la[c], B = lb[c], M = lm[c];
            acc[7 * c + 0] += A;
            acc[7 * c + 1] += A * A;
            acc[7 * c + 2] += B;
            acc[7 * c + 3] += B * B;
            acc[7 * c + 4] += A * B;
            acc[7 * c + 5] += M;
            acc[7 * c + 6] += M * M;
        }
    }
    if (MODE == kPrepLabOnly) return;
    // integer sums: exact, so the order of the block partials and of the atomics does not matter
    __shared__ unsigned long long red[4][kStats];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < kStats; ++s) {
        const unsigned long long v = wave_sum_u64(acc[s]);
        if (lane == 0) red[wave][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < kStats) {
        const int s = threadIdx.x;
        atomicAdd(p.stats + s, red[0][s] + red[1][s] + red[2][s] + red[3][s]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// rhs: histogram blend (and its BGR), then the Poisson right-hand side
// ---------------------------------------------------------------------------------------------------------------------
struct RhsArgs {
    const uint8_t *lab_a, *lab_b, *mask;
    const unsigned long long* stats;  // FROM_HIST
    const uint8_t* blend_bgr;         // !FROM_HIST: the image whose Lab is the data term
    double hw1, hw2;                  // histogram weights (1 - weight1, 1 - weight2)
    float gw2[3];                     // squared gradient weights
    int w, h;
    uint8_t *out_bgr, *out_lab;       // FROM_HIST: histogram blend BGR / Lab (each nullable)
    float* rhs;                       // GRAD: (3, h, w)
};

// histogram_blend.blend's statistics, per channel: the transfer of a and b to mean 128 / std 256/36, and of their
// blend to the min-error image's mean and std.  The blend's std follows from the exact integer cross moment of a and b.
struct HistCoef {
    double ma, sa, mb, sb, mab, sab, mm, sm;  // a std of 0 (a constant channel) transfers to the target mean
};

__device__ __forceinline__ double transfer(double x, double m, double s, double ts, double tm) {
    return s > 0.0 ? (x - m) * ts / s + tm : tm;
}

__device__ HistCoef hist_coef(const unsigned long long* S, int c, double n, double hw1, double hw2) {
    const double ts = double(float(256.0 / 36.0));
    const unsigned long long* s = S + 7 * c;
    HistCoef k;
    k.ma = double(s[0]) / n;
    k.mb = double(s[2]) / n;
    k.mm = double(s[5]) / n;
    const double va = fmax(double(s[1]) / n - k.ma * k.ma, 0.0), vb = fmax(double(s[3]) / n - k.mb * k.mb, 0.0);
    const double vm = fmax(double(s[6]) / n - k.mm * k.mm, 0.0);
    const double sa = sqrt(va), sb = sqrt(vb);
    k.sa = sa, k.sb = sb, k.sm = sqrt(vm);
    // ab = 2 (w1 A + w2 B) - 256 (w1 + w2) + 256, A and B with std ts and correlation rho = cov(a, b) / (sa sb)
    const double rho = (sa > 0.0 && sb > 0.0) ? (double(s[4]) / n - k.ma * k.mb) / (sa * sb) : 0.0;
    const double a_std = sa > 0.0 ? ts : 0.0, b_std = sb > 0.0 ? ts : 0.0;
    const double vab = 4.0 * (hw1 * hw1 * a_std * a_std + hw2 * hw2 * b_std * b_std + 2.0 * hw1 * hw2 * rho * a_std * b_std);
    k.mab = (128.0 * hw1 + 128.0 * hw2 - 128.0) / 0.5 + 128.0;
    k.sab = sqrt(fmax(vab, 0.0));
    return k;
}

__device__ __forceinline__ float clip100(int v) { return float(v < -100 ? -100 : (v > 100 ? 100 : v)); }

// forward difference of the gradient source image (Ia, or Ib where mask > 0) from pixel q to pixel q + step
__device__ __forceinline__ float grad_at(const RhsArgs& p, size_t q, size_t step, int c) {
    const uint8_t* I = p.mask[q] ? p.lab_b : p.lab_a;
    return clip100(int(I[3 * q + c]) - int(I[3 * (q + step) + c]));
}

template <bool FROM_HIST, bool GRAD>
__global__ __launch_bounds__(256) void blend_rhs(RhsArgs p) {
    __shared__ HistCoef coef[3];
    const int n = p.w * p.h;
    if (FROM_HIST) {
        if (threadIdx.x < 3) coef[threadIdx.x] = hist_coef(p.stats, threadIdx.x, double(n), p.hw1, p.hw2);
        __syncthreads();
    }
    const double ts = double(float(256.0 / 36.0));
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        uint8_t lab[3];
        if (FROM_HIST) {
            uint8_t hb[3], bgr[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const HistCoef& k = coef[c];
                const double A = transfer(double(p.lab_a[3 * q + c]), k.ma, k.sa, ts, 128.0);
                const double B = transfer(double(p.lab_b[3 * q + c]), k.mb, k.sb, ts, 128.0);
                const double ab = (A * p.hw1 + B * p.hw2 - 128.0) / 0.5 + 128.0;
                // histogram_transform reads its input as float32 before the second transfer
                hb[c] = sat_u8(transfer(double(float(ab)), k.mab, k.sab, k.sm, k.mm));
            }
            lab_to_bgr(hb[0], hb[1], hb[2], bgr);
            if (p.out_lab)
                for (int c = 0; c < 3; ++c) p.out_lab[3 * q + c] = hb[c];
            if (p.out_bgr)
                for (int c = 0; c < 3; ++c) p.out_bgr[3 * q + c] = bgr[c];
            if (GRAD) bgr_to_lab(bgr[0], bgr[1], bgr[2], lab);  // poisson_fusion converts the uint8 BGR blend again
        } else {
            bgr_to_lab(p.blend_bgr[3 * q], p.blend_bgr[3 * q + 1], p.blend_bgr[3 * q + 2], lab);
        }
        if (GRAD) {
            const int x = q % p.w, y = q / p.w;
            const size_t W = size_t(p.w);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // (Gx^T gx + Gy^T gy)[q]: gx / gy are zero on the last row / column
                float div = 0.f;
                if (y < p.h - 1) div += grad_at(p, q, W, c);
                if (y > 0) div -= grad_at(p, q - W, W, c);
                if (x < p.w - 1) div += grad_at(p, q, 1, c);
                if (x > 0) div -= grad_at(p, q - 1, 1, c);
                // the constant offset passes through the solve unchanged (eigenvalue 1), so 128 stands in for the mean
                p.rhs[size_t(c) * n + q] = p.gw2[c] * div + (float(lab[c]) - 128.0f);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the exact least-squares solve: orthonormal DCT-II tables and batched fp32 GEMMs
// ---------------------------------------------------------------------------------------------------------------------
struct Tables {
    float *ch, *cht, *cw, *cwt, *lam_h, *lam_w;
};

// C[k][m] = s_k cos(pi (2m + 1) k / 2N) with (2m + 1) k reduced mod 4N in integers first; lam_k = 4 sin^2(pi k / 2N)
__device__ __forceinline__ void dct_entry(int N, int k, int m, float* C, float* CT, float* lam) {
    const long long r = (static_cast<long long>(2 * m + 1) * k) % (4LL * N);
    const double s = k == 0 ? sqrt(1.0 / N) : sqrt(2.0 / N);
    const float v = float(s * cospi(double(r) / (2.0 * N)));
    C[size_t(k) * N + m] = v;
    CT[size_t(m) * N + k] = v;
    if (m == 0) {
        const double sn = sinpi(double(k) / (2.0 * N));
        lam[k] = float(4.0 * sn * sn);
    }
}

__global__ __launch_bounds__(256) void blend_tables(Tables t, int h, int w) {
    const size_t nh = size_t(h) * h, total = nh + size_t(w) * w;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += size_t(gridDim.x) * 256) {
        if (i < nh)
            dct_entry(h, int(i / h), int(i % h), t.ch, t.cht, t.lam_h);
        else
            dct_entry(w, int((i - nh) / w), int((i - nh) % w), t.cw, t.cwt, t.lam_w);
    }
}

enum GemmEpi { kEpiStore = 0, kEpiScale = 1, kEpiLab = 2 };

struct GemmArgs {
    const float *A, *B;  // row-major (M, K) and (K, N); batch strides sA / sB elements (0: shared table)
    float* C;            // kEpiStore / kEpiScale: row-major (M, N), batch stride M N
    uint8_t* lab;        // kEpiLab: (M, N, 3) interleaved, batch = channel
    size_t sA, sB;
    int M, N, K;
    const float *lam_m, *lam_n;  // kEpiScale: divide by 1 + gw2[z] (lam_m[i] + lam_n[j])
    float gw2[3];
};

// 64 x 64 output tile per 256-thread workgroup, 4 x 4 per thread, k-steps of 16 staged in LDS (8.5 KB).  Tiles are
// zero-filled past the matrix edges, so any M, N, K work.  Each output is a k-ordered fmaf chain per k-step and a
// k-ordered fp64 sum of the steps: deterministic.  The fp64 sum is what keeps the solve's error far below kTruncGuard
// at large sides: one fp32 chain over K = 4096 rounds every add at the size of the running sum, which the DC term
// (up to 127 sqrt(K) forward, 127 from the first step on backward) dominates, and on high-contrast frames that error
// passed the guard from 2048^2 up.
template <int EPI>
__global__ __launch_bounds__(256) void blend_gemm(GemmArgs g) {
    __shared__ float As[kGemmK][kGemmTile + 4];  // transposed: As[k][m]
    __shared__ float Bs[kGemmK][kGemmTile];
    const int z = blockIdx.z;
    const float* A = g.A + g.sA * z;
    const float* B = g.B + g.sB * z;
    const int M = g.M, N = g.N, K = g.K;
    const int m0 = blockIdx.y * kGemmTile, n0 = blockIdx.x * kGemmTile;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    const int ar = t >> 2, ac = (t & 3) * 4;   // A tile: row ar, columns ac .. ac + 3
    const int br = t >> 4, bc = (t & 15) * 4;  // B tile: row br, columns bc .. bc + 3
    for (int k0 = 0; k0 < K; k0 += kGemmK) {
        {
            const int gm = m0 + ar;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gk = k0 + ac + u;
                As[ac + u][ar] = (gm < M && gk < K) ? A[size_t(gm) * K + gk] : 0.f;
            }
        }
        {
            const int gk = k0 + br;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gn = n0 + bc + u;
                Bs[br][bc + u] = (gk < K && gn < N) ? B[size_t(gk) * N + gn] : 0.f;
            }
        }
        __syncthreads();
        float part[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[i][j] = 0.f;
#pragma unroll
        for (int k = 0; k < kGemmK; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[k][ty * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[k][tx * 4 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[i][j] = fmaf(a[i], b[j], part[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += double(part[i][j]);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty * 4 + i;
        if (gm >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx * 4 + j;
            if (gn >= N) continue;
            const size_t o = size_t(gm) * N + gn;
            float v = float(acc[i][j]);
            if (EPI == kEpiScale) v = v / (1.0f + g.gw2[z] * (g.lam_m[gm] + g.lam_n[gn]));
            if (EPI == kEpiLab) {
                // poisson_fusion: clip(x + mean, 0, 255).astype(uint8) truncates; kTruncGuard keeps an exactly
                // integer solution (the blend's Lab agrees with the gradients) from truncating on rounding noise
                v = v + (128.0f + kTruncGuard);
                v = v > 0.0f ? (v < 255.0f ? v : 255.0f) : 0.0f;
                g.lab[3 * o + z] = uint8_t(v);
            } else {
                g.C[size_t(M) * N * z + o] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct BlendWs {
    unsigned long long* stats;
    uint8_t *lab_a, *lab_b, *lab_out;
    float *p0, *p1;
    Tables t;
};

size_t blend_ws_bytes(int w, int h, BlendWs* ws, void* base) {
    char* p = static_cast<char*>(base);
    char* const start = p;
    const size_t n = size_t(w) * h;
    BlendWs z;
    z.stats = carve<unsigned long long>(p, 32);
    z.lab_a = carve<uint8_t>(p, 3 * n);
    z.lab_b = carve<uint8_t>(p, 3 * n);
    z.lab_out = carve<uint8_t>(p, 3 * n);
    z.p0 = carve<float>(p, 3 * n);
    z.p1 = carve<float>(p, 3 * n);
    z.t.ch = carve<float>(p, size_t(h) * h);
    z.t.cht = carve<float>(p, size_t(h) * h);
    z.t.cw = carve<float>(p, size_t(w) * w);
    z.t.cwt = carve<float>(p, size_t(w) * w);
    z.t.lam_h = carve<float>(p, h);
    z.t.lam_w = carve<float>(p, w);
    if (ws) *ws = z;
    return size_t(p - start);
}

bool side_ok(int w, int h) { return w >= 2 && h >= 2 && w <= kBlendMaxSide && h <= kBlendMaxSide; }

int pixel_blocks(int n) {
    const int b = (n + 255) / 256, cap = 4 * device_cus();
    return b < cap ? b : cap;
}

struct BlendRun {
    hipStream_t st;
    int err;
    void chk() {
        if (err == FRESCO_OK) err = check_launch();
    }
    void memset0(void* p, size_t bytes) {
        if (err != FRESCO_OK) return;
        const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
        if (e != hipSuccess) {
            set_last_error(e);
            err = FRESCO_ELAUNCH;
        }
    }
    template <int MODE>
    void prep(const PrepArgs& a) {
        if (err != FRESCO_OK) return;
        blend_prep<MODE><<<pixel_blocks(a.w * a.h), 256, 0, st>>>(a);
        chk();
    }
    template <bool FROM_HIST, bool GRAD>
    void rhs(const RhsArgs& a) {
        if (err != FRESCO_OK) return;
        blend_rhs<FROM_HIST, GRAD><<<pixel_blocks(a.w * a.h), 256, 0, st>>>(a);
        chk();
    }
    template <int EPI>
    void gemm(const GemmArgs& g) {
        if (err != FRESCO_OK) return;
        const dim3 grid((g.N + kGemmTile - 1) / kGemmTile, (g.M + kGemmTile - 1) / kGemmTile, 3);
        blend_gemm<EPI><<<grid, 256, 0, st>>>(g);
        chk();
    }
    // rhs planes in z.p0 (3, h, w) -> solution as Lab bytes in z.lab_out
    void solve(const BlendWs& z, int w, int h, const float gw2[3]) {
        if (err != FRESCO_OK) return;
        const size_t total = size_t(h) * h + size_t(w) * w;
        const size_t tb = (total + 255) / 256;
        blend_tables<<<unsigned(tb < 2048 ? tb : 2048), 256, 0, st>>>(z.t, h, w);
        chk();
        const size_t plane = size_t(w) * h;
        GemmArgs g{};
        g.M = h;
        g.N = w;
        for (int c = 0; c < 3; ++c) g.gw2[c] = gw2[c];
        // T1 = C_h R
        g.A = z.t.ch, g.sA = 0, g.B = z.p0, g.sB = plane, g.C = z.p1, g.K = h;
        gemm<kEpiStore>(g);
        // T2 = (T1 C_w^T) / (1 + w^2 (lam_i + mu_j))
        g.A = z.p1, g.sA = plane, g.B = z.t.cwt, g.sB = 0, g.C = z.p0, g.K = w, g.lam_m = z.t.lam_h, g.lam_n = z.t.lam_w;
        gemm<kEpiScale>(g);
        // T3 = T2 C_w
        g.A = z.p0, g.sA = plane, g.B = z.t.cw, g.sB = 0, g.C = z.p1, g.K = w;
        gemm<kEpiStore>(g);
        // x = C_h^T T3, + 128, clipped and truncated to Lab bytes
        g.A = z.t.cht, g.sA = 0, g.B = z.p1, g.sB = plane, g.C = nullptr, g.lab = z.lab_out, g.K = h;
        gemm<kEpiLab>(g);
    }
    void finish(const uint8_t* lab, uint8_t* bgr, uint8_t* lab_copy, int n) {
        if (err != FRESCO_OK) return;
        blend_lab2bgr<<<(n + 255) / 256, 256, 0, st>>>(lab, bgr, n);
        chk();
        if (lab_copy && err == FRESCO_OK) {
            const hipError_t e = hipMemcpyAsync(lab_copy, lab, size_t(3) * n, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) {
                set_last_error(e);
                err = FRESCO_ELAUNCH;
            }
        }
    }
};

bool grad_weights_ok(const float* gw, float gw2[3]) {
    if (!gw) return false;
    for (int c = 0; c < 3; ++c) {
        if (!(std::isfinite(gw[c]))) return false;
        gw2[c] = gw[c] * gw[c];
    }
    return true;
}

}  // namespace
}  // namespace fresco

using namespace fresco;

extern "C" size_t fresco_blend_workspace_bytes(int w, int h) {
    if (!side_ok(w, h)) return 0;
    return blend_ws_bytes(w, h, nullptr, nullptr);
}

extern "C" int fresco_blend_frame(const uint8_t* oa, const uint8_t* ob, const float* d1, const float* d2, int w, int h,
                                  double weight1, const uint8_t* prev_mask, const float* flow, int flags,
                                  const float* grad_weight, uint8_t* out_mask, uint8_t* out_bgr, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (!side_ok(w, h)) return FRESCO_EUNSUPPORTED;
    if (!oa || !ob || !d1 || !d2 || !out_mask || !out_bgr || !workspace) return FRESCO_EINVAL;
    if ((prev_mask == nullptr) != (flow == nullptr) || (prev_mask && prev_mask == out_mask)) return FRESCO_EINVAL;
    if (!(weight1 >= 0.0 && weight1 <= 1.0) || (flags & ~FRESCO_BLEND_GRADIENT)) return FRESCO_EINVAL;
    const bool grad = flags & FRESCO_BLEND_GRADIENT;
    float gw2[3] = {0.f, 0.f, 0.f};
    if (grad && !grad_weights_ok(grad_weight, gw2)) return FRESCO_EINVAL;
    BlendWs z;
    if (workspace_bytes < blend_ws_bytes(w, h, &z, workspace)) return FRESCO_EWORKSPACE;
    const int n = w * h;
    BlendRun R{as_stream(stream), FRESCO_OK};
    R.memset0(z.stats, sizeof(unsigned long long) * kStats);
    PrepArgs pa{};
    pa.a = oa, pa.b = ob, pa.d1 = d1, pa.d2 = d2, pa.prev = prev_mask, pa.flow = flow, pa.weight1 = weight1;
    pa.w = w, pa.h = h, pa.lab_a = z.lab_a, pa.lab_b = z.lab_b, pa.mask = out_mask, pa.stats = z.stats;
    R.prep<kPrepFrame>(pa);
    RhsArgs ra{};
    ra.lab_a = z.lab_a, ra.lab_b = z.lab_b, ra.mask = out_mask, ra.stats = z.stats;
    ra.hw1 = 1.0 - weight1, ra.hw2 = 1.0 - (1.0 - weight1), ra.w = w, ra.h = h, ra.rhs = z.p0;
    for (int c = 0; c < 3; ++c) ra.gw2[c] = gw2[c];
    if (grad) {
        R.rhs<true, true>(ra);
        R.solve(z, w, h, gw2);
        R.finish(z.lab_out, out_bgr, nullptr, n);
    } else {
        ra.out_bgr = out_bgr;
        R.rhs<true, false>(ra);
    }
    return R.err;
}

extern "C" int fresco_bgr_to_lab_u8(const uint8_t* bgr, uint8_t* lab, int n_pixels, void* stream) {
    if (!bgr || !lab || n_pixels < 0) return FRESCO_EINVAL;
    if (n_pixels == 0) return FRESCO_OK;
    blend_bgr2lab<<<(n_pixels + 255) / 256, 256, 0, as_stream(stream)>>>(bgr, lab, n_pixels);
    return check_launch();
}

extern "C" int fresco_lab_to_bgr_u8(const uint8_t* lab, uint8_t* bgr, int n_pixels, void* stream) {
    if (!bgr || !lab || n_pixels < 0) return FRESCO_EINVAL;
    if (n_pixels == 0) return FRESCO_OK;
    blend_lab2bgr<<<(n_pixels + 255) / 256, 256, 0, as_stream(stream)>>>(lab, bgr, n_pixels);
    return check_launch();
}

extern "C" int fresco_histogram_blend(const uint8_t* a, const uint8_t* b, const uint8_t* min_error, int w, int h,
                                      double weight1, double weight2, uint8_t* out_bgr, uint8_t* out_lab,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!side_ok(w, h)) return FRESCO_EUNSUPPORTED;
    if (!a || !b || !min_error || !out_bgr || !workspace) return FRESCO_EINVAL;
    if (!std::isfinite(weight1) || !std::isfinite(weight2)) return FRESCO_EINVAL;
    BlendWs z;
    if (workspace_bytes < blend_ws_bytes(w, h, &z, workspace)) return FRESCO_EWORKSPACE;
    BlendRun R{as_stream(stream), FRESCO_OK};
    R.memset0(z.stats, sizeof(unsigned long long) * kStats);
    PrepArgs pa{};
    pa.a = a, pa.b = b, pa.min_error = min_error, pa.w = w, pa.h = h, pa.lab_a = z.lab_a, pa.lab_b = z.lab_b;
    pa.stats = z.stats;
    R.prep<kPrepHist>(pa);
    RhsArgs ra{};
    ra.lab_a = z.lab_a, ra.lab_b = z.lab_b, ra.stats = z.stats, ra.hw1 = weight1, ra.hw2 = weight2, ra.w = w, ra.h = h;
    ra.out_bgr = out_bgr, ra.out_lab = out_lab;
    R.rhs<true, false>(ra);
    return R.err;
}

extern "C" int fresco_poisson_fusion(const uint8_t* blend_bgr, const uint8_t* i1, const uint8_t* i2,
                                     const uint8_t* mask, int w, int h, const float* grad_weight, uint8_t* out_bgr,
                                     uint8_t* out_lab, void* workspace, size_t workspace_bytes, void* stream) {
    if (!side_ok(w, h)) return FRESCO_EUNSUPPORTED;
    if (!blend_bgr || !i1 || !i2 || !mask || !out_bgr || !workspace) return FRESCO_EINVAL;
    float gw2[3];
    if (!grad_weights_ok(grad_weight, gw2)) return FRESCO_EINVAL;
    BlendWs z;
    if (workspace_bytes < blend_ws_bytes(w, h, &z, workspace)) return FRESCO_EWORKSPACE;
    BlendRun R{as_stream(stream), FRESCO_OK};
    PrepArgs pa{};
    pa.a = i1, pa.b = i2, pa.w = w, pa.h = h, pa.lab_a = z.lab_a, pa.lab_b = z.lab_b;
    R.prep<kPrepLabOnly>(pa);
    RhsArgs ra{};
    ra.lab_a = z.lab_a, ra.lab_b = z.lab_b, ra.mask = mask, ra.blend_bgr = blend_bgr, ra.w = w, ra.h = h;
    ra.rhs = z.p0;
    for (int c = 0; c < 3; ++c) ra.gw2[c] = gw2[c];
    R.rhs<false, true>(ra);
    R.solve(z, w, h, gw2);
    R.finish(z.lab_out, out_bgr, out_lab, w * h);
    return R.err;
}
