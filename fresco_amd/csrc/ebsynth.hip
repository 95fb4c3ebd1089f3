// Ebsynth: guided patch-based synthesis (PatchMatch search + patch voting over an image pyramid), the second stage of
// FRESCO's video_blend.py (src/ebsynth/deps/ebsynth, ebsynthRun) -- written for gfx950 from the algorithm's
// description; see DESIGN.md section 9 for the semantics kept and the two deliberate departures (counter-based random
// numbers, Omega read from a per-pass snapshot so a run is bit-reproducible).
//
// Data layout: every pixel is one record of RW x 16 bytes, channels in the order [style (ns) | guide (ng) | zero pad]:
//   source record  = source style | source guide
//   target record  = current target style | target guide        (double-buffered: the vote writes the other copy)
//   modulation rec = unused | target modulation                 (only with a modulation image)
// so one patch tap is RW 16-byte loads from each side.  Weights are per record byte (0 on the padding).
//
// Batches (fresco_ebsynth_run_batch): n problems of one shape run through one launch sequence; the problem index is
// blockIdx.z.  Every buffer is problem-major and dense at the current level's size (problem b of a level's target
// records starts at b * tw * th * RW), so one memset or snapshot copy covers the whole batch.  The random bits hash the
// problem's own seed, never its batch position: fresco_ebsynth_run is the n = 1 case.
#include <cfloat>
#include <cmath>
#include <utility>

#include "common.h"

namespace fresco {
namespace {

constexpr int kEbBlock = 16;  // 16 x 16 pixel tiles: four wave64s, each 16 x 4 pixels
constexpr int kEbMaxStyle = 8, kEbMaxGuide = 24;
constexpr int kEbMaxBatch = FRESCO_EBSYNTH_MAX_BATCH;  // the per-problem seeds travel in the random kernels' arguments

struct EbSeeds {
    uint64_t s[kEbMaxBatch];
};

struct EbWeights {
    float w[32];  // per record byte
};

// What the per-pixel kernels of one pass need: the level's images and sizes, the patch and the uniformity weight.
// The record pointers are problem 0's; problem b's are b * tstride / sstride records further.
struct EbLevel {
    const uint4* trec;  // target records, tw x th
    const uint4* srec;  // source records, sw x sh
    const uint4* mrec;  // modulation records (MOD only)
    size_t tstride, sstride;  // records per problem: tw * th * RW, sw * sh * RW
    int tw, th, sw, sh, ns, patch;
    float lambda, omega_best;
    EbWeights W;
};

// one problem's records of a level
struct EbRecs {
    const uint4 *t, *s, *m;
};

__device__ __forceinline__ size_t prob() { return blockIdx.z; }

__device__ __forceinline__ EbRecs recs_of(const EbLevel& L) {
    const size_t b = prob();
    return EbRecs{L.trec + b * L.tstride, L.srec + b * L.sstride, L.mrec ? L.mrec + b * L.tstride : nullptr};
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint32_t word(const uint4& v, int k) {
    return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w));
}
__device__ __forceinline__ float byte_f(const uint4& v, int j) {
    return float((word(v, j >> 2) >> (8 * (j & 3))) & 0xffu);
}

// Weighted SSD of the target patch at (tx, ty) against the source patch at (sx, sy), rows top to bottom; returns as
// soon as a completed row leaves the sum above `bound`.  Target taps are clamped to the image; source centres are
// always at least patch/2 from the border.
template <int RW, bool MOD>
__device__ float patch_error(const EbLevel& L, const EbRecs& P, int r, int tx, int ty, int sx, int sy, float bound) {
    float err = 0.f;
    for (int py = -r; py <= r; ++py) {
        const int trow = clampi(ty + py, 0, L.th - 1) * L.tw;
        const int srow = (sy + py) * L.sw;
        for (int px = -r; px <= r; ++px) {
            const int ti = trow + clampi(tx + px, 0, L.tw - 1);
            const int si = srow + sx + px;
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                const uint4 a = P.t[ti * RW + k];
                const uint4 b = P.s[si * RW + k];
                uint4 m = {0, 0, 0, 0};
                if (MOD) m = P.m[ti * RW + k];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = k * 16 + j;
                    const float d = byte_f(a, j) - byte_f(b, j);
                    float w = L.W.w[c];
                    if (MOD && c >= L.ns) w = w * (byte_f(m, j) / 255.0f);
                    err += w * d * d;
                }
            }
        }
        if (err > bound) return err;
    }
    return err;
}

__device__ __forceinline__ int omega_sum(const int* om, int sw, int r, int bx, int by) {
    int s = 0;
    for (int oy = -r; oy <= r; ++oy)
        for (int ox = -r; ox <= r; ++ox) s += om[(by + oy) * sw + bx + ox];
    return s;
}

__device__ __forceinline__ void omega_add(int* om, int sw, int r, int bx, int by, int d) {
    for (int oy = -r; oy <= r; ++oy)
        for (int ox = -r; ox <= r; ++ox) atomicAdd(&om[(by + oy) * sw + bx + ox], d);
}

__device__ __forceinline__ int patch_overlap(int p, int2 a, int2 b) {
    return max(0, p - abs(a.x - b.x)) * max(0, p - abs(a.y - b.y));
}

// Occupancy of the source patch at c as this pixel sees Omega during a pass: the pass-start snapshot, with the pixel's
// own patch moved from its snapshot-time centre n0 to its current best nb (other pixels' moves land in the live copy
// and show from the next pass on).  Normalised by the patch area and omega_best; 0 without a uniformity term.
__device__ __forceinline__ float occupancy(const EbLevel& L, const int* osnap, int2 c, int2 n0, int2 nb) {
    if (L.lambda == 0.f) return 0.f;
    const int s = omega_sum(osnap, L.sw, L.patch / 2, c.x, c.y) - patch_overlap(L.patch, c, n0) +
                  patch_overlap(L.patch, c, nb);
    return (float(s) / float(L.patch * L.patch)) / L.omega_best;
}

// One candidate: accepted iff err + lambda * occupancy drops (occupancies per `occupancy`; cur_occ is that of the
// current best).  Accepted moves go to the live Omega with integer atomics (order-independent).  The decision is not
// contracted, so given err it is the IEEE one the tests restate.  patch_error may be contracted (FMAs): its sum equals
// the tests' exact one only while every weighted product and partial sum is an exact fp32 integer, which
// tests/test_gpu_ebsynth_matrix.py checks on its inputs (integer weights, patch^2 * sum_c w_c * range_c^2 < 2^24).
template <int RW, bool MOD>
__device__ __forceinline__ void try_patch(const EbLevel& L, const EbRecs& P, const int* osnap, int* olive, int ax,
                                          int ay, int2 c, int2 n0, int2& nbest, float& ebest, float& cur_occ) {
#pragma clang fp contract(off)
    const int r = L.patch / 2;
    const float new_occ = occupancy(L, osnap, c, n0, nbest);
    const float cur = ebest + L.lambda * cur_occ;
    const float e = patch_error<RW, MOD>(L, P, r, ax, ay, c.x, c.y, cur);
    if (e + L.lambda * new_occ < cur) {
        if (L.lambda != 0.f) {
            omega_add(olive, L.sw, r, c.x, c.y, +1);
            omega_add(olive, L.sw, r, nbest.x, nbest.y, -1);
        }
        nbest = c;
        ebest = e;
        cur_occ = occupancy(L, osnap, c, n0, c);
    }
}

// counter-based random bits: splitmix64 finaliser over (seed, pixel, pass, radius step)
__device__ __forceinline__ uint64_t eb_hash(uint64_t seed, uint32_t pixel, uint32_t pass, uint32_t step) {
    uint64_t z = seed ^ (0x9E3779B97F4A7C15ull * (uint64_t(pixel) + 1));
    z += (uint64_t(pass) << 32 | step) * 0xD6E8FEB86659FD93ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint32_t kInitPass = 0xffffffffu;  // pass id of the random initial NNF

#define EB_XY                                              \
    const int x = blockIdx.x * kEbBlock + threadIdx.x;     \
    const int y = blockIdx.y * kEbBlock + threadIdx.y;

// ---------------------------------------------------------------------------------------------------------------------
// kernels

// record[i] = a[i][0..na) (zeros if a is null) | b[i][0..nb) | zero pad
template <int RW>
__global__ __launch_bounds__(256) void eb_pack(const uint8_t* __restrict__ a, int na, const uint8_t* __restrict__ b,
                                               int nb, uint4* __restrict__ out, size_t n) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t w[RW * 4];
#pragma unroll
    for (int k = 0; k < RW * 4; ++k) w[k] = 0;
#pragma unroll
    for (int c = 0; c < RW * 16; ++c) {
        uint32_t v = 0;
        if (c < na) v = a ? a[(size_t)i * na + c] : 0u;
        else if (c < na + nb) v = b[(size_t)i * nb + (c - na)];
        w[c >> 2] |= v << (8 * (c & 3));
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) out[i * RW + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// Bilinear resample of whole records (every byte channel alike), sample point s * (x, y) with s = iw / ow for both axes,
// taps clamped to the image, result truncated to a byte.
template <int RW>
__global__ __launch_bounds__(256) void eb_resample(const uint4* __restrict__ in, int iw, int ih,
                                                   uint4* __restrict__ out, int ow, int oh) {
#pragma clang fp contract(off)
    EB_XY
    if (x >= ow || y >= oh) return;
    in += prob() * iw * ih * RW;
    out += prob() * ow * oh * RW;
    const float sc = float(iw) / float(ow);
    const float fx = sc * float(x), fy = sc * float(y);
    const int ix = int(fx), iy = int(fy);
    const float s = fx - float(ix), t = fy - float(iy);
    const int x0 = clampi(ix, 0, iw - 1), x1 = clampi(ix + 1, 0, iw - 1);
    const int y0 = clampi(iy, 0, ih - 1), y1 = clampi(iy + 1, 0, ih - 1);
    const float w00 = (1.0f - s) * (1.0f - t), w10 = s * (1.0f - t), w01 = (1.0f - s) * t, w11 = s * t;
#pragma unroll
    for (int k = 0; k < RW; ++k) {
        const uint4 a = in[(y0 * iw + x0) * RW + k], b = in[(y0 * iw + x1) * RW + k];
        const uint4 c = in[(y1 * iw + x0) * RW + k], d = in[(y1 * iw + x1) * RW + k];
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float v = w00 * byte_f(a, j) + w10 * byte_f(b, j) + w01 * byte_f(c, j) + w11 * byte_f(d, j);
            w[j >> 2] |= (uint32_t(v) & 0xffu) << (8 * (j & 3));
        }
        out[(y * ow + x) * RW + k] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// random NNF of the coarsest level: centres uniform in [r, size - r)
__global__ __launch_bounds__(256) void eb_nnf_random(int2* __restrict__ nnf, int tw, int th, int sw, int sh, int r,
                                                     EbSeeds seeds) {
    EB_XY
    if (x >= tw || y >= th) return;
    nnf += prob() * tw * th;
    const uint64_t h = eb_hash(seeds.s[blockIdx.z], uint32_t(y * tw + x), kInitPass, 0);
    nnf[y * tw + x] = make_int2(r + int(uint32_t(h) % uint32_t(sw - 2 * r)),
                                r + int(uint32_t(h >> 32) % uint32_t(sh - 2 * r)));
}

// x2 upscale of the previous level's NNF plus the parity offset, clamped to [patch, size - patch - 1]
__global__ __launch_bounds__(256) void eb_nnf_upscale(const int2* __restrict__ prev, int pw, int ph,
                                                      int2* __restrict__ nnf, int tw, int th, int sw, int sh,
                                                      int patch) {
    EB_XY
    if (x >= tw || y >= th) return;
    prev += prob() * pw * ph;
    nnf += prob() * tw * th;
    const int2 p = prev[clampi(y / 2, 0, ph - 1) * pw + clampi(x / 2, 0, pw - 1)];
    nnf[y * tw + x] = make_int2(clampi(p.x * 2 + (x & 1), patch, sw - patch - 1),
                                clampi(p.y * 2 + (y & 1), patch, sh - patch - 1));
}

// Omega: how many target patches cover each source pixel
__global__ __launch_bounds__(256) void eb_omega_build(const int2* __restrict__ nnf, int tw, int th,
                                                      int* __restrict__ omega, int sw, int sh, int r) {
    EB_XY
    if (x >= tw || y >= th) return;
    nnf += prob() * tw * th;
    omega += prob() * sw * sh;
    const int2 n = nnf[y * tw + x];
    omega_add(omega, sw, r, n.x, n.y, +1);
}

// Vote: the new target style at (x, y) is the (1/(1+E)-weighted) mean of the source style under every patch that
// covers (x, y); the guide bytes of the record are carried over.
template <int RW, bool WEIGHTED>
__global__ __launch_bounds__(256) void eb_vote(const uint4* __restrict__ srec, int sw, const int2* __restrict__ nnf,
                                               const float* __restrict__ E, const uint4* __restrict__ told,
                                               uint4* __restrict__ tnew, int tw, int th, int sh, int ns,
                                               int patch) {
#pragma clang fp contract(off)
    EB_XY
    if (x >= tw || y >= th) return;
    const size_t b = prob(), T = size_t(tw) * th;
    srec += b * sw * sh * RW;
    nnf += b * T;
    if (WEIGHTED) E += b * T;
    told += b * T * RW;
    tnew += b * T * RW;
    const int r = patch / 2;
    float sum[kEbMaxStyle];
#pragma unroll
    for (int c = 0; c < kEbMaxStyle; ++c) sum[c] = 0.f;
    float wsum = 0.f;
    for (int py = -r; py <= r; ++py) {
        const int yy = clampi(y + py, 0, th - 1);
        for (int px = -r; px <= r; ++px) {
            const int xx = clampi(x + px, 0, tw - 1);
            const int2 n = nnf[yy * tw + xx];
            float w = 1.0f;
            if (WEIGHTED) w = 1.0f / (1.0f + E[yy * tw + xx] / float(patch * patch * ns));
            const uint4 s = srec[((n.y - py) * sw + (n.x - px)) * RW];  // style bytes are in the first 16
#pragma unroll
            for (int c = 0; c < kEbMaxStyle; ++c) sum[c] += w * byte_f(s, c);
            wsum += w;
        }
    }
    uint4 o0 = told[(y * tw + x) * RW];
    uint32_t lo[2] = {o0.x, o0.y};
#pragma unroll
    for (int c = 0; c < kEbMaxStyle; ++c) {
        if (c < ns) {
            const uint32_t v = uint32_t(sum[c] / wsum) & 0xffu;
            lo[c >> 2] = (lo[c >> 2] & ~(0xffu << (8 * (c & 3)))) | (v << (8 * (c & 3)));
        }
    }
    o0.x = lo[0];
    o0.y = lo[1];
    tnew[(y * tw + x) * RW] = o0;
    if (RW > 1) tnew[(y * tw + x) * RW + 1] = told[(y * tw + x) * RW + 1];
}

// E = patch error of the current NNF, no early exit
template <int RW, bool MOD>
__global__ __launch_bounds__(256) void eb_error_pass(EbLevel L, const int2* __restrict__ nnf, float* __restrict__ E) {
    EB_XY
    if (x >= L.tw || y >= L.th) return;
    const size_t T = size_t(L.tw) * L.th;
    nnf += prob() * T;
    E += prob() * T;
    const int2 n = nnf[y * L.tw + x];
    E[y * L.tw + x] = patch_error<RW, MOD>(L, recs_of(L), L.patch / 2, x, y, n.x, n.y, FLT_MAX);
}

// Propagation at jump radius `jump`: try the four axis neighbours' matches shifted back by the offset.  Reads nnf_in,
// writes nnf_out (every pixel), E in place.
template <int RW, bool MOD>
__global__ __launch_bounds__(256) void eb_propagate(EbLevel L, int jump, const int2* __restrict__ nnf_in,
                                                    int2* __restrict__ nnf_out, float* __restrict__ E,
                                                    const uint8_t* __restrict__ mask, const int* __restrict__ osnap,
                                                    int* __restrict__ olive) {
    EB_XY
    if (x >= L.tw || y >= L.th) return;
    const size_t b = prob(), T = size_t(L.tw) * L.th, S = size_t(L.sw) * L.sh;
    nnf_in += b * T;
    nnf_out += b * T;
    E += b * T;
    mask += b * T;
    osnap += b * S;
    olive += b * S;
    const EbRecs P = recs_of(L);
    const int i = y * L.tw + x;
    int2 nbest = nnf_in[i];
    float ebest = E[i];
    if (mask[i] == 255) {
        const int hp = L.patch / 2;
        const int2 n0 = nbest;
        float cur_occ = occupancy(L, osnap, n0, n0, n0);
        const int offs[4][2] = {{-jump, 0}, {jump, 0}, {0, -jump}, {0, jump}};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ox = offs[k][0], oy = offs[k][1];
            const int2 on = nnf_in[clampi(y + oy, 0, L.th - 1) * L.tw + clampi(x + ox, 0, L.tw - 1)];
            const int nx = on.x - ox, ny = on.y - oy;
            if (nx >= hp && nx < L.sw - hp && ny >= hp && ny < L.sh - hp)
                try_patch<RW, MOD>(L, P, osnap, olive, x, y, make_int2(nx, ny), n0, nbest, ebest, cur_occ);
        }
    }
    E[i] = ebest;
    nnf_out[i] = nbest;
}

// Random search, every radius r = 1, 2, 4, ... < max(sw, sh) / 2 in one launch: one uniform candidate in the window of
// radius r around the current best (clamped to valid centres) per radius.  NNF and E in place.
template <int RW, bool MOD>
__global__ __launch_bounds__(256) void eb_random_search(EbLevel L, int2* __restrict__ nnf, float* __restrict__ E,
                                                        const uint8_t* __restrict__ mask,
                                                        const int* __restrict__ osnap, int* __restrict__ olive,
                                                        EbSeeds seeds, uint32_t pass, int r_first, int r_end) {
    EB_XY
    if (x >= L.tw || y >= L.th) return;
    const size_t b = prob(), T = size_t(L.tw) * L.th, S = size_t(L.sw) * L.sh;
    nnf += b * T;
    E += b * T;
    mask += b * T;
    osnap += b * S;
    olive += b * S;
    const int i = y * L.tw + x;
    if (mask[i] != 255) return;
    const EbRecs P = recs_of(L);
    const uint64_t seed = seeds.s[blockIdx.z];
    const int hp = L.patch / 2;
    int2 nbest = nnf[i];
    float ebest = E[i];
    const int2 n0 = nbest;
    float cur_occ = occupancy(L, osnap, n0, n0, n0);
    uint32_t step = 31 - __builtin_clz(r_first);
    for (int r = r_first; r < r_end; r *= 2, ++step) {
        const int xmin = max(nbest.x - r, hp), xmax = min(nbest.x + r, L.sw - 1 - hp);
        const int ymin = max(nbest.y - r, hp), ymax = min(nbest.y + r, L.sh - 1 - hp);
        const uint64_t h = eb_hash(seed, uint32_t(i), pass, step);
        const int nx = xmin + int(uint32_t(h) % uint32_t(xmax - xmin + 1));
        const int ny = ymin + int(uint32_t(h >> 32) % uint32_t(ymax - ymin + 1));
        try_patch<RW, MOD>(L, P, osnap, olive, x, y, make_int2(nx, ny), n0, nbest, ebest, cur_occ);
    }
    E[i] = ebest;
    nnf[i] = nbest;
}

// stop mask: 255 iff some style channel changed by >= threshold in the last vote
template <int RW>
__global__ __launch_bounds__(256) void eb_mask_eval(const uint4* __restrict__ tnew, const uint4* __restrict__ told,
                                                    uint8_t* __restrict__ mask, int tw, int th, int ns, int thr) {
    EB_XY
    if (x >= tw || y >= th) return;
    const size_t T = size_t(tw) * th;
    tnew += prob() * T * RW;
    told += prob() * T * RW;
    mask += prob() * T;
    const int i = y * tw + x;
    const uint4 a = tnew[i * RW], b = told[i * RW];
    int md = 0;
    for (int c = 0; c < ns; ++c) md = max(md, abs(int(byte_f(a, c)) - int(byte_f(b, c))));
    mask[i] = md < thr ? 0 : 255;
}

// dilation of the stop mask by the patch (taps clamped)
__global__ __launch_bounds__(256) void eb_mask_dilate(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                      int tw, int th, int r) {
    EB_XY
    if (x >= tw || y >= th) return;
    in += prob() * tw * th;
    out += prob() * tw * th;
    uint8_t m = 0;
    for (int py = -r; py <= r; ++py)
        for (int px = -r; px <= r; ++px)
            if (in[clampi(y + py, 0, th - 1) * tw + clampi(x + px, 0, tw - 1)] == 255) m = 255;
    out[y * tw + x] = m;
}

template <int RW>
__global__ __launch_bounds__(256) void eb_unpack_style(const uint4* __restrict__ rec, uint8_t* __restrict__ out,
                                                       size_t n, int ns) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 v = rec[i * RW];
    for (int c = 0; c < ns; ++c) out[i * ns + c] = uint8_t(byte_f(v, c));
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct EbSizes {
    int rw;  // 16-byte words per record
    size_t src_rec, tgt_rec, nnf, e, mask, omega;  // bytes per problem at the finest level
};

EbSizes eb_sizes(int ns, int ng, int sw, int sh, int tw, int th) {
    EbSizes z;
    z.rw = (ns + ng <= 16) ? 1 : 2;
    const size_t S = size_t(sw) * sh, T = size_t(tw) * th;
    z.src_rec = S * z.rw * 16;
    z.tgt_rec = T * z.rw * 16;
    z.nnf = T * sizeof(int2);
    z.e = T * sizeof(float);
    z.mask = T;
    z.omega = S * sizeof(int);
    return z;
}

// every buffer holds n problems back to back
size_t eb_workspace(const EbSizes& z, int with_mod, size_t n) {
    const size_t a = 256;
    size_t b = 2 * align_up(n * z.src_rec, a) + 3 * align_up(n * z.tgt_rec, a) + 2 * align_up(n * z.nnf, a) +
               align_up(n * z.e, a) + 2 * align_up(n * z.mask, a) + 2 * align_up(n * z.omega, a);
    if (with_mod) b += 2 * align_up(n * z.tgt_rec, a);
    return b;
}

// level size: size * 2^-(levels - 1 - level), truncated
inline int level_size(int size, int levels, int level) {
    return int(float(size) * std::ldexp(1.0f, -(levels - 1 - level)));
}

inline dim3 grid3(int w, int h, int n) {
    return dim3((w + kEbBlock - 1) / kEbBlock, (h + kEbBlock - 1) / kEbBlock, n);
}

struct EbRun {
    hipStream_t st;
    int rw;
    bool mod;
    int n;  // problems
    EbSeeds seeds;
    uint32_t pass;  // random-search pass counter
    int launches;
    int err;

    void chk() {
        ++launches;
        if (err == FRESCO_OK) err = check_launch();
    }
    void async(hipError_t e) {
        ++launches;
        if (e != hipSuccess && err == FRESCO_OK) {
            set_last_error(e);
            err = FRESCO_ELAUNCH;
        }
    }
    void snapshot(int* snap, const int* live, size_t bytes) {
        if (err != FRESCO_OK) return;
        async(hipMemcpyAsync(snap, live, bytes, hipMemcpyDeviceToDevice, st));
    }
    dim3 grid(int w, int h) const { return grid3(w, h, n); }

    template <int RW, bool MOD>
    void patchmatch_t(const EbLevel& L, int iters, int2*& nnf, int2*& nnf2, float* E, const uint8_t* mask, int* olive,
                      int* osnap, size_t omega_bytes) {
        const dim3 g = grid(L.tw, L.th), b(kEbBlock, kEbBlock);
        eb_error_pass<RW, MOD><<<g, b, 0, st>>>(L, nnf, E);
        chk();
        const bool occ = L.lambda != 0.f;
        for (int it = 0; it < iters; ++it) {
            for (int jump = 4; jump >= 1; jump /= 2) {
                if (occ) snapshot(osnap, olive, omega_bytes);
                eb_propagate<RW, MOD><<<g, b, 0, st>>>(L, jump, nnf, nnf2, E, mask, osnap, olive);
                chk();
                std::swap(nnf, nnf2);
            }
            if (occ) snapshot(osnap, olive, omega_bytes);
            eb_random_search<RW, MOD><<<g, b, 0, st>>>(L, nnf, E, mask, osnap, olive, seeds, pass++, 1,
                                                        std::max(L.sw, L.sh) / 2);
            chk();
        }
        eb_error_pass<RW, MOD><<<g, b, 0, st>>>(L, nnf, E);
        chk();
    }
    void patchmatch(const EbLevel& L, int iters, int2*& nnf, int2*& nnf2, float* E, const uint8_t* mask, int* olive,
                    int* osnap, size_t omega_bytes) {
        if (rw == 1 && !mod) patchmatch_t<1, false>(L, iters, nnf, nnf2, E, mask, olive, osnap, omega_bytes);
        else if (rw == 1) patchmatch_t<1, true>(L, iters, nnf, nnf2, E, mask, olive, osnap, omega_bytes);
        else if (!mod) patchmatch_t<2, false>(L, iters, nnf, nnf2, E, mask, olive, osnap, omega_bytes);
        else patchmatch_t<2, true>(L, iters, nnf, nnf2, E, mask, olive, osnap, omega_bytes);
    }
    void error_pass(const EbLevel& L, const int2* nnf, float* E) {
        const dim3 g = grid(L.tw, L.th), b(kEbBlock, kEbBlock);
        if (rw == 1 && !mod) eb_error_pass<1, false><<<g, b, 0, st>>>(L, nnf, E);
        else if (rw == 1) eb_error_pass<1, true><<<g, b, 0, st>>>(L, nnf, E);
        else if (!mod) eb_error_pass<2, false><<<g, b, 0, st>>>(L, nnf, E);
        else eb_error_pass<2, true><<<g, b, 0, st>>>(L, nnf, E);
        chk();
    }
    void vote(bool weighted, const uint4* srec, int sw, int sh, const int2* nnf, const float* E, const uint4* told,
              uint4* tnew, int tw, int th, int ns, int patch) {
        const dim3 g = grid(tw, th), b(kEbBlock, kEbBlock);
        if (rw == 1 && !weighted)
            eb_vote<1, false><<<g, b, 0, st>>>(srec, sw, nnf, E, told, tnew, tw, th, sh, ns, patch);
        else if (rw == 1) eb_vote<1, true><<<g, b, 0, st>>>(srec, sw, nnf, E, told, tnew, tw, th, sh, ns, patch);
        else if (!weighted) eb_vote<2, false><<<g, b, 0, st>>>(srec, sw, nnf, E, told, tnew, tw, th, sh, ns, patch);
        else eb_vote<2, true><<<g, b, 0, st>>>(srec, sw, nnf, E, told, tnew, tw, th, sh, ns, patch);
        chk();
    }
    void resample(const uint4* in, int iw, int ih, uint4* out, int ow, int oh) {
        const dim3 g = grid(ow, oh), b(kEbBlock, kEbBlock);
        if (rw == 1) eb_resample<1><<<g, b, 0, st>>>(in, iw, ih, out, ow, oh);
        else eb_resample<2><<<g, b, 0, st>>>(in, iw, ih, out, ow, oh);
        chk();
    }
    // `pixels` per problem; inputs and output are dense over the n problems, so one flat launch covers them
    void pack(const uint8_t* a, int na, const uint8_t* b, int nb, uint4* out, size_t pixels) {
        const size_t total = pixels * n;
        const dim3 g(unsigned((total + 255) / 256));
        if (rw == 1) eb_pack<1><<<g, 256, 0, st>>>(a, na, b, nb, out, total);
        else eb_pack<2><<<g, 256, 0, st>>>(a, na, b, nb, out, total);
        chk();
    }
    void unpack_style(const uint4* rec, uint8_t* out, size_t pixels, int ns) {
        const size_t total = pixels * n;
        const dim3 g(unsigned((total + 255) / 256));
        if (rw == 1) eb_unpack_style<1><<<g, 256, 0, st>>>(rec, out, total, ns);
        else eb_unpack_style<2><<<g, 256, 0, st>>>(rec, out, total, ns);
        chk();
    }
    void mask_eval(const uint4* tnew, const uint4* told, uint8_t* mask, int tw, int th, int ns, int thr) {
        const dim3 g = grid(tw, th), b(kEbBlock, kEbBlock);
        if (rw == 1) eb_mask_eval<1><<<g, b, 0, st>>>(tnew, told, mask, tw, th, ns, thr);
        else eb_mask_eval<2><<<g, b, 0, st>>>(tnew, told, mask, tw, th, ns, thr);
        chk();
    }
};

int validate_common(int ns, int ng, int sw, int sh, int tw, int th, int patch) {
    if (ns < 1 || ng < 1 || sw < 1 || sh < 1 || tw < 1 || th < 1) return FRESCO_EINVAL;
    if (ns > kEbMaxStyle || ng > kEbMaxGuide) return FRESCO_EUNSUPPORTED;
    if (patch < 3 || patch % 2 == 0) return FRESCO_EUNSUPPORTED;
    return FRESCO_OK;
}

// n problems of one shape through one launch sequence (fresco_ebsynth_run is n = 1); `seeds` is a host array of n
int eb_run(int n, const uint8_t* src_style, const uint8_t* src_guide, const uint8_t* tgt_guide,
           const uint8_t* tgt_modulation, const float* style_weights, const float* guide_weights, int n_style,
           int n_guide, int src_w, int src_h, int tgt_w, int tgt_h, float uniformity, int patch, int vote_mode,
           int levels, const int* search_vote_iters, const int* patchmatch_iters, const int* stop_threshold,
           int extra_pass_3x3, const uint64_t* seeds, int32_t* out_nnf, uint8_t* out_style, float* out_error,
           void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 1) return FRESCO_EINVAL;
    if (n > kEbMaxBatch) return FRESCO_EUNSUPPORTED;
    int rc = validate_common(n_style, n_guide, src_w, src_h, tgt_w, tgt_h, patch);
    if (rc != FRESCO_OK) return rc;
    if (!src_style || !src_guide || !tgt_guide || !style_weights || !guide_weights || !search_vote_iters ||
        !patchmatch_iters || !stop_threshold || !seeds || !out_style || !out_error || !workspace)
        return FRESCO_EINVAL;
    if (vote_mode != FRESCO_EBSYNTH_VOTE_PLAIN && vote_mode != FRESCO_EBSYNTH_VOTE_WEIGHTED) return FRESCO_EINVAL;
    if (!(uniformity >= 0.f) || uniformity > FLT_MAX) return FRESCO_EINVAL;
    const int max_levels = fresco_ebsynth_max_levels(src_w, src_h, tgt_w, tgt_h, patch);
    if (max_levels == 0) return FRESCO_EUNSUPPORTED;  // an image side is below 2 * patch + 1
    if (levels == -1) levels = max_levels;
    if (levels < 1) return FRESCO_EINVAL;
    if (levels > max_levels) return FRESCO_EUNSUPPORTED;
    for (int l = 0; l < levels; ++l)
        if (search_vote_iters[l] < 0 || patchmatch_iters[l] < 0 || stop_threshold[l] < 0) return FRESCO_EINVAL;
    const EbSizes z = eb_sizes(n_style, n_guide, src_w, src_h, tgt_w, tgt_h);
    const bool mod = tgt_modulation != nullptr;
    if (workspace_bytes < eb_workspace(z, mod, n)) return FRESCO_EWORKSPACE;

    const size_t N = size_t(n);
    char* p = static_cast<char*>(workspace);
    uint4* src_fine = carve<uint4>(p, N * z.src_rec / 16);
    uint4* src_lvl = carve<uint4>(p, N * z.src_rec / 16);
    uint4* tgt_fine = carve<uint4>(p, N * z.tgt_rec / 16);
    uint4* tgt_a = carve<uint4>(p, N * z.tgt_rec / 16);
    uint4* tgt_b = carve<uint4>(p, N * z.tgt_rec / 16);
    int2* nnf_a = carve<int2>(p, N * z.nnf / sizeof(int2));
    int2* nnf_b = carve<int2>(p, N * z.nnf / sizeof(int2));
    float* E = carve<float>(p, N * z.e / sizeof(float));
    uint8_t* mask = carve<uint8_t>(p, N * z.mask);
    uint8_t* mask2 = carve<uint8_t>(p, N * z.mask);
    int* olive = carve<int>(p, N * z.omega / sizeof(int));
    int* osnap = carve<int>(p, N * z.omega / sizeof(int));
    uint4* mod_fine = mod ? carve<uint4>(p, N * z.tgt_rec / 16) : nullptr;
    uint4* mod_lvl = mod ? carve<uint4>(p, N * z.tgt_rec / 16) : nullptr;

    EbRun R;
    R.st = as_stream(stream);
    R.rw = z.rw;
    R.mod = mod;
    R.n = n;
    for (int b = 0; b < kEbMaxBatch; ++b) R.seeds.s[b] = b < n ? seeds[b] : 0;
    R.pass = 0u;
    R.launches = 0;
    R.err = FRESCO_OK;
    EbWeights W;
    for (int c = 0; c < 32; ++c) W.w[c] = 0.f;
    for (int c = 0; c < n_style; ++c) W.w[c] = style_weights[c];
    for (int c = 0; c < n_guide; ++c) W.w[n_style + c] = guide_weights[c];

    R.pack(src_style, n_style, src_guide, n_guide, src_fine, size_t(src_w) * src_h);
    R.pack(nullptr, n_style, tgt_guide, n_guide, tgt_fine, size_t(tgt_w) * tgt_h);
    if (mod) R.pack(nullptr, n_style, tgt_modulation, n_guide, mod_fine, size_t(tgt_w) * tgt_h);

    const dim3 blk(kEbBlock, kEbBlock);
    int pw = 0, ph = 0;  // previous level's target size
    for (int level = 0; level < levels && R.err == FRESCO_OK; ++level) {
        const bool fine = level == levels - 1;
        const int sw = level_size(src_w, levels, level), sh = level_size(src_h, levels, level);
        const int tw = level_size(tgt_w, levels, level), th = level_size(tgt_h, levels, level);
        const size_t S = size_t(sw) * sh, T = size_t(tw) * th;
        ProfScope prof(FRESCO_PROF_EBSYNTH_LEVEL, level, tw, th, patch, R.st);
        const uint4* srec = src_fine;
        const uint4* mrec = mod_fine;
        if (fine) {
            R.async(hipMemcpyAsync(tgt_a, tgt_fine, N * z.tgt_rec, hipMemcpyDeviceToDevice, R.st));
        } else {
            R.resample(src_fine, src_w, src_h, src_lvl, sw, sh);
            R.resample(tgt_fine, tgt_w, tgt_h, tgt_a, tw, th);
            if (mod) R.resample(mod_fine, tgt_w, tgt_h, mod_lvl, tw, th);
            srec = src_lvl;
            mrec = mod_lvl;
        }
        if (level == 0) {
            eb_nnf_random<<<R.grid(tw, th), blk, 0, R.st>>>(nnf_a, tw, th, sw, sh, patch / 2, R.seeds);
        } else {
            eb_nnf_upscale<<<R.grid(tw, th), blk, 0, R.st>>>(nnf_a, pw, ph, nnf_b, tw, th, sw, sh, patch);
            std::swap(nnf_a, nnf_b);
        }
        R.chk();
        R.async(hipMemsetAsync(E, 0, N * T * sizeof(float), R.st));
        R.async(hipMemsetAsync(olive, 0, N * S * sizeof(int), R.st));
        eb_omega_build<<<R.grid(tw, th), blk, 0, R.st>>>(nnf_a, tw, th, olive, sw, sh, patch / 2);
        R.chk();

        // the level's search/vote loop; at the finest level optionally once more with 3x3 patches and no uniformity
        for (int pass = 0; pass < (fine && extra_pass_3x3 ? 2 : 1) && R.err == FRESCO_OK; ++pass) {
            EbLevel L;
            L.trec = tgt_a;
            L.srec = srec;
            L.mrec = mrec;
            L.tstride = T * z.rw;
            L.sstride = S * z.rw;
            L.tw = tw;
            L.th = th;
            L.sw = sw;
            L.sh = sh;
            L.ns = n_style;
            L.patch = pass == 0 ? patch : 3;
            L.lambda = pass == 0 ? uniformity : 0.f;
            L.omega_best = (float(tw * th) / float(sw * sh)) * float(L.patch * L.patch);
            L.W = W;

            R.vote(false, srec, sw, sh, nnf_a, E, tgt_a, tgt_b, tw, th, n_style, L.patch);
            std::swap(tgt_a, tgt_b);
            R.async(hipMemsetAsync(mask, 255, N * T, R.st));
            for (int v = 0; v < search_vote_iters[level]; ++v) {
                L.trec = tgt_a;
                if (patchmatch_iters[level] > 0)
                    R.patchmatch(L, patchmatch_iters[level], nnf_a, nnf_b, E, mask, olive, osnap,
                                 N * S * sizeof(int));
                else
                    R.error_pass(L, nnf_a, E);
                R.vote(vote_mode == FRESCO_EBSYNTH_VOTE_WEIGHTED, srec, sw, sh, nnf_a, E, tgt_a, tgt_b, tw, th,
                       n_style, L.patch);
                std::swap(tgt_a, tgt_b);
                if (v < search_vote_iters[level] - 1) {
                    R.mask_eval(tgt_a, tgt_b, mask2, tw, th, n_style, stop_threshold[level]);
                    eb_mask_dilate<<<R.grid(tw, th), blk, 0, R.st>>>(mask2, mask, tw, th, L.patch / 2);
                    R.chk();
                }
            }
        }
        pw = tw;
        ph = th;
    }
    if (R.err != FRESCO_OK) return R.err;

    R.unpack_style(tgt_a, out_style, size_t(tgt_w) * tgt_h, n_style);
    if (R.err != FRESCO_OK) return R.err;
    R.async(hipMemcpyAsync(out_error, E, N * z.e, hipMemcpyDeviceToDevice, R.st));
    if (out_nnf) R.async(hipMemcpyAsync(out_nnf, nnf_a, N * z.nnf, hipMemcpyDeviceToDevice, R.st));
    return R.err;
}

}  // namespace
}  // namespace fresco

extern "C" int fresco_ebsynth_max_levels(int src_w, int src_h, int tgt_w, int tgt_h, int patch) {
    if (src_w < 1 || src_h < 1 || tgt_w < 1 || tgt_h < 1 || patch < 1) return 0;
    const int mw = src_w < tgt_w ? src_w : tgt_w, mh = src_h < tgt_h ? src_h : tgt_h;
    for (int level = 32; level >= 0; --level) {
        const float f = std::ldexp(1.0f, -level);
        const int w = int(float(mw) * f), h = int(float(mh) * f);
        if ((w < h ? w : h) >= 2 * patch + 1) return level + 1;
    }
    return 0;
}

extern "C" size_t fresco_ebsynth_workspace_bytes(int n_style, int n_guide, int src_w, int src_h, int tgt_w, int tgt_h,
                                                 int patch, int levels, int with_modulation) {
    return fresco_ebsynth_batch_workspace_bytes(1, n_style, n_guide, src_w, src_h, tgt_w, tgt_h, patch, levels,
                                                with_modulation);
}

extern "C" size_t fresco_ebsynth_batch_workspace_bytes(int n, int n_style, int n_guide, int src_w, int src_h, int tgt_w,
                                                       int tgt_h, int patch, int levels, int with_modulation) {
    using namespace fresco;
    if (n < 1 || n > kEbMaxBatch) return 0;
    if (validate_common(n_style, n_guide, src_w, src_h, tgt_w, tgt_h, patch) != FRESCO_OK) return 0;
    (void)levels;
    return eb_workspace(eb_sizes(n_style, n_guide, src_w, src_h, tgt_w, tgt_h), with_modulation, size_t(n));
}

extern "C" int fresco_ebsynth_run(const uint8_t* src_style, const uint8_t* src_guide, const uint8_t* tgt_guide,
                                  const uint8_t* tgt_modulation, const float* style_weights,
                                  const float* guide_weights, int n_style, int n_guide, int src_w, int src_h,
                                  int tgt_w, int tgt_h, float uniformity, int patch, int vote_mode, int levels,
                                  const int* search_vote_iters, const int* patchmatch_iters,
                                  const int* stop_threshold, int extra_pass_3x3, uint64_t seed, int32_t* out_nnf,
                                  uint8_t* out_style, float* out_error, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return fresco::eb_run(1, src_style, src_guide, tgt_guide, tgt_modulation, style_weights, guide_weights, n_style,
                          n_guide, src_w, src_h, tgt_w, tgt_h, uniformity, patch, vote_mode, levels,
                          search_vote_iters, patchmatch_iters, stop_threshold, extra_pass_3x3, &seed, out_nnf,
                          out_style, out_error, workspace, workspace_bytes, stream);
}

extern "C" int fresco_ebsynth_run_batch(int n, const uint8_t* src_style, const uint8_t* src_guide,
                                        const uint8_t* tgt_guide, const uint8_t* tgt_modulation,
                                        const float* style_weights, const float* guide_weights, int n_style,
                                        int n_guide, int src_w, int src_h, int tgt_w, int tgt_h, float uniformity,
                                        int patch, int vote_mode, int levels, const int* search_vote_iters,
                                        const int* patchmatch_iters, const int* stop_threshold, int extra_pass_3x3,
                                        const uint64_t* seeds, int32_t* out_nnf, uint8_t* out_style,
                                        float* out_error, void* workspace, size_t workspace_bytes, void* stream) {
    return fresco::eb_run(n, src_style, src_guide, tgt_guide, tgt_modulation, style_weights, guide_weights, n_style,
                          n_guide, src_w, src_h, tgt_w, tgt_h, uniformity, patch, vote_mode, levels,
                          search_vote_iters, patchmatch_iters, stop_threshold, extra_pass_3x3, seeds, out_nnf,
                          out_style, out_error, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// single stages, for the tests: the same kernels as fresco_ebsynth_run on channel-interleaved images

extern "C" size_t fresco_ebsynth_stage_workspace_bytes(int w, int h, int ow, int oh) {
    if (w < 1 || h < 1 || ow < 1 || oh < 1) return 0;
    const size_t a = 256;
    return fresco::align_up(size_t(w) * h * 16, a) + fresco::align_up(size_t(ow) * oh * 16, a) +
           fresco::align_up(size_t(w) * h, a);
}

namespace {
fresco::EbRun stage_run(void* stream) {
    fresco::EbRun R;
    R.st = fresco::as_stream(stream);
    R.rw = 1;
    R.mod = false;
    R.n = 1;
    R.seeds.s[0] = 0;
    R.pass = 0u;
    R.launches = 0;
    R.err = FRESCO_OK;
    return R;
}
}  // namespace

extern "C" int fresco_ebsynth_resample(const uint8_t* in, int iw, int ih, int nc, uint8_t* out, int ow, int oh,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    using namespace fresco;
    if (!in || !out || !workspace || iw < 1 || ih < 1 || ow < 1 || oh < 1 || nc < 1) return FRESCO_EINVAL;
    if (nc > 16) return FRESCO_EUNSUPPORTED;
    if (workspace_bytes < fresco_ebsynth_stage_workspace_bytes(iw, ih, ow, oh)) return FRESCO_EWORKSPACE;
    char* p = static_cast<char*>(workspace);
    uint4* a = carve<uint4>(p, size_t(iw) * ih);
    uint4* b = carve<uint4>(p, size_t(ow) * oh);
    EbRun R = stage_run(stream);
    R.pack(in, nc, nullptr, 0, a, size_t(iw) * ih);
    R.resample(a, iw, ih, b, ow, oh);
    R.unpack_style(b, out, size_t(ow) * oh, nc);
    return R.err;
}

extern "C" int fresco_ebsynth_stop_mask(const uint8_t* style_new, const uint8_t* style_old, int w, int h, int ns,
                                        int stop_threshold, int patch, uint8_t* mask, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    using namespace fresco;
    if (!style_new || !style_old || !mask || !workspace || w < 1 || h < 1 || ns < 1) return FRESCO_EINVAL;
    if (ns > kEbMaxStyle || patch < 1 || patch % 2 == 0) return FRESCO_EUNSUPPORTED;
    if (workspace_bytes < fresco_ebsynth_stage_workspace_bytes(w, h, w, h)) return FRESCO_EWORKSPACE;
    char* p = static_cast<char*>(workspace);
    uint4* a = carve<uint4>(p, size_t(w) * h);
    uint4* b = carve<uint4>(p, size_t(w) * h);
    uint8_t* m = carve<uint8_t>(p, size_t(w) * h);
    EbRun R = stage_run(stream);
    R.pack(style_new, ns, nullptr, 0, a, size_t(w) * h);
    R.pack(style_old, ns, nullptr, 0, b, size_t(w) * h);
    R.mask_eval(a, b, m, w, h, ns, stop_threshold);
    eb_mask_dilate<<<grid3(w, h, 1), dim3(kEbBlock, kEbBlock), 0, R.st>>>(m, mask, w, h, patch / 2);
    R.chk();
    return R.err;
}
