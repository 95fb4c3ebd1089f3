// resize_image where it enlarges (reference: src/utils.py resize_image -> cv2.resize with INTER_LANCZOS4 for k > 1, and
// INTER_AREA's two-tap rule when the rounding to multiples of 64 enlarges a side), batched over uint8 RGB frames
// (n, H, W, 3).  Integer arithmetic on the device; DESIGN.md section 15 has the rules, include/fresco_resize.h declares the
// entry points (frame_resize_*, beside the pinned fresco_* and keyframe_* surfaces).  keyframe.hip has the shrinking case.
//
//   frame_resize_kernel<8>  LANCZOS4:    eight taps per axis, (v + 2^21) >> 22
//   frame_resize_kernel<2>  LINEAR_AREA: two taps per axis, OpenCV's two-stage shifts
//
// One workgroup per 32 x 32 output tile.  With ssize <= 2 dsize on both axes the taps of a tile lie in a window of at most
// 72 x 72 source pixels (31 steps of at most 2, one more for the float rounding of the sample position, eight taps).  The
// window goes to LDS as bytes at coordinates clamped to the frame (the replicated border), the horizontal pass runs once
// per window row into 32-bit LDS words, the vertical pass reads those: 8 + 8 multiply-adds per value at most, not 64.
// Only the rows and columns the tile's taps reach are staged.  The grid is the tile count (at most 2^23, more are
// refused): no cap, no stride.
//
// frame_resize_table writes a geometry's tap table to the caller's host memory (no HIP call); the caller uploads it once.
// The kernel trusts none of it: first-tap indices are clamped to the axis, their offsets to the window, table reads to the
// arrays whose size the launcher checked; sums that a wrong table could overflow are formed in unsigned words.
// Built with -ffp-contract=off: the float / double steps of the coefficient rules round where OpenCV's do.
#include <float.h>
#include <math.h>

#include "../../include/fresco_resize.h"
#include "common.h"

namespace fresco {

constexpr int RS_T = 32;                    // tile side, output pixels
constexpr int RS_WIN = 2 * RS_T + 8;        // window side, source pixels
constexpr int RS_ROWB = RS_T * 3;           // values of a tile row, channels interleaved as they lie in memory
constexpr int RS_WINB = RS_WIN * 3;         // bytes of a window row
constexpr int RS_SLACK = 16;                // first-tap indices are clamped to [-RS_SLACK, ssize + RS_SLACK]
constexpr int RS_MAX_SIDE = 1 << 24;
constexpr int64_t RS_MAX_BYTES = (int64_t)1 << 40;
constexpr int64_t RS_MAX_TILES = (int64_t)1 << 23;  // one workgroup each: grid x 256 threads stays below 2^32

// One axis of the tap table: output index d reads source indices first[d] .. first[d] + K - 1 (replicated at the borders)
// with the 11-bit fixed-point weights coef[d K] .. coef[d K + K - 1]
struct RsAxis {
    const int* first;
    const int16_t* coef;
    int ssize, dsize;
};

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int rs_first(const RsAxis& ax, int d) {
    return rs_clamp(ax.first[rs_clamp(d, 0, ax.dsize - 1)], -RS_SLACK, ax.ssize + RS_SLACK);
}

template <int K>
__global__ __launch_bounds__(256) void frame_resize_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           RsAxis xt, RsAxis yt, int tx, int ty) {
    __shared__ uint8_t px[RS_WIN * RS_WINB];
    __shared__ int32_t hz[RS_WIN * RS_ROWB];
    __shared__ int16_t xc[RS_T * K], yc[RS_T * K];
    __shared__ int xrel[RS_T], yrel[RS_T];
    const int t = threadIdx.x;
    const int H0 = yt.ssize, W0 = xt.ssize, H = yt.dsize, W = xt.dsize;
    const int per_frame = tx * ty;
    const int f = (int)(blockIdx.x / (uint32_t)per_frame), r = (int)(blockIdx.x - (uint32_t)f * per_frame);
    const int oy0 = (r / tx) * RS_T, ox0 = (r % tx) * RS_T;
    // the window: from the first tap of the tile's first index to the last tap of its last one
    const int x0 = rs_first(xt, ox0), y0 = rs_first(yt, oy0);
    const int nx = rs_clamp(rs_first(xt, ox0 + RS_T - 1) + K - x0, K, RS_WIN);
    const int ny = rs_clamp(rs_first(yt, oy0 + RS_T - 1) + K - y0, K, RS_WIN);
    if (t < 2 * RS_T) {  // the tile's slice of the table; indices past the frame's edge repeat the last one
        const bool is_y = t >= RS_T;
        const int l = t & (RS_T - 1);
        const RsAxis& ax = is_y ? yt : xt;
        const int d = rs_clamp((is_y ? oy0 : ox0) + l, 0, ax.dsize - 1);
        (is_y ? yrel : xrel)[l] = rs_clamp(rs_first(ax, d) - (is_y ? y0 : x0), 0, (is_y ? ny : nx) - K);
        int16_t* c = (is_y ? yc : xc) + l * K;
#pragma unroll
        for (int k = 0; k < K; ++k) c[k] = ax.coef[(int64_t)d * K + k];
    }
    // bytes, so any alignment of src; a thread keeps its byte column and walks every other row
    const uint8_t* fsrc = src + (int64_t)f * H0 * W0 * 3;
    for (int b = t & 127; b < nx * 3; b += 128) {
        const int j = b / 3, c = b - 3 * j;
        const int64_t col = (int64_t)rs_clamp(x0 + j, 0, W0 - 1) * 3 + c;
        for (int row = t >> 7; row < ny; row += 2)
            px[row * RS_WINB + b] = fsrc[(int64_t)rs_clamp(y0 + row, 0, H0 - 1) * W0 * 3 + col];
    }
    __syncthreads();
    for (int i = t; i < ny * RS_ROWB; i += 256) {
        const int row = i / RS_ROWB, cb = i - row * RS_ROWB;
        const int col = cb / 3, c = cb - col * 3;
        const uint8_t* l = px + row * RS_WINB + xrel[col] * 3 + c;
        int32_t h = 0;  // |h| <= 255 * 8 * 2^15 whatever the table holds
#pragma unroll
        for (int k = 0; k < K; ++k) h += (int32_t)xc[col * K + k] * (int32_t)l[3 * k];
        hz[i] = h;
    }
    __syncthreads();
    uint8_t* fdst = dst + (((int64_t)f * H + oy0) * W + ox0) * 3;
    for (int i = t; i < RS_T * RS_ROWB; i += 256) {
        const int ly = i / RS_ROWB, cb = i - ly * RS_ROWB;
        if (oy0 + ly >= H || ox0 + cb / 3 >= W) continue;
        const int32_t* hp = hz + yrel[ly] * RS_ROWB + cb;
        const int16_t* b = yc + ly * K;
        int32_t out;
        if (K == 8) {
            // the right table keeps |v| + 2^21 below 2^31; unsigned words so that a wrong one wraps
            uint32_t v = 1u << 21;
#pragma unroll
            for (int k = 0; k < K; ++k) v += (uint32_t)(int32_t)b[k] * (uint32_t)hp[k * RS_ROWB];
            out = (int32_t)v >> 22;
        } else {
            const int32_t v0 = (int32_t)((uint32_t)(int32_t)b[0] * (uint32_t)(hp[0] >> 4)) >> 16;
            const int32_t v1 = (int32_t)((uint32_t)(int32_t)b[1] * (uint32_t)(hp[RS_ROWB] >> 4)) >> 16;
            out = (v0 + v1 + 2) >> 2;
        }
        fdst[(int64_t)ly * W * 3 + cb] = (uint8_t)rs_clamp(out, 0, 255);
    }
}

// ---- the tap tables, built on the host into the caller's memory
static inline int rs_taps(int method) {
    return method == FRAME_RESIZE_LANCZOS4 ? 8 : (method == FRAME_RESIZE_LINEAR_AREA ? 2 : 0);
}

// the table blob: x.first[W] (int32) | x.coef[W K] (int16) | y.first[H] | y.coef[H K]; K is even, so every part starts on
// a 32-bit word -- a function of the geometry and the method alone
struct RsLayout {
    size_t xfirst, xcoef, yfirst, ycoef, bytes;
};

static inline RsLayout rs_layout(int H, int W, int K) {
    RsLayout l;
    l.xfirst = 0;
    l.xcoef = l.xfirst + (size_t)W * 4;
    l.yfirst = l.xcoef + (size_t)W * K * 2;
    l.ycoef = l.yfirst + (size_t)H * 4;
    l.bytes = l.ycoef + (size_t)H * K * 2;
    return l;
}

static inline int16_t rs_fixed(float c) { return (int16_t)rintf(c * 2048.f); }  // round half to even, as cvRound

// interpolateLanczos4: x + 3 - i in float, the angles and the quotient in double, the sum and the normalisation in float
static void rs_lanczos_coeffs(float x, float* c) {
    static const double r = 0.70710678118654752440;
    static const double cs[8][2] = {{1, 0}, {-r, -r}, {0, 1}, {r, -r}, {-1, 0}, {r, r}, {0, -1}, {-r, r}};
    static const double pi = 3.1415926535897932384626433832795;
    if (x < FLT_EPSILON) {
        for (int i = 0; i < 8; ++i) c[i] = 0.f;
        c[3] = 1.f;
        return;
    }
    const double y0 = -(x + 3) * pi * 0.25, s0 = sin(y0), c0 = cos(y0);
    float sum = 0.f;
    for (int i = 0; i < 8; ++i) {
        const double y = -(x + 3 - i) * pi * 0.25;
        c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        sum += c[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; ++i) c[i] *= sum;
}

static void rs_lanczos_axis(int ssize, int dsize, int* first, int16_t* coef) {
    const double scale = 1. / ((double)dsize / ssize);
    for (int d = 0; d < dsize; ++d) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        const int s = (int)floorf(fx);
        fx -= (float)s;
        float c[8];
        rs_lanczos_coeffs(fx, c);
        first[d] = s - 3;
        for (int i = 0; i < 8; ++i) coef[(size_t)d * 8 + i] = rs_fixed(c[i]);
    }
}

static void rs_linear_area_axis(int ssize, int dsize, int* first, int16_t* coef) {
    const double inv = (double)dsize / ssize, scale = 1. / inv;
    for (int d = 0; d < dsize; ++d) {
        int s = (int)floor(d * scale);
        float fx = (float)((d + 1) - (s + 1) * inv);
        fx = fx <= 0 ? 0.f : fx - floorf(fx);
        if (s < 0) {
            s = 0;
            fx = 0.f;
        }
        if (s + 1 >= ssize) {
            s = ssize - 1;
            fx = 0.f;
        }
        first[d] = s;
        coef[(size_t)d * 2] = rs_fixed(1.f - fx);
        coef[(size_t)d * 2 + 1] = rs_fixed(fx);
    }
}

// FRESCO_OK when the resize takes the geometry
static inline int rs_geometry(int H0, int W0, int H, int W, int method) {
    if (H0 <= 0 || W0 <= 0 || H <= 0 || W <= 0 || !rs_taps(method)) return FRESCO_EINVAL;
    if (H0 > RS_MAX_SIDE || W0 > RS_MAX_SIDE || H > RS_MAX_SIDE || W > RS_MAX_SIDE) return FRESCO_EUNSUPPORTED;
    if (H0 > 2 * H || W0 > 2 * W) return FRESCO_EUNSUPPORTED;  // the window of a tile would not fit
    return FRESCO_OK;
}

}  // namespace fresco

using namespace fresco;

extern "C" size_t frame_resize_table_bytes(int H0, int W0, int H, int W, int method) {
    if (rs_geometry(H0, W0, H, W, method) != FRESCO_OK) return 0;
    return rs_layout(H, W, rs_taps(method)).bytes;
}

extern "C" int frame_resize_table(int H0, int W0, int H, int W, int method, void* host_table, size_t table_bytes) {
    const int rc = rs_geometry(H0, W0, H, W, method);
    if (rc != FRESCO_OK) return rc;
    if (!host_table || !aligned_to(host_table, 4)) return FRESCO_EINVAL;
    const RsLayout l = rs_layout(H, W, rs_taps(method));
    if (table_bytes < l.bytes) return FRESCO_EWORKSPACE;
    char* p = static_cast<char*>(host_table);
    int* xf = reinterpret_cast<int*>(p + l.xfirst);
    int* yf = reinterpret_cast<int*>(p + l.yfirst);
    int16_t* xc = reinterpret_cast<int16_t*>(p + l.xcoef);
    int16_t* yc = reinterpret_cast<int16_t*>(p + l.ycoef);
    if (method == FRAME_RESIZE_LANCZOS4) {
        rs_lanczos_axis(W0, W, xf, xc);
        rs_lanczos_axis(H0, H, yf, yc);
    } else {
        rs_linear_area_axis(W0, W, xf, xc);
        rs_linear_area_axis(H0, H, yf, yc);
    }
    return FRESCO_OK;
}

extern "C" int frame_resize_u8(const uint8_t* src, uint8_t* dst, const void* table, size_t table_bytes, int n, int H0, int W0,
                               int H, int W, int method, void* stream) {
    if (!src || !dst || !table || !aligned_to(table, 4) || n <= 0) return FRESCO_EINVAL;
    const int rc = rs_geometry(H0, W0, H, W, method);
    if (rc != FRESCO_OK) return rc;
    const int64_t hw0 = (int64_t)H0 * W0;  // < 2^48
    if (hw0 >= RS_MAX_BYTES / 3 || n > (RS_MAX_BYTES - 1) / (hw0 * 3)) return FRESCO_EUNSUPPORTED;
    const int64_t hw = (int64_t)H * W;     // < 2^48
    if (hw >= (int64_t)1 << 31 || (int64_t)n * hw >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    const int K = rs_taps(method);
    const RsLayout l = rs_layout(H, W, K);
    if (table_bytes < l.bytes) return FRESCO_EWORKSPACE;
    const char* p = static_cast<const char*>(table);
    const RsAxis xt = {reinterpret_cast<const int*>(p + l.xfirst), reinterpret_cast<const int16_t*>(p + l.xcoef), W0, W};
    const RsAxis yt = {reinterpret_cast<const int*>(p + l.yfirst), reinterpret_cast<const int16_t*>(p + l.ycoef), H0, H};
    const int tx = (W + RS_T - 1) / RS_T, ty = (H + RS_T - 1) / RS_T;
    const int64_t tiles = (int64_t)n * tx * ty;  // <= n H W < 2^31
    if (tiles > RS_MAX_TILES) return FRESCO_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    if (K == 8)
        hipLaunchKernelGGL(frame_resize_kernel<8>, dim3((uint32_t)tiles), dim3(256), 0, st, src, dst, xt, yt, tx, ty);
    else
        hipLaunchKernelGGL(frame_resize_kernel<2>, dim3((uint32_t)tiles), dim3(256), 0, st, src, dst, xt, yt, tx, ty);
    return check_launch();
}
