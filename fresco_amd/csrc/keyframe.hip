// Key-frame selection's per-frame work (reference: src/keyframe_selection.py get_keyframe_ind -- for every frame of the video
// resize_image -> cv2.GaussianBlur(img, (9, 9), 0) -> numpy2tensor(...).cuda() -> F.mse_loss(prev, cur).cpu()), batched over
// frames on the device.  uint8 RGB frames (n, H, W, 3); integer or fixed-order fp32 arithmetic; DESIGN.md section 15 has the
// rules.  include/fresco_keyframe.h declares the entry points (keyframe_*, beside the pinned fresco_* surface).
//
//   keyframe_resize_box_kernel    INTER_AREA, both scale factors integer: one thread per output pixel sums its box in integers
//   keyframe_resize_table_kernel  INTER_AREA otherwise: one thread per output pixel walks the two coverage tables in order
//   keyframe_blur_diff_kernel     per (pair of consecutive frames, 32 x 32 tile): both tiles + a halo of 4 in LDS, the 9-tap
//                                 fixed-point blur in two passes, (a - b)^2 summed in integers -> one partial per block
//   keyframe_sum_kernel           per pair: the sum of its partials
//
// keyframe_resize_table writes the two coverage tables of a geometry to the caller's host memory (no HIP call); the caller
// uploads them once per geometry and hands the device copy to every resize of it: nothing is allocated in here.
// Both resize kernels read the source through aligned 32-bit words where the buffer's alignment allows (ByteRun).
// Every loop of the blur / sum kernels is bounded by the arguments; the resize kernel's table walks are clamped to them as well.
// Built with -ffp-contract=off: the table path multiplies and adds in OpenCV's order, one rounding each.
#include <math.h>
#include <string.h>

#include "../../include/fresco_keyframe.h"
#include "common.h"

namespace fresco {

constexpr int KF_T = 32;                     // tile side, pixels
constexpr int KF_R = 4;                      // halo: the radius of the 9-tap blur
constexpr int KF_S = KF_T + 2 * KF_R;        // tile + halo
constexpr int KF_ROWB = KF_T * 3;            // bytes of a tile row, channels interleaved as they lie in memory
constexpr int KF_SROWB = KF_S * 3;           // bytes of a tile + halo row
constexpr int KF_MAX_BLOCKS = 1 << 20;       // grid cap: workgroups walk the tiles with a stride
constexpr int KF_MIN_SIDE = KF_R + 1;        // below it reflect-101 would fold twice
constexpr int64_t KF_MAX_BYTES = (int64_t)1 << 40;
constexpr int KF_MAX_SIDE = 1 << 24;         // of a resize source: the table offsets stay ints

// OpenCV's 8.8 fixed-point Gaussian for ksize 9, sigma 0 (-> 1.7): error diffusion from the outside in, the centre takes the
// remainder (sum 256; plain rounding would give 61 in the centre and 257)
__device__ __forceinline__ constexpr uint32_t kf_w(int k) {
    return (k == 0 || k == 8) ? 4u : (k == 1 || k == 7) ? 13u : (k == 2 || k == 6) ? 30u : (k == 3 || k == 5) ? 51u : 60u;
}

// BORDER_REFLECT_101: exact for -n < i < 2n - 1; further out (only positions no output of the frame reads) it is clamped
__device__ __forceinline__ int kf_reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// Consecutive bytes of a buffer of `total` bytes, read as aligned 32-bit words when `wide` (base is then 4-byte aligned); the
// last, partial word of the buffer is put together from its bytes
struct ByteRun {
    const uint8_t* base;
    int64_t total;
    bool wide;
    int64_t widx;
    uint32_t w;
    __device__ __forceinline__ ByteRun(const uint8_t* b, int64_t t, bool wd) : base(b), total(t), wide(wd), widx(-1), w(0) {}
    __device__ __forceinline__ uint32_t get(int64_t b) {
        if (!wide) return base[b];
        const int64_t wi = b >> 2;
        if (wi != widx) {
            widx = wi;
            if (wi * 4 + 4 <= total)
                w = reinterpret_cast<const uint32_t*>(base)[wi];
            else {
                w = 0;
                for (int j = 0; j < 4; ++j)
                    if (wi * 4 + j < total) w |= (uint32_t)base[wi * 4 + j] << (8 * j);
            }
        }
        return (w >> (8 * (int)(b & 3))) & 0xffu;
    }
};

__device__ __forceinline__ uint8_t kf_round_u8(float v) {
    const float r = rintf(v);  // round half to even, as cvRound
    return (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// ix x iy box per output pixel.  2 x 2: (s + 2) >> 2; otherwise float(s) * inv_area (inv_area = 1.f / area), rounded half-even
__global__ __launch_bounds__(256) void keyframe_resize_box_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                  uint32_t pixels, int H, int W, int iy, int ix,
                                                                  float inv_area, int64_t src_bytes, int wide) {
    ByteRun run(src, src_bytes, wide != 0);
    const int W0 = W * ix, H0 = H * iy;
    // (pixels < 2^31: 32-bit divisions)
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < pixels; idx += gridDim.x * 256u) {
        const uint32_t q = idx / (uint32_t)W;
        const int dx = (int)(idx - q * (uint32_t)W), dy = (int)(q % (uint32_t)H);
        const int64_t f = q / (uint32_t)H;
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (int j = 0; j < iy; ++j) {
            int64_t o = ((f * H0 + (int64_t)dy * iy + j) * W0 + (int64_t)dx * ix) * 3;
            for (int k = 0; k < ix; ++k, o += 3) {
                s0 += run.get(o);
                s1 += run.get(o + 1);
                s2 += run.get(o + 2);
            }
        }
        uint8_t* d = dst + (int64_t)idx * 3;
        if (ix == 2 && iy == 2) {
            d[0] = (uint8_t)((s0 + 2) >> 2);
            d[1] = (uint8_t)((s1 + 2) >> 2);
            d[2] = (uint8_t)((s2 + 2) >> 2);
        } else {
            d[0] = kf_round_u8((float)s0 * inv_area);
            d[1] = kf_round_u8((float)s1 * inv_area);
            d[2] = kf_round_u8((float)s2 * inv_area);
        }
    }
}

// One axis of the coverage tables: entries ofs[d] .. ofs[d + 1] - 1 belong to output index d, in OpenCV's order (partial
// left, full, partial right); si is the source index, alpha the weight
struct AreaAxis {
    const int* ofs;
    const int* si;
    const float* alpha;
    int cap;    // entries the si / alpha arrays hold
    int ssize;  // source size along the axis
};

// The tables come from the caller's memory (keyframe_resize_table wrote them, the launcher cannot look): offsets are clamped
// to the arrays and source indices to the frame, so whatever they hold every loop is bounded by the arguments and every read
// stays inside the buffers
__device__ __forceinline__ int kf_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void keyframe_resize_table_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                    uint32_t pixels, int H0, int W0, int H, int W, AreaAxis xt,
                                                                    AreaAxis yt, int64_t src_bytes, int wide) {
    ByteRun run(src, src_bytes, wide != 0);
    // (pixels < 2^31: 32-bit divisions)
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < pixels; idx += gridDim.x * 256u) {
        const uint32_t q = idx / (uint32_t)W;
        const int dx = (int)(idx - q * (uint32_t)W), dy = (int)(q % (uint32_t)H);
        const int64_t f = q / (uint32_t)H;
        const int xb = kf_clamp(xt.ofs[dx], 0, xt.cap), xe = kf_clamp(xt.ofs[dx + 1], xb, xt.cap);
        const int yb = kf_clamp(yt.ofs[dy], 0, yt.cap), ye = kf_clamp(yt.ofs[dy + 1], yb, yt.cap);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int j = yb; j < ye; ++j) {
            const int64_t row = (f * H0 + kf_clamp(yt.si[j], 0, H0 - 1)) * (int64_t)W0 * 3;
            const float beta = yt.alpha[j];
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;  // buf[dx] = 0, then buf[dx] += S[sx] * alpha in table order
            for (int k = xb; k < xe; ++k) {
                const int64_t o = row + (int64_t)kf_clamp(xt.si[k], 0, W0 - 1) * 3;
                const float a = xt.alpha[k];
                b0 = b0 + (float)run.get(o) * a;
                b1 = b1 + (float)run.get(o + 1) * a;
                b2 = b2 + (float)run.get(o + 2) * a;
            }
            if (j == yb) {  // the first row of a cell: sum = beta * buf
                s0 = beta * b0;
                s1 = beta * b1;
                s2 = beta * b2;
            } else {        // sum += beta * buf
                s0 = s0 + beta * b0;
                s1 = s1 + beta * b1;
                s2 = s2 + beta * b2;
            }
        }
        uint8_t* d = dst + (int64_t)idx * 3;
        d[0] = kf_round_u8(s0);
        d[1] = kf_round_u8(s1);
        d[2] = kf_round_u8(s2);
    }
}

struct KfTiles {
    int tx, ty;      // tiles per row, per column of one frame
    int first;       // the first pair that is computed: 0 with a carried frame, else 1
    int64_t total;   // (n - first) tx ty
};

// prev / cur tiles + halo -> LDS; horizontal pass -> 16 bit; vertical pass, rounding, squared difference; one partial per block
__global__ __launch_bounds__(256) void keyframe_blur_diff_kernel(const uint8_t* __restrict__ frames,
                                                                 const uint8_t* __restrict__ carry,
                                                                 uint64_t* __restrict__ partial, KfTiles tl, int H, int W) {
    __shared__ uint8_t px[2][KF_S * KF_SROWB];
    __shared__ uint16_t hz[2][KF_S * KF_ROWB];
    __shared__ uint32_t red[4];
    const int t = threadIdx.x;
    const int per_frame = tl.tx * tl.ty;
    const int64_t frame_bytes = (int64_t)H * W * 3;
    for (int64_t tile = blockIdx.x; tile < tl.total; tile += gridDim.x) {
        const int p = tl.first + (int)(tile / per_frame), r = (int)(tile % per_frame);
        const int y0 = (r / tl.tx) * KF_T, x0 = (r % tl.tx) * KF_T;
        const uint8_t* cur = frames + (int64_t)p * frame_bytes;
        const uint8_t* prev = p == 0 ? carry : cur - frame_bytes;
        for (int i = t; i < 2 * KF_S * KF_S; i += 256) {
            const int which = i / (KF_S * KF_S), q = i - which * (KF_S * KF_S);
            const int ly = q / KF_S, lx = q - ly * KF_S;
            const int gy = kf_reflect101(y0 - KF_R + ly, H), gx = kf_reflect101(x0 - KF_R + lx, W);
            const uint8_t* g = (which ? cur : prev) + ((int64_t)gy * W + gx) * 3;
            uint8_t* l = px[which] + q * 3;
            l[0] = g[0];
            l[1] = g[1];
            l[2] = g[2];
        }
        __syncthreads();
        // the row starts 4 pixels = 12 bytes left of the tile: tap k of output byte cb is byte cb + 3 k
        for (int i = t; i < 2 * KF_S * KF_ROWB; i += 256) {
            const int which = i / (KF_S * KF_ROWB), q = i - which * (KF_S * KF_ROWB);
            const int ly = q / KF_ROWB, cb = q - ly * KF_ROWB;
            const uint8_t* l = px[which] + ly * KF_SROWB + cb;
            uint32_t h = 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) h += kf_w(k) * l[3 * k];
            hz[which][q] = (uint16_t)h;  // <= 255 * 256
        }
        __syncthreads();
        uint32_t acc = 0;  // <= 12 * 255^2 per thread, 3072 * 255^2 < 2^32 per block
        for (int i = t; i < KF_T * KF_ROWB; i += 256) {
            const int ly = i / KF_ROWB, cb = i - ly * KF_ROWB;
            if (y0 + ly >= H || x0 + cb / 3 >= W) continue;
            uint32_t va = 0, vb = 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                va += kf_w(k) * hz[0][(ly + k) * KF_ROWB + cb];
                vb += kf_w(k) * hz[1][(ly + k) * KF_ROWB + cb];
            }
            const int d = (int)((va + 32768u) >> 16) - (int)((vb + 32768u) >> 16);
            acc += (uint32_t)(d * d);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += (uint32_t)__shfl_xor((int)acc, o, 64);
        if ((t & 63) == 0) red[t >> 6] = acc;
        __syncthreads();
        if (t == 0) partial[(int64_t)p * per_frame + r] = (uint64_t)red[0] + red[1] + red[2] + red[3];
        __syncthreads();  // the next tile of this workgroup overwrites px / hz / red
    }
}

// one workgroup per pair
__global__ __launch_bounds__(256) void keyframe_sum_kernel(const uint64_t* __restrict__ partial, uint64_t* __restrict__ err,
                                                           int per_frame, int first) {
    __shared__ uint64_t red[256];
    const int t = threadIdx.x, p = blockIdx.x;
    uint64_t s = 0;
    if (p >= first)
        for (int i = t; i < per_frame; i += 256) s += partial[(int64_t)p * per_frame + i];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) err[p] = red[0];
}

static inline KfTiles kf_tiles(int n, int H, int W, bool has_carry) {
    KfTiles t;
    t.tx = (W + KF_T - 1) / KF_T;
    t.ty = (H + KF_T - 1) / KF_T;
    t.first = has_carry ? 0 : 1;
    t.total = (int64_t)(n - t.first) * t.tx * t.ty;
    return t;
}

// n H W 3 when the calls take the size, else 0
static inline int64_t kf_bytes(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t hw = (int64_t)H * W;  // < 2^62
    if (hw >= KF_MAX_BYTES / 3) return 0;
    if (n > (KF_MAX_BYTES - 1) / (hw * 3)) return 0;
    return hw * 3 * n;
}

// ---- the coverage tables of OpenCV's computeResizeAreaTab, built on the host into the caller's memory
// One axis holds at most two partial entries per output index and one full entry per source index.
static inline int kf_axis_cap(int ssize, int dsize) { return ssize + 2 * dsize; }

// the table blob, 32-bit words: x.ofs[W + 1] | x.si[capx] | x.alpha[capx] | y.ofs[H + 1] | y.si[capy] | y.alpha[capy] -- a
// function of the geometry alone, so the launcher finds the parts without reading the blob
struct KfLayout {
    size_t xofs, xsi, xa, yofs, ysi, ya, words;
    int capx, capy;
};

static inline KfLayout kf_layout(int H0, int W0, int H, int W) {
    KfLayout l;
    l.capx = kf_axis_cap(W0, W);
    l.capy = kf_axis_cap(H0, H);
    l.xofs = 0;
    l.xsi = l.xofs + (size_t)W + 1;
    l.xa = l.xsi + (size_t)l.capx;
    l.yofs = l.xa + (size_t)l.capx;
    l.ysi = l.yofs + (size_t)H + 1;
    l.ya = l.ysi + (size_t)l.capy;
    l.words = l.ya + (size_t)l.capy;
    return l;
}

// the scale factor as cv::resize forms it: 1 / (dsize / ssize)
static inline double kf_scale(int ssize, int dsize) { return 1. / ((double)dsize / ssize); }

// false if the entries would not fit `cap` (they do: see kf_axis_cap)
static bool kf_area_axis(int ssize, int dsize, int cap, int* ofs, int* si, float* alpha) {
    const double scale = kf_scale(ssize, dsize);
    int k = 0;
    ofs[0] = 0;
    for (int d = 0; d < dsize; ++d) {
        const double f1 = d * scale, f2 = f1 + scale;
        const double cell = fmin(scale, ssize - f1);
        int s1 = (int)ceil(f1), s2 = (int)floor(f2);
        s2 = s2 < ssize - 1 ? s2 : ssize - 1;
        s1 = s1 < s2 ? s1 : s2;
        const int full = s2 > s1 ? s2 - s1 : 0;
        if (k + full + 2 > cap) return false;
        if (s1 - f1 > 1e-3 && s1 >= 1) {
            si[k] = s1 - 1;
            alpha[k++] = (float)((s1 - f1) / cell);
        }
        for (int s = s1; s < s2; ++s) {
            si[k] = s;
            alpha[k++] = (float)(1.0 / cell);
        }
        if (f2 - s2 > 1e-3) {
            si[k] = s2;
            alpha[k++] = (float)(fmin(fmin(f2 - s2, 1.), cell) / cell);
        }
        ofs[d + 1] = k;
    }
    return true;
}

// FRESCO_OK when the resize takes the geometry
static inline int kf_resize_geometry(int H0, int W0, int H, int W) {
    if (H0 <= 0 || W0 <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (H > H0 || W > W0) return FRESCO_EUNSUPPORTED;  // INTER_AREA enlarging is another algorithm
    if (H0 > KF_MAX_SIDE || W0 > KF_MAX_SIDE) return FRESCO_EUNSUPPORTED;
    return FRESCO_OK;
}

static inline int kf_blocks(int64_t want) { return (int)(want < KF_MAX_BLOCKS ? want : KF_MAX_BLOCKS); }

}  // namespace fresco

using namespace fresco;

extern "C" size_t keyframe_resize_table_bytes(int H0, int W0, int H, int W) {
    if (kf_resize_geometry(H0, W0, H, W) != FRESCO_OK) return 0;
    return kf_layout(H0, W0, H, W).words * 4;
}

extern "C" int keyframe_resize_table(int H0, int W0, int H, int W, void* host_table, size_t table_bytes) {
    const int rc = kf_resize_geometry(H0, W0, H, W);
    if (rc != FRESCO_OK) return rc;
    if (!host_table || !aligned_to(host_table, 4)) return FRESCO_EINVAL;
    const KfLayout l = kf_layout(H0, W0, H, W);
    if (table_bytes < l.words * 4) return FRESCO_EWORKSPACE;
    memset(host_table, 0, l.words * 4);
    int* w = static_cast<int*>(host_table);
    float* f = static_cast<float*>(host_table);
    if (!kf_area_axis(W0, W, l.capx, w + l.xofs, w + l.xsi, f + l.xa) ||
        !kf_area_axis(H0, H, l.capy, w + l.yofs, w + l.ysi, f + l.ya))
        return FRESCO_EINVAL;
    return FRESCO_OK;
}

extern "C" int keyframe_resize_area_u8(const uint8_t* src, uint8_t* dst, const void* table, size_t table_bytes, int n, int H0,
                                       int W0, int H, int W, void* stream) {
    if (!src || !dst || !table || !aligned_to(table, 4) || n <= 0) return FRESCO_EINVAL;
    const int rc = kf_resize_geometry(H0, W0, H, W);
    if (rc != FRESCO_OK) return rc;
    const int64_t src_bytes = kf_bytes(n, H0, W0);
    if (!src_bytes) return FRESCO_EUNSUPPORTED;
    const int64_t npix = (int64_t)n * H * W;  // <= n H0 W0 < 2^40
    if (npix >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    const KfLayout l = kf_layout(H0, W0, H, W);
    if (table_bytes < l.words * 4) return FRESCO_EWORKSPACE;
    const uint32_t pixels = (uint32_t)npix;
    const int wide = aligned_to(src, 4) ? 1 : 0;
    const double sx = kf_scale(W0, W), sy = kf_scale(H0, H);
    const int ix = (int)lrint(sx), iy = (int)lrint(sy);
    // cv::resize's is_area_fast; the box kernel also needs the sizes to divide (they do whenever the factor is an integer)
    const bool fast = fabs(sx - ix) < 2.220446049250313e-16 && fabs(sy - iy) < 2.220446049250313e-16 &&
                      (int64_t)W * ix == W0 && (int64_t)H * iy == H0;
    hipStream_t st = as_stream(stream);
    if (fast) {
        hipLaunchKernelGGL(keyframe_resize_box_kernel, dim3(stream_blocks(pixels)), dim3(256), 0, st, src, dst, pixels, H, W, iy,
                           ix, 1.f / (float)(ix * iy), src_bytes, wide);
        return check_launch();
    }
    const int* w = static_cast<const int*>(table);
    const float* f = static_cast<const float*>(table);
    const AreaAxis xt = {w + l.xofs, w + l.xsi, f + l.xa, l.capx, W0};
    const AreaAxis yt = {w + l.yofs, w + l.ysi, f + l.ya, l.capy, H0};
    hipLaunchKernelGGL(keyframe_resize_table_kernel, dim3(stream_blocks(pixels)), dim3(256), 0, st, src, dst, pixels, H0, W0, H,
                       W, xt, yt, src_bytes, wide);
    return check_launch();
}

extern "C" size_t keyframe_workspace_bytes(int n, int H, int W) {
    if (!kf_bytes(n, H, W) || H < KF_MIN_SIDE || W < KF_MIN_SIDE) return 0;
    const KfTiles tl = kf_tiles(n, H, W, true);
    return align_up((size_t)tl.total * sizeof(uint64_t), 256);
}

extern "C" int keyframe_frame_errors(const uint8_t* frames, const uint8_t* carry, uint64_t* err, void* workspace,
                                     size_t workspace_bytes, int n, int H, int W, void* stream) {
    if (!frames || !err || !workspace || n <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (!aligned_to(err, 8) || !aligned_to(workspace, 8)) return FRESCO_EINVAL;
    if (H < KF_MIN_SIDE || W < KF_MIN_SIDE || !kf_bytes(n, H, W)) return FRESCO_EUNSUPPORTED;
    if (workspace_bytes < keyframe_workspace_bytes(n, H, W)) return FRESCO_EWORKSPACE;
    const KfTiles tl = kf_tiles(n, H, W, carry != nullptr);
    uint64_t* partial = static_cast<uint64_t*>(workspace);
    hipStream_t st = as_stream(stream);
    if (tl.total > 0) {
        hipLaunchKernelGGL(keyframe_blur_diff_kernel, dim3(kf_blocks(tl.total)), dim3(256), 0, st, frames, carry, partial, tl, H,
                           W);
        const int rc = check_launch();
        if (rc != FRESCO_OK) return rc;
    }
    hipLaunchKernelGGL(keyframe_sum_kernel, dim3(n), dim3(256), 0, st, (const uint64_t*)partial, err, tl.tx * tl.ty, tl.first);
    return check_launch();
}
