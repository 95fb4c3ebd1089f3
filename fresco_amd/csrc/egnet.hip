// The EGNet saliency detector behind FRESCO's background smoothing (reference: src/EGNet/model.py + resnet.py, called by
// src/utils.py::get_saliency), the parts fresco_fn_gemm / fresco_fn_conv7_rgb / fresco_fn_prep have no shape for.  The
// network's 93 live convolutions run on flownet.hip's implicit-GEMM kernel from (hi, lo) fp16 operand planes (NHWC rows,
// folded BatchNorm shift + ReLU in its epilogue).  DESIGN.md section 13.
//
//   egnet_input_kernel       uint8 frames -> cv2sod's tensor: (x - mean) halved with bilinear weights (the 2 x 2 block mean),
//                            fp32 NHWC rows of 3 channels, what fresco_fn_conv7_rgb reads
//   pool3s2_kernel<-1>       MaxPool2d(3, stride 2, padding 1, ceil_mode=True) on 64-channel fp32 NHWC rows -> operand planes
//                            (pool3s2.h, shared with midas.hip)
//   egnet_resize_add_kernel  F.interpolate(bilinear, align_corners=True) on NHWC fp32 (+ addend) (ReLU) -> fp32 and / or planes
//   egnet_saliency_kernel    the tail: resize of the logit, sigmoid, k x k box sum with replicate padding, clamp, 1 - x
//
// All four are bound by memory traffic; no float atomics anywhere: same inputs, same bits.
#include "common.h"
#include "fn_split.h"
#include "pool3s2.h"

namespace fresco {

constexpr int EG_MAX_K = 15;         // widest box of the tail
constexpr int EG_TILE = 16;          // the tail's output tile (one pixel per thread)
constexpr int EG_MAX_SIDE = 32768;   // map sides of the resizes: destination index * (source side - 1) stays an int

// cv2sod (src/utils.py:26-31): image minus the channel mean, then F.interpolate(scale_factor=0.5, bilinear): source position
// 2 d + 0.5, so all four weights are 1 / 4 -- the mean of the 2 x 2 block.  The reference rounds to fp32 after the subtraction
// and after each of the three adds (absolute errors of 2^-24 * 150 on results that cancel to anything down to zero); here the
// block sum is an integer, exact, and (sum / 4 - mean) is formed in double and rounded to fp32 ONCE.
// One thread per output value.
__global__ __launch_bounds__(256) void egnet_input_kernel(const uint8_t* __restrict__ x, float* __restrict__ out, int64_t total,
                                                          int H, int W, int OH, int OW) {
    const double mean[3] = {104.00699, 116.66877, 122.67892};
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % 3);
        const int64_t p = idx / 3;
        const int ox = (int)(p % OW), oy = (int)((p / OW) % OH);
        const int64_t img = p / ((int64_t)OW * OH);
        const uint8_t* s = x + ((img * H + 2 * oy) * W + 2 * ox) * 3 + c;  // (2 oy + 1 < H, 2 ox + 1 < W: OH = H / 2, OW = W / 2)
        const int64_t row = (int64_t)W * 3;
        const int sum = (int)s[0] + (int)s[3] + (int)s[row] + (int)s[row + 3];
        out[idx] = (float)((double)sum * 0.25 - mean[c]);
    }
}

// align_corners=True source position of destination index d: d (src - 1) / (dst - 1) (0 for a single destination sample),
// as a quotient and a remainder of integers -- the first tap and the numerator of the second tap's weight are EXACT, the
// weight is rounded once.  (torch forms scale = (src - 1) / (dst - 1) and scale * d in fp32: a position off by up to
// 2^-24 * dst, times the difference of the two taps, on a result that may be much smaller than either.)  The second tap is
// the next sample, or the same one at the last; weights (1 - f, f).
__device__ __forceinline__ void egnet_tap(int d, int src, int dst, int& i0, int& i1, float& f) {
    const int den = dst > 1 ? dst - 1 : 1;
    const int num = dst > 1 ? d * (src - 1) : 0;  // (< 2^31: both sizes are below 2^15.5, launcher)
    i0 = num / den;
    f = (float)(num - i0 * den) / (float)den;
    i1 = i0 + (i0 < src - 1 ? 1 : 0);
}

// One thread per (output pixel, four channels).  same: the sizes agree and the resize is the identity -- an exact copy.
__global__ __launch_bounds__(256) void egnet_resize_add_kernel(const float* __restrict__ x, const float* __restrict__ addend,
                                                               float* __restrict__ out, half_t* __restrict__ o_hi,
                                                               half_t* __restrict__ o_lo, int64_t total, int h, int w, int H,
                                                               int W, int C, int relu, float scale, int32_t* range_flag) {
    const int Q = C / 4;
    const bool same = h == H && w == W;
    bool sat = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % Q) * 4;
        const int64_t p = idx / Q;
        floatx4 v;
        if (same) {
            v = *reinterpret_cast<const floatx4*>(x + p * C + c);
        } else {
            const int ox = (int)(p % W), oy = (int)((p / W) % H);
            const int64_t img = p / ((int64_t)W * H);
            int x0, x1, y0, y1;
            float fx, fy;
            egnet_tap(ox, w, W, x0, x1, fx);
            egnet_tap(oy, h, H, y0, y1, fy);
            const float* b = x + img * h * w * C + c;
            const floatx4 a00 = *reinterpret_cast<const floatx4*>(b + ((int64_t)y0 * w + x0) * C);
            const floatx4 a01 = *reinterpret_cast<const floatx4*>(b + ((int64_t)y0 * w + x1) * C);
            const floatx4 a10 = *reinterpret_cast<const floatx4*>(b + ((int64_t)y1 * w + x0) * C);
            const floatx4 a11 = *reinterpret_cast<const floatx4*>(b + ((int64_t)y1 * w + x1) * C);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[e] = (1.f - fy) * ((1.f - fx) * a00[e] + fx * a01[e]) + fy * ((1.f - fx) * a10[e] + fx * a11[e]);
        }
        if (addend) {
            const floatx4 t = *reinterpret_cast<const floatx4*>(addend + p * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += t[e];
        }
        if (relu)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        if (out) *reinterpret_cast<floatx4*>(out + p * C + c) = v;
        if (o_hi) sat |= fn_split_store4(v, scale, o_hi, o_lo, p * C + c);
    }
    fn_flag_range(range_flag, sat);
}

// The resized logit at pixel (y, x) of the (Hs, Ws) map, from the (h, w) map m of one image.
__device__ __forceinline__ float egnet_logit_at(const float* __restrict__ m, int y, int x, int h, int w, int Hs, int Ws) {
    int x0, x1, y0, y1;
    float fx, fy;
    egnet_tap(x, w, Ws, x0, x1, fx);
    egnet_tap(y, h, Hs, y0, y1, fy);
    return (1.f - fy) * ((1.f - fx) * m[y0 * w + x0] + fx * m[y0 * w + x1]) +
           fy * ((1.f - fx) * m[y1 * w + x0] + fx * m[y1 * w + x1]);
}

// get_saliency's 1 - dilate(sigmoid(up_sal_final[-1])) in one pass.  A block owns a 16 x 16 tile of the output: the sigmoid
// of the resized logit over the tile and its halo (replicate padding = coordinates clamped to the map) goes to LDS once, then
// every thread adds its k x k window in row order -- a fixed order.  grid (ceil(Ws / 16), ceil(Hs / 16), n).
__global__ __launch_bounds__(256) void egnet_saliency_kernel(const float* __restrict__ logit, float* __restrict__ out,
                                                             float* __restrict__ logit_out, int h, int w, int Hs, int Ws,
                                                             int k) {
    __shared__ float sig[(EG_TILE + EG_MAX_K - 1) * (EG_TILE + EG_MAX_K - 1)];
    const int r = k >> 1, T = EG_TILE + k - 1;
    const int img = blockIdx.z, oy0 = blockIdx.y * EG_TILE, ox0 = blockIdx.x * EG_TILE;
    const float* m = logit + (int64_t)img * h * w;
    for (int e = threadIdx.x; e < T * T; e += 256) {
        const int ty = e / T, tx = e - ty * T;
        const int y = min(max(oy0 + ty - r, 0), Hs - 1), x = min(max(ox0 + tx - r, 0), Ws - 1);
        const float v = egnet_logit_at(m, y, x, h, w, Hs, Ws);
        sig[e] = 1.f / (1.f + expf(-v));
    }
    __syncthreads();
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int y = oy0 + ty, x = ox0 + tx;
    if (y >= Hs || x >= Ws) return;
    float s = 0.f;
    for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) s += sig[(ty + ky) * T + tx + kx];
    s = fminf(fmaxf(s, 0.f), 1.f);
    const int64_t o = ((int64_t)img * Hs + y) * Ws + x;
    out[o] = 1.f - s;
    if (logit_out) logit_out[o] = egnet_logit_at(m, y, x, h, w, Hs, Ws);
}

// MaxPool2d(3, 2, 1, ceil_mode=True): ceil((size + 2 pad - k) / stride) + 1, minus one where the last window would start
// beyond the input and its left padding
static inline int eg_pool_size(int size) {
    int o = (size + 2 - 3 + 1) / 2 + 1;
    if ((o - 1) * 2 >= size + 1) --o;
    return o;
}

}  // namespace fresco

using namespace fresco;

extern "C" int fresco_egnet_input(const uint8_t* frames, float* out, int n, int H, int W, void* stream) {
    if (!frames || !out || n <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (!aligned_to(out, 4)) return FRESCO_EINVAL;
    if (H < 2 || W < 2) return FRESCO_EUNSUPPORTED;  // (no halved pixel)
    if ((int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    const int OH = H / 2, OW = W / 2;
    const int64_t total = (int64_t)n * OH * OW * 3;
    hipLaunchKernelGGL(egnet_input_kernel, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), frames, out, total, H, W,
                       OH, OW);
    return check_launch();
}

extern "C" int fresco_egnet_pool(const float* x, float* out, void* out_hi, void* out_lo, int n, int H, int W, int C,
                                 float split_scale, int32_t* range_flag, void* stream) {
    if (!x || !out_hi || !out_lo || n <= 0 || H <= 0 || W <= 0 || C <= 0 || !(split_scale > 0.f)) return FRESCO_EINVAL;
    if (C != 64) return FRESCO_EUNSUPPORTED;
    if ((int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(out, 16) || !aligned_to(out_hi, 8) || !aligned_to(out_lo, 8)) return FRESCO_EINVAL;
    const int OH = eg_pool_size(H), OW = eg_pool_size(W);
    const int64_t total = (int64_t)n * OH * OW * (C / 4);
    hipLaunchKernelGGL(pool3s2_kernel<-1>, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), x, out,
                       static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), total, H, W, OH, OW, split_scale, range_flag);
    return check_launch();
}

extern "C" int fresco_egnet_resize_add(const float* x, const float* addend, float* out, void* out_hi, void* out_lo, int n,
                                       int h, int w, int H, int W, int C, int relu, float split_scale, int32_t* range_flag,
                                       void* stream) {
    if (!x || n <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || C <= 0 || (!out && !out_hi) ||
        ((out_hi != nullptr) != (out_lo != nullptr)))
        return FRESCO_EINVAL;
    if (out_hi && !(split_scale > 0.f)) return FRESCO_EINVAL;
    if (C % 32 != 0 || C > 512) return FRESCO_EUNSUPPORTED;
    if (h > EG_MAX_SIDE || w > EG_MAX_SIDE || H > EG_MAX_SIDE || W > EG_MAX_SIDE) return FRESCO_EUNSUPPORTED;
    if ((int64_t)n * H * W >= (int64_t)1 << 31 || (int64_t)n * h * w >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(addend, 16) || !aligned_to(out, 16) || !aligned_to(out_hi, 8) || !aligned_to(out_lo, 8))
        return FRESCO_EINVAL;
    const int64_t total = (int64_t)n * H * W * (C / 4);
    hipLaunchKernelGGL(egnet_resize_add_kernel, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), x, addend, out,
                       static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), total, h, w, H, W, C, relu ? 1 : 0,
                       split_scale, range_flag);
    return check_launch();
}

extern "C" int fresco_egnet_saliency(const float* logit, float* out, float* logit_out, int n, int h, int w, int Hs, int Ws,
                                     int k, void* stream) {
    if (!logit || !out || n <= 0 || h <= 0 || w <= 0 || Hs <= 0 || Ws <= 0 || k <= 0) return FRESCO_EINVAL;
    if (k % 2 == 0 || k > EG_MAX_K) return FRESCO_EUNSUPPORTED;
    if (h > EG_MAX_SIDE || w > EG_MAX_SIDE || Hs > EG_MAX_SIDE || Ws > EG_MAX_SIDE) return FRESCO_EUNSUPPORTED;
    if (n > 65535 || (Hs + EG_TILE - 1) / EG_TILE > 65535) return FRESCO_EUNSUPPORTED;
    if ((int64_t)n * Hs * Ws >= (int64_t)1 << 31 || (int64_t)h * w >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(logit, 4) || !aligned_to(out, 4) || !aligned_to(logit_out, 4)) return FRESCO_EINVAL;
    hipLaunchKernelGGL(egnet_saliency_kernel, dim3((Ws + EG_TILE - 1) / EG_TILE, (Hs + EG_TILE - 1) / EG_TILE, n), dim3(256), 0,
                       as_stream(stream), logit, out, logit_out, h, w, Hs, Ws, k);
    return check_launch();
}
