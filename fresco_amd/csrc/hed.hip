// The HED annotator of the ControlNet condition (reference: src/ControlNet/annotator/hed/__init__.py), the parts
// fresco_fn_gemm has no shape for.  The network is five VGG blocks of 3 x 3 convolutions (13 in all) with a 1 x 1 "side"
// projection per block; the convolutions run on flownet.hip's implicit-GEMM kernel from (hi, lo) fp16 operand planes
// (NHWC rows, bias + ReLU in its epilogue).  DESIGN.md section 12.
//
//   hed_input_kernel      uint8 RGB frames -> the planes of (x - norm) * scale, 32 channels per pixel (3 real + 29 zeros:
//                         the first convolution runs as K = 9 * 32), the subtraction BEFORE the zero padding
//   hed_side_pool_kernel  the last activation of a block, fp32 NHWC, read ONCE: the side projection (a dot product over
//                         the channels per pixel, fixed order) and the planes of max_pool2d(h, 2, 2), the next block's input
//   hed_fuse_kernel       the five side maps -> bilinear resize to the frame (cv2.resize INTER_LINEAR semantics), mean,
//                         float64 sigmoid, * 255, truncation to uint8; optionally the fp32 mean and the ControlNet condition
//
// All three are bound by memory traffic (section 12 has the bytes); no float atomics anywhere: same inputs, same bits.
// Built with -ffp-contract=off: the interpolation and the condition follow the reference's operation order.
#include "common.h"
#include "fn_split.h"

namespace fresco {

constexpr int HED_LEVELS = 5;

// One thread per (pixel, 16-byte piece of its 64-byte plane row): piece 0 carries the three channels, pieces 1-3 are zeros.
__global__ __launch_bounds__(256) void hed_input_kernel(const uint8_t* __restrict__ x, half_t* __restrict__ o_hi,
                                                        half_t* __restrict__ o_lo, int64_t npix,
                                                        const float* __restrict__ norm3, float scale,
                                                        int32_t* range_flag) {
    const float norm[3] = {norm3[0], norm3[1], norm3[2]};
    bool sat = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < npix * 4; idx += (int64_t)gridDim.x * 256) {
        const int64_t p = idx >> 2;
        half8_t h = {0, 0, 0, 0, 0, 0, 0, 0}, l = {0, 0, 0, 0, 0, 0, 0, 0};
        if ((idx & 3) == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                half_t hh, ll;
                sat |= fn_split((float)x[p * 3 + c] - norm[c], scale, hh, ll);
                h[c] = hh;
                l[c] = ll;
            }
        }
        *reinterpret_cast<half8_t*>(o_hi + idx * 8) = h;
        *reinterpret_cast<half8_t*>(o_lo + idx * 8) = l;
    }
    fn_flag_range(range_flag, sat);
}

// A QUAD is the 2 x 2 pixels of one pooled pixel (the odd last row / column of a map makes quads with 2 or 1 pixels: they
// have side outputs and no pooled pixel).  16 lanes per quad, lane t owns channels 4 (16 j + t) .. + 3 for j < NJ = C / 64:
// per j a lane group reads 256 consecutive bytes of each of the four pixel rows and writes 128 of each plane row.
// The dot product: a lane's fused multiply-adds in channel order, then the 16 lanes by a fixed xor tree.
template <int NJ>
__global__ __launch_bounds__(256) void hed_side_pool_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ proj,
                                                            half_t* __restrict__ o_hi, half_t* __restrict__ o_lo, int n,
                                                            int H, int W, float scale, int32_t* range_flag) {
    constexpr int C = NJ * 64;
    const int t = threadIdx.x & 15, grp = threadIdx.x >> 4;
    floatx4 wv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) wv[j] = *reinterpret_cast<const floatx4*>(w + (j * 16 + t) * 4);
    const float b = bias ? bias[0] : 0.f;
    const int QH = (H + 1) >> 1, QW = (W + 1) >> 1, PH = H >> 1, PW = W >> 1;
    const int64_t nquads = (int64_t)n * QH * QW;
    bool sat = false;
    // (the trip count is the same for every lane of a block: the shuffles below see whole waves)
    for (int64_t base = (int64_t)blockIdx.x * 16; base < nquads; base += (int64_t)gridDim.x * 16) {
        const bool qok = base + grp < nquads;
        const int64_t quad = qok ? base + grp : 0;
        const int qx = (int)(quad % QW), qy = (int)((quad / QW) % QH);
        const int64_t img = quad / ((int64_t)QW * QH);
        bool ok[4];
        int64_t pix[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int y = 2 * qy + (d >> 1), xx = 2 * qx + (d & 1);
            ok[d] = qok && y < H && xx < W;
            pix[d] = ok[d] ? (img * H + y) * W + xx : 0;
        }
        const bool pool = o_hi && ok[3];  // all four pixels exist
        const int64_t prow = ((img * PH + qy) * PW + qx) * C;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = (j * 16 + t) * 4;
            floatx4 v[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                v[d] = floatx4{0.f, 0.f, 0.f, 0.f};
                if (ok[d]) v[d] = *reinterpret_cast<const floatx4*>(h + pix[d] * C + c);
            }
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[d] = fmaf(v[d][e], wv[j][e], acc[d]);
            if (pool) {
                half4_t ph, pl;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    half_t hh, ll;
                    sat |= fn_split(fmaxf(fmaxf(v[0][e], v[1][e]), fmaxf(v[2][e], v[3][e])), scale, hh, ll);
                    ph[e] = hh;
                    pl[e] = ll;
                }
                *reinterpret_cast<half4_t*>(o_hi + prow + c) = ph;
                *reinterpret_cast<half4_t*>(o_lo + prow + c) = pl;
            }
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[d] += __shfl_xor(acc[d], o, 64);
            if (proj && t == 0 && ok[d]) proj[pix[d]] = acc[d] + b;
        }
    }
    fn_flag_range(range_flag, sat);
}

struct HedSides {
    const float* p[HED_LEVELS];  // level k is (n, H >> k, W >> k)
};

// cv2.resize(INTER_LINEAR) source position of destination index d: ((d + 0.5) * (src / dst) - 0.5) formed in double and
// rounded to float; below the first sample -> the first sample, at or past the last -> the last.  i1 is the second tap
// (never outside the map: its weight is zero where it would be).
__device__ __forceinline__ void hed_tap(int d, int src, int dst, int& i0, int& i1, float& f) {
    f = (float)(((double)d + 0.5) * ((double)src / (double)dst) - 0.5);
    i0 = (int)floorf(f);
    f -= (float)i0;
    if (i0 < 0) {
        i0 = 0;
        f = 0.f;
    }
    if (i0 >= src - 1) {
        i0 = src - 1;
        f = 0.f;
    }
    i1 = i0 + 1 < src ? i0 + 1 : src - 1;
}

// One thread per pixel of the frame (n H W < 2^31: launcher).  T: element type of the optional condition.
template <typename T>
__global__ __launch_bounds__(256) void hed_fuse_kernel(HedSides s, uint8_t* __restrict__ out, float* __restrict__ logit,
                                                       T* __restrict__ cond, uint32_t total, int H, int W) {
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const uint32_t img = idx / HW, r = idx - img * HW;
        const int y = (int)(r / (uint32_t)W), x = (int)(r - (uint32_t)y * (uint32_t)W);
        float e[HED_LEVELS];
        e[0] = s.p[0][idx];  // level 1: cv2.resize to the same size returns the map
#pragma unroll
        for (int k = 1; k < HED_LEVELS; ++k) {
            const int hh = H >> k, ww = W >> k;
            const float* m = s.p[k] + (int64_t)img * (hh * ww);
            int x0, x1, y0, y1;
            float fx, fy;
            hed_tap(x, ww, W, x0, x1, fx);
            hed_tap(y, hh, H, y0, y1, fy);
            // horizontal pass on the two source rows, then the vertical one
            const float r0 = m[y0 * ww + x0] * (1.f - fx) + m[y0 * ww + x1] * fx;
            const float r1 = m[y1 * ww + x0] * (1.f - fx) + m[y1 * ww + x1] * fx;
            e[k] = r0 * (1.f - fy) + r1 * fy;
        }
        const float mean = ((((e[0] + e[1]) + e[2]) + e[3]) + e[4]) / 5.f;
        double v = 1.0 / (1.0 + exp(-(double)mean)) * 255.0;
        v = v >= 0.0 ? (v > 255.0 ? 255.0 : v) : 0.0;  // (a NaN mean gives 0)
        const uint8_t u = (uint8_t)v;
        out[idx] = u;
        if (logit) logit[idx] = mean;
        if (cond) {
            // numpy2tensor(u) * 0.5 + 0.5 in PyTorch's fp32 order on the device: x / 255.0 there is x * (1 / 255.0)
            const float c = (((float)u * (1.f / 255.f)) * 2.f - 1.f) * 0.5f + 0.5f;
            T* o = cond + ((int64_t)img * 3 * HW + r);
            const T cv = (T)c;
            o[0] = cv;
            o[HW] = cv;
            o[2 * (int64_t)HW] = cv;
        }
    }
}

}  // namespace fresco

using namespace fresco;

extern "C" int fresco_hed_input(const uint8_t* frames, const float* norm, void* out_hi, void* out_lo, int n, int H, int W,
                                float split_scale, int32_t* range_flag, void* stream) {
    if (!frames || !norm || !out_hi || !out_lo || n <= 0 || H <= 0 || W <= 0 || !(split_scale > 0.f)) return FRESCO_EINVAL;
    if (!aligned_to(norm, 4) || !aligned_to(out_hi, 16) || !aligned_to(out_lo, 16)) return FRESCO_EINVAL;
    const int64_t npix = (int64_t)n * H * W;
    if (npix >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(hed_input_kernel, dim3(stream_blocks(npix * 4)), dim3(256), 0, as_stream(stream), frames,
                       static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), npix, norm, split_scale, range_flag);
    return check_launch();
}

extern "C" int fresco_hed_side_pool(const float* h, const float* w, const float* bias, float* proj, void* pool_hi,
                                    void* pool_lo, int n, int H, int W, int C, float split_scale, int32_t* range_flag,
                                    void* stream) {
    if (!h || !w || n <= 0 || H <= 0 || W <= 0 || C <= 0 || (!proj && !pool_hi) || ((pool_hi != nullptr) != (pool_lo != nullptr)))
        return FRESCO_EINVAL;
    if (pool_hi && !(split_scale > 0.f)) return FRESCO_EINVAL;
    if (C != 64 && C != 128 && C != 256 && C != 512) return FRESCO_EUNSUPPORTED;
    if (pool_hi && (H < 2 || W < 2)) return FRESCO_EUNSUPPORTED;  // (no pooled pixel to write)
    if ((int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(h, 16) || !aligned_to(w, 16) || !aligned_to(bias, 4) || !aligned_to(proj, 4) || !aligned_to(pool_hi, 16) ||
        !aligned_to(pool_lo, 16))
        return FRESCO_EINVAL;
    const int64_t nquads = (int64_t)n * ((H + 1) / 2) * ((W + 1) / 2);
    const dim3 grid(stream_blocks(nquads * 16));
    half_t* ph = static_cast<half_t*>(pool_hi);
    half_t* pl = static_cast<half_t*>(pool_lo);
    hipStream_t st = as_stream(stream);
#define HED_SP(NJ_)                                                                                                     \
    hipLaunchKernelGGL(hed_side_pool_kernel<NJ_>, grid, dim3(256), 0, st, h, w, bias, proj, ph, pl, n, H, W, split_scale, \
                       range_flag)
    if (C == 64)
        HED_SP(1);
    else if (C == 128)
        HED_SP(2);
    else if (C == 256)
        HED_SP(4);
    else
        HED_SP(8);
#undef HED_SP
    return check_launch();
}

extern "C" int fresco_hed_fuse(const float* s1, const float* s2, const float* s3, const float* s4, const float* s5,
                               uint8_t* out, float* logit, void* cond, int cond_dtype, int n, int H, int W, void* stream) {
    if (!s1 || !s2 || !s3 || !s4 || !s5 || !out || n <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (cond && cond_dtype != FRESCO_F16 && cond_dtype != FRESCO_BF16 && cond_dtype != FRESCO_F32) return FRESCO_EINVAL;
    if (H < 16 || W < 16) return FRESCO_EUNSUPPORTED;  // (level 5 = the size halved four times must have a pixel)
    const int64_t total = (int64_t)n * H * W;
    if (total >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(s1, 4) || !aligned_to(s2, 4) || !aligned_to(s3, 4) || !aligned_to(s4, 4) || !aligned_to(s5, 4) ||
        !aligned_to(logit, 4) || !aligned_to(cond, cond_dtype == FRESCO_F32 ? 4 : 2))
        return FRESCO_EINVAL;
    const HedSides s = {{s1, s2, s3, s4, s5}};
    const dim3 grid(stream_blocks(total));
    hipStream_t st = as_stream(stream);
    if (cond && cond_dtype == FRESCO_F16)
        hipLaunchKernelGGL(hed_fuse_kernel<half_t>, grid, dim3(256), 0, st, s, out, logit, static_cast<half_t*>(cond),
                           (uint32_t)total, H, W);
    else if (cond && cond_dtype == FRESCO_BF16)
        hipLaunchKernelGGL(hed_fuse_kernel<bf16_t>, grid, dim3(256), 0, st, s, out, logit, static_cast<bf16_t*>(cond),
                           (uint32_t)total, H, W);
    else
        hipLaunchKernelGGL(hed_fuse_kernel<float>, grid, dim3(256), 0, st, s, out, logit, static_cast<float*>(cond),
                           (uint32_t)total, H, W);
    return check_launch();
}
