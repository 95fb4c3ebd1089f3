// The MiDaS depth annotator (reference: src/ControlNet/annotator/midas, DPTDepthModel on the vitb_rn50_384 backbone), the parts
// fresco_fn_gemm / fresco_attn_f32 / fresco_egnet_resize_add have no shape for (include/fresco_midas.h).  The network's
// convolutions and linear layers run on flownet.hip's GEMM from (hi, lo) fp16 operand planes.  DESIGN.md section 16.
//
//   midas_input_kernel         uint8 frames -> x / 127.5 - 1, fp32 NHWC rows of 3 channels (the stem splits them itself)
//   gn_stats_kernel<float> / gn_finish_kernel   GroupNorm(32): the statistics pass shared with vae.hip (groupnorm_stats.h)
//   midas_gn_apply_kernel      (x - mean) rstd gamma + beta [ReLU] [+ residual, ReLU] -> fp32 and / or planes, the planes with a
//                              row pitch of their own (the far-side zero border of a "same" stride-2 convolution)
//   pool3s2_kernel<0>          MaxPool2dSame(3, 2) at even sizes: windows start AT 2 oy (0 before, 1 after) (pool3s2.h, shared
//                              with egnet.hip; H, W even: the first two rows and columns of every window exist)
//   midas_layernorm_kernel     LayerNorm over up to 1024 channels, one wave per row
//   midas_tokens_kernel        [cls | grid] + positional embedding
//   midas_head_merge_kernel    (head * n + image, L, 64) attention output -> (n L, heads 64) rows
//   midas_rowbias_gelu_kernel  GELU(x + a per-image bias row): ProjectReadout's cls half
//   midas_minmax_kernel / midas_tail_kernel   per-frame range; depth image, Sobel normals, the ControlNet condition
//
// All are bound by memory traffic.  Built with -ffp-contract=off: the tail follows the reference's fp32 operation order.
#include "common.h"
#include "fn_split.h"
#include "groupnorm_stats.h"
#include "pool3s2.h"
#include "../../include/fresco_midas.h"

namespace fresco {

constexpr int MD_GROUPS = GN_GROUPS;
constexpr int MD_LN_MAXQ = 4;      // 16-byte pieces per lane of a LayerNorm row: C <= 64 * 4 * 4
constexpr int MD_MM_BLOCKS = 64;   // partial min / max pairs per frame

__global__ __launch_bounds__(256) void midas_input_kernel(const uint8_t* __restrict__ x, float* __restrict__ out, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        out[i] = (float)x[i] / 127.5f - 1.0f;
}

// One thread per (pixel, four channels).
__global__ __launch_bounds__(256) void midas_gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ residual,
                                                             float* __restrict__ y, half_t* __restrict__ o_hi,
                                                             half_t* __restrict__ o_lo, int64_t total, int H, int W, int C,
                                                             int plane_h, int plane_w, int relu, float scale,
                                                             int32_t* range_flag) {
    const int Q = C >> 2, cpg = C / MD_GROUPS;
    const int64_t HW = (int64_t)H * W;
    bool sat = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % Q) * 4;
        const int64_t p = idx / Q;
        const int64_t img = p / HW;
        floatx4 v = *reinterpret_cast<const floatx4*>(x + p * C + c);
        const floatx4 ga = *reinterpret_cast<const floatx4*>(gamma + c), be = *reinterpret_cast<const floatx4*>(beta + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int g = (int)img * MD_GROUPS + (c + e) / cpg;
            v[e] = (v[e] - mean[g]) * rstd[g] * ga[e] + be[e];
            if (relu) v[e] = fmaxf(v[e], 0.f);
        }
        if (residual) {
            const floatx4 r = *reinterpret_cast<const floatx4*>(residual + p * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e] + r[e], 0.f);
        }
        if (y) *reinterpret_cast<floatx4*>(y + p * C + c) = v;
        if (o_hi) {
            const int64_t rem = p - img * HW;
            const int py = (int)(rem / W), px = (int)(rem - (int64_t)py * W);
            sat |= fn_split_store4(v, scale, o_hi, o_lo, ((img * plane_h + py) * plane_w + px) * C + c);
        }
    }
    fn_flag_range(range_flag, sat);
}

// One wave per row, four rows per workgroup; lane l holds the 16-byte pieces l, l + 64, ... of the row in registers.
__global__ __launch_bounds__(256) void midas_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ y,
                                                              half_t* __restrict__ o_hi, half_t* __restrict__ o_lo, int64_t M,
                                                              int C, float eps, float scale, int32_t* range_flag) {
    const int lane = threadIdx.x & 63, Q = C >> 2;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;  // (wave-uniform; no barrier below)
    floatx4 v[MD_LN_MAXQ];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MD_LN_MAXQ; ++k) {
        const int q = lane + 64 * k;
        v[k] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (q < Q) v[k] = *reinterpret_cast<const floatx4*>(x + row * C + q * 4);
        s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    }
    const float mean = wave_sum(s) / (float)C;
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < MD_LN_MAXQ; ++k) {
        if (lane + 64 * k < Q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[k][e] -= mean;
                s2 += v[k][e] * v[k][e];
            }
        }
    }
    const float rstd = 1.f / sqrtf(wave_sum(s2) / (float)C + eps);
    bool sat = false;
#pragma unroll
    for (int k = 0; k < MD_LN_MAXQ; ++k) {
        const int q = lane + 64 * k;
        if (q < Q) {
            const floatx4 ga = *reinterpret_cast<const floatx4*>(gamma + q * 4), be = *reinterpret_cast<const floatx4*>(beta + q * 4);
            floatx4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = v[k][e] * rstd * ga[e] + be[e];
            if (y) *reinterpret_cast<floatx4*>(y + row * C + q * 4) = o;
            sat |= fn_split_store4<true>(o, scale, o_hi, o_lo, row * C + q * 4);
        }
    }
    fn_flag_range(o_hi ? range_flag : nullptr, sat);
}

__global__ __launch_bounds__(256) void midas_tokens_kernel(const float* __restrict__ grid, const float* __restrict__ cls,
                                                           const float* __restrict__ pos, float* __restrict__ out, int64_t total,
                                                           int L, int C) {
    const int Q = C >> 2;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % Q) * 4;
        const int64_t row = idx / Q;
        const int t = (int)(row % L);
        const int64_t img = row / L;
        const floatx4 a = t == 0 ? *reinterpret_cast<const floatx4*>(cls + c)
                                 : *reinterpret_cast<const floatx4*>(grid + (img * (L - 1) + t - 1) * C + c);
        const floatx4 b = *reinterpret_cast<const floatx4*>(pos + (int64_t)t * C + c);
        *reinterpret_cast<floatx4*>(out + row * C + c) = a + b;
    }
}

__global__ __launch_bounds__(256) void midas_head_merge_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                               half_t* __restrict__ o_hi, half_t* __restrict__ o_lo,
                                                               int64_t total, int n, int L, int heads, float scale,
                                                               int32_t* range_flag) {
    bool sat = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int d = (int)(idx & 15) * 4;
        const int h = (int)((idx >> 4) % heads);
        const int64_t row = (idx >> 4) / heads;
        const int64_t img = row / L, t = row - img * L;
        const floatx4 v = *reinterpret_cast<const floatx4*>(x + (((int64_t)h * n + img) * L + t) * 64 + d);
        const int64_t o = row * heads * 64 + h * 64 + d;
        if (out) *reinterpret_cast<floatx4*>(out + o) = v;
        if (o_hi) sat |= fn_split_store4(v, scale, o_hi, o_lo, o);
    }
    fn_flag_range(range_flag, sat);
}

__global__ __launch_bounds__(256) void midas_rowbias_gelu_kernel(const float* __restrict__ x, const float* __restrict__ rowbias,
                                                                 float* __restrict__ out, half_t* __restrict__ o_hi,
                                                                 half_t* __restrict__ o_lo, int64_t total, int C,
                                                                 int rows_per_img, float scale, int32_t* range_flag) {
    const int Q = C >> 2;
    bool sat = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % Q) * 4;
        const int64_t row = idx / Q;
        floatx4 v = *reinterpret_cast<const floatx4*>(x + row * C + c);
        const floatx4 b = *reinterpret_cast<const floatx4*>(rowbias + (row / rows_per_img) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = v[e] + b[e];
            v[e] = 0.5f * t * (1.f + erff(t * 0.70710678118654752440f));
        }
        if (out) *reinterpret_cast<floatx4*>(out + row * C + c) = v;
        sat |= fn_split_store4<true>(v, scale, o_hi, o_lo, row * C + c);
    }
    fn_flag_range(o_hi ? range_flag : nullptr, sat);
}

// grid (MD_MM_BLOCKS, n): the minimum and maximum of the block's share of one frame (order-free: exact whatever the grid).
__global__ __launch_bounds__(256) void midas_minmax_kernel(const float* __restrict__ depth, float* __restrict__ part, int HW) {
    __shared__ float lo[4], hi[4];
    const float* d = depth + (int64_t)blockIdx.y * HW;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        mn = fminf(mn, d[i]);
        mx = fmaxf(mx, d[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        lo[threadIdx.x >> 6] = mn;
        hi[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = part + ((int64_t)blockIdx.y * MD_MM_BLOCKS + blockIdx.x) * 2;
        o[0] = fminf(fminf(lo[0], lo[1]), fminf(lo[2], lo[3]));
        o[1] = fmaxf(fmaxf(hi[0], hi[1]), fmaxf(hi[2], hi[3]));
    }
}

__device__ __forceinline__ int midas_reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// grid (blocks, n), one thread per pixel (grid-stride inside the frame).  The reference's lines in fp32, one rounding per
// operation: t = d - min, pt = t / max(t), trunc(clip(pt * 255)); Sobel as cv2's separable filter ([-1 0 1] along the
// derivative's axis first, [1 2 1] across: (a + c) + 2 b); (gx, gy, a) / sqrt((gx^2 + gy^2) + a^2).
template <typename T>
__global__ __launch_bounds__(256) void midas_tail_kernel(const float* __restrict__ depth, const float* __restrict__ part,
                                                         uint8_t* __restrict__ dimg, uint8_t* __restrict__ nimg,
                                                         T* __restrict__ cond, int H, int W, float a, float bg_th) {
    __shared__ float range[2];
    const int img = blockIdx.y, HW = H * W;
    if (threadIdx.x < 64) {
        float mn = INFINITY, mx = -INFINITY;
        if (threadIdx.x < MD_MM_BLOCKS) {
            mn = part[((int64_t)img * MD_MM_BLOCKS + threadIdx.x) * 2];
            mx = part[((int64_t)img * MD_MM_BLOCKS + threadIdx.x) * 2 + 1];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        }
        if (threadIdx.x == 0) {
            range[0] = mn;
            range[1] = mx;
        }
    }
    __syncthreads();
    const float mn = range[0], span = range[1] - range[0];
    const float* d = depth + (int64_t)img * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const int y = i / W, x = i - y * W;
        const bool flat = !(span > 0.f);
        const float pt = flat ? 0.f : (d[i] - mn) / span;
        float v = pt * 255.0f;
        v = v >= 0.f ? (v > 255.f ? 255.f : v) : 0.f;
        const uint8_t u = (uint8_t)v;
        dimg[(int64_t)img * HW + i] = u;
        const int ym = midas_reflect101(y - 1, H), yp = midas_reflect101(y + 1, H);
        const int xm = midas_reflect101(x - 1, W), xp = midas_reflect101(x + 1, W);
        const float* r0 = d + ym * W;
        const float* r1 = d + y * W;
        const float* r2 = d + yp * W;
        float gx = ((r0[xp] - r0[xm]) + (r2[xp] - r2[xm])) + 2.f * (r1[xp] - r1[xm]);
        float gy = ((r2[xm] + r2[xp]) + 2.f * r2[x]) - ((r0[xm] + r0[xp]) + 2.f * r0[x]);
        if (flat || pt < bg_th) gx = gy = 0.f;
        const float nrm = sqrtf((gx * gx + gy * gy) + a * a);
        const float nv[3] = {gx / nrm, gy / nrm, a / nrm};
        uint8_t* no = nimg + ((int64_t)img * HW + i) * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            float w = nv[e] * 127.5f + 127.5f;
            w = w >= 0.f ? (w > 255.f ? 255.f : w) : 0.f;
            no[e] = (uint8_t)w;
        }
        if (cond) {
            // numpy2tensor(u) * 0.5 + 0.5 in PyTorch's fp32 order on the device, as hed_fuse_kernel writes it
            const float c = (((float)u * (1.f / 255.f)) * 2.f - 1.f) * 0.5f + 0.5f;
            T* o = cond + ((int64_t)img * 3 * HW + i);
            const T cv = (T)c;
            o[0] = cv;
            o[HW] = cv;
            o[2 * (int64_t)HW] = cv;
        }
    }
}

static inline bool md_gn_channels(int C) { return C == 64 || C == 128 || C == 256 || C == 512 || C == 1024; }
static inline bool md_planes_ok(const void* hi, const void* lo, float scale) {
    return (hi != nullptr) == (lo != nullptr) && (!hi || (scale > 0.f && aligned_to(hi, 8) && aligned_to(lo, 8)));
}

}  // namespace fresco

using namespace fresco;

extern "C" int midas_input(const uint8_t* frames, float* out, int n, int H, int W, void* stream) {
    if (!frames || !out || n <= 0 || H <= 0 || W <= 0 || !aligned_to(out, 4)) return FRESCO_EINVAL;
    if ((int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    const int64_t total = (int64_t)n * H * W * 3;
    hipLaunchKernelGGL(midas_input_kernel, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), frames, out, total);
    return check_launch();
}

extern "C" size_t midas_groupnorm_workspace_bytes(int n, int P, int C) {
    if (n <= 0 || P <= 0 || !md_gn_channels(C)) return 0;
    return gn_workspace_bytes(n, P, false);
}

extern "C" int midas_groupnorm_stats(const float* x, float* mean, float* rstd, void* workspace, size_t workspace_bytes, int n,
                                     int P, int C, float eps, void* stream) {
    if (!x || !mean || !rstd || !workspace || n <= 0 || P <= 0 || C <= 0 || !(eps >= 0.f)) return FRESCO_EINVAL;
    if (!md_gn_channels(C)) return FRESCO_EUNSUPPORTED;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(workspace, 8) || !aligned_to(mean, 4) || !aligned_to(rstd, 4)) return FRESCO_EINVAL;
    if (workspace_bytes < midas_groupnorm_workspace_bytes(n, P, C)) return FRESCO_EWORKSPACE;
    return gn_statistics(x, workspace, mean, rstd, n, P, C, eps, as_stream(stream));
}

extern "C" int midas_groupnorm_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     const float* residual, float* y, void* out_hi, void* out_lo, int n, int H, int W, int C,
                                     int plane_h, int plane_w, int relu, float split_scale, int32_t* range_flag, void* stream) {
    if (!x || !mean || !rstd || !gamma || !beta || n <= 0 || H <= 0 || W <= 0 || C <= 0 || (!y && !out_hi)) return FRESCO_EINVAL;
    if (!md_planes_ok(out_hi, out_lo, split_scale)) return FRESCO_EINVAL;
    if (out_hi && (plane_h < H || plane_w < W)) return FRESCO_EINVAL;
    if (!md_gn_channels(C)) return FRESCO_EUNSUPPORTED;
    if ((int64_t)n * H * W >= (int64_t)1 << 31 || (out_hi && (int64_t)n * plane_h * plane_w >= (int64_t)1 << 31))
        return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(gamma, 16) || !aligned_to(beta, 16) || !aligned_to(residual, 16) || !aligned_to(y, 16))
        return FRESCO_EINVAL;
    const int64_t total = (int64_t)n * H * W * (C / 4);
    hipLaunchKernelGGL(midas_gn_apply_kernel, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), x, mean, rstd, gamma,
                       beta, residual, y, static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), total, H, W, C, plane_h,
                       plane_w, relu ? 1 : 0, split_scale, range_flag);
    return check_launch();
}

extern "C" int midas_pool(const float* x, float* out, void* out_hi, void* out_lo, int n, int H, int W, int C, float split_scale,
                          int32_t* range_flag, void* stream) {
    if (!x || !out_hi || !out_lo || n <= 0 || H <= 0 || W <= 0 || C <= 0 || !(split_scale > 0.f)) return FRESCO_EINVAL;
    if (C != 64 || H % 2 || W % 2) return FRESCO_EUNSUPPORTED;
    if ((int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(out, 16) || !aligned_to(out_hi, 8) || !aligned_to(out_lo, 8)) return FRESCO_EINVAL;
    const int OH = H / 2, OW = W / 2;
    const int64_t total = (int64_t)n * OH * OW * (C / 4);
    hipLaunchKernelGGL(pool3s2_kernel<0>, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), x, out,
                       static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), total, H, W, OH, OW, split_scale, range_flag);
    return check_launch();
}

extern "C" int midas_layernorm(const float* x, const float* gamma, const float* beta, float* y, void* out_hi, void* out_lo,
                               int64_t M, int C, float eps, float split_scale, int32_t* range_flag, void* stream) {
    if (!x || !gamma || !beta || M <= 0 || C <= 0 || (!y && !out_hi) || !(eps >= 0.f)) return FRESCO_EINVAL;
    if (!md_planes_ok(out_hi, out_lo, split_scale)) return FRESCO_EINVAL;
    if (C % 4 || C > 64 * 4 * MD_LN_MAXQ) return FRESCO_EUNSUPPORTED;
    if ((M + 3) / 4 > 0x7fffffff) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(gamma, 16) || !aligned_to(beta, 16) || !aligned_to(y, 16)) return FRESCO_EINVAL;
    hipLaunchKernelGGL(midas_layernorm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, as_stream(stream), x, gamma, beta, y,
                       static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), M, C, eps, out_hi ? split_scale : 1.f,
                       range_flag);
    return check_launch();
}

extern "C" int midas_tokens(const float* grid, const float* cls, const float* pos, float* out, int n, int L, int C,
                            void* stream) {
    if (!grid || !cls || !pos || !out || n <= 0 || L < 2 || C <= 0) return FRESCO_EINVAL;
    if (C % 4) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(grid, 16) || !aligned_to(cls, 16) || !aligned_to(pos, 16) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    const int64_t total = (int64_t)n * L * (C / 4);
    hipLaunchKernelGGL(midas_tokens_kernel, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), grid, cls, pos, out,
                       total, L, C);
    return check_launch();
}

extern "C" int midas_head_merge(const float* x, float* out, void* out_hi, void* out_lo, int n, int L, int heads,
                                float split_scale, int32_t* range_flag, void* stream) {
    if (!x || n <= 0 || L <= 0 || heads <= 0 || (!out && !out_hi)) return FRESCO_EINVAL;
    if (!md_planes_ok(out_hi, out_lo, split_scale)) return FRESCO_EINVAL;
    if (!aligned_to(x, 16) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    const int64_t total = (int64_t)n * L * heads * 16;
    hipLaunchKernelGGL(midas_head_merge_kernel, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), x, out,
                       static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), total, n, L, heads,
                       out_hi ? split_scale : 1.f, range_flag);
    return check_launch();
}

extern "C" int midas_rowbias_gelu(const float* x, const float* rowbias, float* out, void* out_hi, void* out_lo, int64_t M,
                                  int C, int rows_per_img, float split_scale, int32_t* range_flag, void* stream) {
    if (!x || !rowbias || M <= 0 || C <= 0 || rows_per_img <= 0 || (!out && !out_hi)) return FRESCO_EINVAL;
    if (!md_planes_ok(out_hi, out_lo, split_scale)) return FRESCO_EINVAL;
    if (C % 4) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(rowbias, 16) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    const int64_t total = M * (C / 4);
    hipLaunchKernelGGL(midas_rowbias_gelu_kernel, dim3(stream_blocks(total)), dim3(256), 0, as_stream(stream), x, rowbias, out,
                       static_cast<half_t*>(out_hi), static_cast<half_t*>(out_lo), total, C, rows_per_img,
                       out_hi ? split_scale : 1.f, range_flag);
    return check_launch();
}

extern "C" size_t midas_tail_workspace_bytes(int n, int H, int W) {
    if (n <= 0 || H < 2 || W < 2 || (int64_t)n * H * W >= (int64_t)1 << 31) return 0;
    return (size_t)n * MD_MM_BLOCKS * 2 * sizeof(float);
}

extern "C" int midas_tail(const float* depth, uint8_t* depth_image, uint8_t* normal_image, void* cond, int cond_dtype,
                          void* workspace, size_t workspace_bytes, int n, int H, int W, float a, float bg_th, void* stream) {
    if (!depth || !depth_image || !normal_image || !workspace || n <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (cond && cond_dtype != FRESCO_F16 && cond_dtype != FRESCO_BF16 && cond_dtype != FRESCO_F32) return FRESCO_EINVAL;
    if (H < 2 || W < 2 || n > 65535 || (int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(depth, 4) || !aligned_to(workspace, 4) || !aligned_to(cond, cond_dtype == FRESCO_F32 ? 4 : 2))
        return FRESCO_EINVAL;
    if (workspace_bytes < midas_tail_workspace_bytes(n, H, W)) return FRESCO_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(midas_minmax_kernel, dim3(MD_MM_BLOCKS, n), dim3(256), 0, st, depth, part, H * W);
    if (int rc = check_launch()) return rc;
    const dim3 grid((unsigned)stream_blocks((int64_t)H * W), n);
    if (cond && cond_dtype == FRESCO_F16)
        hipLaunchKernelGGL(midas_tail_kernel<half_t>, grid, dim3(256), 0, st, depth, part, depth_image, normal_image,
                           static_cast<half_t*>(cond), H, W, a, bg_th);
    else if (cond && cond_dtype == FRESCO_BF16)
        hipLaunchKernelGGL(midas_tail_kernel<bf16_t>, grid, dim3(256), 0, st, depth, part, depth_image, normal_image,
                           static_cast<bf16_t*>(cond), H, W, a, bg_th);
    else
        hipLaunchKernelGGL(midas_tail_kernel<float>, grid, dim3(256), 0, st, depth, part, depth_image, normal_image,
                           static_cast<float*>(cond), H, W, a, bg_th);
    return check_launch();
}
