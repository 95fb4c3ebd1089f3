// The 3 x 3 stride-2 max pool on 64-channel fp32 NHWC rows -> fp32 rows (optional) and (hi, lo) operand planes (always).
// egnet.hip and midas.hip include it; the output size is the launcher's rule.  Unnamed namespace: each file compiles its own
// instantiation under its own flags (groupnorm_stats.h says why).
#pragma once
#include "common.h"
#include "fn_split.h"

namespace fresco {
namespace {

// One thread per (output pixel, four channels): 16 threads per pixel.  The window of output (oy, ox) starts at input
// (2 oy + ORIGIN, 2 ox + ORIGIN) and is clipped to the map: what lies outside never wins (-inf), and every window holds at
// least one pixel of the map (the launcher's output size sees to that).  A NaN in a window never wins either (fmaxf), so it
// raises the range flag on its own: the planes stay finite and would be wrong without a word.
//   ORIGIN = -1: MaxPool2d(3, 2, padding 1, ceil_mode=True) (EGNet);  ORIGIN = 0: MaxPool2dSame(3, 2) at even sizes (MiDaS)
template <int ORIGIN>
__global__ __launch_bounds__(256) void pool3s2_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                      half_t* __restrict__ o_hi, half_t* __restrict__ o_lo, int64_t total, int H,
                                                      int W, int OH, int OW, float scale, int32_t* range_flag) {
    constexpr int C = 64, Q = C / 4;
    bool sat = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % Q) * 4;
        const int64_t p = idx / Q;
        const int ox = (int)(p % OW), oy = (int)((p / OW) % OH);
        const int64_t img = p / ((int64_t)OW * OH);
        float v[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy + ORIGIN + ky;
            if ((ORIGIN < 0 && iy < 0) || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox + ORIGIN + kx;
                if ((ORIGIN < 0 && ix < 0) || ix >= W) continue;
                const floatx4 t = *reinterpret_cast<const floatx4*>(x + ((img * H + iy) * W + ix) * C + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = fmaxf(v[e], t[e]);
                    sat |= t[e] != t[e];  // fmaxf drops a NaN: the maximum stays finite, so the flag has to say it
                }
            }
        }
        if (out) {
            const floatx4 t = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<floatx4*>(out + p * C + c) = t;
        }
        sat |= fn_split_store4(v, scale, o_hi, o_lo, p * C + c);
    }
    fn_flag_range(range_flag, sat);
}

}  // namespace
}  // namespace fresco
