// grid_sample(nearest, zeros, align_corners=True) at pixel + flow, as FRESCO's flow_utils.py runs it (coords_grid +
// flow, then bilinear_sample's normalise to [-1, 1]) and ATen's CPU grid sampler unnormalises it again: fp32 throughout,
// not contracted, rounded half to even.  Shared by blend.hip (the mask warp) and guides.hip (the image warp).
#pragma once

#include <cstddef>
#include <cmath>

#include <hip/hip_runtime.h>

namespace fresco {

// Source pixel index of (x, y) under `flow` ((2, h, w), x plane first), or -1 where the sample falls outside the image
// (NaN included): the zeros padding.
__device__ __forceinline__ long long nearest_source(const float* flow, int x, int y, int w, int h) {
#pragma clang fp contract(off)
    const size_t q = size_t(y) * w + x;
    const float cx = float(x) + flow[q], cy = float(y) + flow[size_t(w) * h + q];
    const float gx = 2.0f * cx / float(w - 1) - 1.0f, gy = 2.0f * cy / float(h - 1) - 1.0f;
    const float ix = rintf((gx + 1.0f) * (float(w - 1) / 2.0f)), iy = rintf((gy + 1.0f) * (float(h - 1) / 2.0f));
    if (!(ix >= 0.0f && ix < float(w) && iy >= 0.0f && iy < float(h))) return -1;
    return (long long)(size_t(iy) * w + size_t(ix));
}

// one-channel form: the warped byte of `prev`
__device__ __forceinline__ uint8_t warp_nearest(const uint8_t* prev, const float* flow, int x, int y, int w, int h) {
    const long long s = nearest_source(flow, x, y, w, h);
    return s < 0 ? 0 : prev[s];
}

}  // namespace fresco
