// Bilinear flow sampling and forward_backward_consistency_check (gmflow/geometry.py:41-96) at one pixel, fp32 and
// not contracted.  Shared by warp.hip (fresco_flow_occlusion) and flowcalc.hip (fresco_flowcalc_output), so the two
// entry points give the same bits by construction.  Planes may be windows of a wider field: `ld` is the row stride of
// the sampled planes, (w, h) the window's own size.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cmath>

#include <hip/hip_runtime.h>

namespace fresco {

struct Taps {
    int i00, i01, i10, i11;
    float w00, w01, w10, w11;
};

// geometry.py:50-55,65-72: grid = pixel + flow, normalised 2*x/(w-1)-1, grid_sample(align_corners=True)
// maps back with ((g+1)/2)*(size-1); zeros padding -> out-of-range taps get weight 0.
__device__ __forceinline__ Taps make_taps(float fx, float fy, int x, int y, int h, int w, int ld) {
#pragma clang fp contract(off)
    const float gx = 2.f * ((float)x + fx) / (float)(w - 1) - 1.f;
    const float gy = 2.f * ((float)y + fy) / (float)(h - 1) - 1.f;
    const float ix = ((gx + 1.f) / 2.f) * (float)(w - 1);
    const float iy = ((gy + 1.f) / 2.f) * (float)(h - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float tx = ix - x0f, ty = iy - y0f;
    // clamp before the int conversion so that huge / non-finite coordinates stay defined
    const float x0c = fminf(fmaxf(x0f, -2.f), (float)w + 1.f);
    const float y0c = fminf(fmaxf(y0f, -2.f), (float)h + 1.f);
    const int x0 = (int)x0c, y0 = (int)y0c, x1 = x0 + 1, y1 = y0 + 1;
    const bool vx0 = x0 >= 0 && x0 < w && x0f == x0c, vx1 = x1 >= 0 && x1 < w && x0f == x0c;
    const bool vy0 = y0 >= 0 && y0 < h && y0f == y0c, vy1 = y1 >= 0 && y1 < h && y0f == y0c;
    const int cx0 = min(max(x0, 0), w - 1), cx1 = min(max(x1, 0), w - 1);
    const int cy0 = min(max(y0, 0), h - 1), cy1 = min(max(y1, 0), h - 1);
    Taps t;
    t.i00 = cy0 * ld + cx0;
    t.i01 = cy0 * ld + cx1;
    t.i10 = cy1 * ld + cx0;
    t.i11 = cy1 * ld + cx1;
    t.w00 = (vx0 && vy0) ? (1.f - tx) * (1.f - ty) : 0.f;
    t.w01 = (vx1 && vy0) ? tx * (1.f - ty) : 0.f;
    t.w10 = (vx0 && vy1) ? (1.f - tx) * ty : 0.f;
    t.w11 = (vx1 && vy1) ? tx * ty : 0.f;
    return t;
}

__device__ __forceinline__ Taps make_taps(float fx, float fy, int x, int y, int h, int w) {
    return make_taps(fx, fy, x, y, h, w, w);
}

__device__ __forceinline__ float sample(const float* __restrict__ plane, const Taps& t) {
#pragma clang fp contract(off)
    return plane[t.i00] * t.w00 + plane[t.i01] * t.w01 + plane[t.i10] * t.w10 + plane[t.i11] * t.w11;
}

// forward_backward_consistency_check at pixel (x, y) of the fields f (fwd) and b (bwd): x planes at f / b, y planes
// `plane` floats further, rows `ld` apart.
//   occ_f = |fwd + warp(bwd, fwd)| > alpha (|fwd| + |bwd|) + beta,  occ_b = |bwd + warp(fwd, bwd)| > (same)
// The two tap sets are returned for callers that sample more planes at the same points.
struct FbCheck {
    Taps tf, tb;
    bool occ_f, occ_b;
};

__device__ __forceinline__ FbCheck fb_check(const float* __restrict__ f, const float* __restrict__ b, size_t plane,
                                            int ld, int x, int y, int h, int w, float alpha, float beta) {
#pragma clang fp contract(off)
    const size_t p = size_t(y) * ld + x;
    const float fx = f[p], fy = f[plane + p], bx = b[p], by = b[plane + p];
    const float mag = sqrtf(fx * fx + fy * fy) + sqrtf(bx * bx + by * by);
    const float thr = alpha * mag + beta;
    FbCheck r;
    r.tf = make_taps(fx, fy, x, y, h, w, ld);
    r.tb = make_taps(bx, by, x, y, h, w, ld);
    const float dfx = fx + sample(b, r.tf), dfy = fy + sample(b + plane, r.tf);
    const float dbx = bx + sample(f, r.tb), dby = by + sample(f + plane, r.tb);
    r.occ_f = sqrtf(dfx * dfx + dfy * dfy) > thr;
    r.occ_b = sqrtf(dbx * dbx + dby * dby) > thr;
    return r;
}

}  // namespace fresco
