// The guide images FRESCO's video_blend.py hands to Ebsynth (src/ebsynth/blender/guide.py), batched over n uint8
// images of (h, w, c), written for gfx950 from their description; DESIGN.md section 9.
//   edge : cv2.filter2D(img, -1, [[0,-1,0],[-1,4,-1],[0,-1,0]]): per-channel correlation, BORDER_REFLECT_101,
//          saturated to [0, 255]; the sums are exact integers
//   warp : flow_calc.warp(img, flow, 'nearest') of a uint8 image (warp_nearest.h), zeros outside
// One launch each, one thread per pixel, the image index in blockIdx.z.
#include "common.h"
#include "warp_nearest.h"

namespace fresco {
namespace {

constexpr int kGuideBlock = 16;
constexpr int kGuideMaxBatch = 65535;  // grid z
constexpr int kGuideMaxChannels = 16;

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(256) void guide_edge(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int w,
                                                  int h, int c) {
    const int x = blockIdx.x * kGuideBlock + threadIdx.x, y = blockIdx.y * kGuideBlock + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t img = size_t(blockIdx.z) * w * h * c;
    in += img;
    out += img;
    const size_t row = size_t(y) * w, up = size_t(reflect101(y - 1, h)) * w, dn = size_t(reflect101(y + 1, h)) * w;
    const int xl = reflect101(x - 1, w), xr = reflect101(x + 1, w);
    for (int k = 0; k < c; ++k) {
        const int v = 4 * int(in[(row + x) * c + k]) - int(in[(up + x) * c + k]) - int(in[(dn + x) * c + k]) -
                      int(in[(row + xl) * c + k]) - int(in[(row + xr) * c + k]);
        out[(row + x) * c + k] = uint8_t(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

__global__ __launch_bounds__(256) void guide_warp_nearest(const uint8_t* __restrict__ in, const float* __restrict__ flow,
                                                          uint8_t* __restrict__ out, int w, int h, int c) {
    const int x = blockIdx.x * kGuideBlock + threadIdx.x, y = blockIdx.y * kGuideBlock + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t b = blockIdx.z, hw = size_t(w) * h;
    in += b * hw * c;
    out += b * hw * c;
    flow += b * 2 * hw;
    const long long s = nearest_source(flow, x, y, w, h);
    const size_t q = size_t(y) * w + x;
    for (int k = 0; k < c; ++k) out[q * c + k] = s < 0 ? uint8_t(0) : in[size_t(s) * c + k];
}

int guide_args(const void* in, const void* out, int n, int w, int h, int c) {
    if (!in || !out || in == out || n < 1 || w < 1 || h < 1 || c < 1) return FRESCO_EINVAL;
    if (n > kGuideMaxBatch || c > kGuideMaxChannels || w < 2 || h < 2) return FRESCO_EUNSUPPORTED;
    return FRESCO_OK;
}

dim3 guide_grid(int w, int h, int n) {
    return dim3((w + kGuideBlock - 1) / kGuideBlock, (h + kGuideBlock - 1) / kGuideBlock, n);
}

}  // namespace
}  // namespace fresco

extern "C" int fresco_edge_guide(const uint8_t* img, uint8_t* out, int n, int w, int h, int c, void* stream) {
    using namespace fresco;
    const int rc = guide_args(img, out, n, w, h, c);
    if (rc != FRESCO_OK) return rc;
    guide_edge<<<guide_grid(w, h, n), dim3(kGuideBlock, kGuideBlock), 0, as_stream(stream)>>>(img, out, w, h, c);
    return check_launch();
}

extern "C" int fresco_warp_nearest(const uint8_t* img, const float* flow, uint8_t* out, int n, int w, int h, int c,
                                   void* stream) {
    using namespace fresco;
    const int rc = guide_args(img, out, n, w, h, c);
    if (rc != FRESCO_OK) return rc;
    if (!flow) return FRESCO_EINVAL;
    guide_warp_nearest<<<guide_grid(w, h, n), dim3(kGuideBlock, kGuideBlock), 0, as_stream(stream)>>>(img, flow, out,
                                                                                                      w, h, c);
    return check_launch();
}
