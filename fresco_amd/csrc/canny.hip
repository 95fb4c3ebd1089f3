// The Canny annotator of the ControlNet condition (reference: src/ControlNet/annotator/canny/__init__.py, one
// cv2.Canny(img, low, high) per frame on the host), batched over frames on the device.  The arithmetic is OpenCV's generic
// path for an 8-bit 3-channel image, aperture 3, L1 magnitude -- all integer; DESIGN.md section 14 has the rules.
//
//   canny_classify_kernel  one tiled pass: RGB tile + 2-pixel replicate halo in LDS -> Sobel and the channel choice on the
//                          tile + 1-pixel halo (zero magnitude outside the frame) -> non-maximum suppression -> class byte
//   hysteresis, union-find labelling in four launches whatever the picture (no host loop, no workgroup waits for another):
//   canny_tile_union_kernel    per tile, in LDS: union over the backward neighbours (W, NW, N, NE) inside the tile,
//                              then parent[p] = the tile-local root as a global index, flag[p] = 0
//   canny_border_union_kernel  the pixels of a tile's first row, first and last column: union with the backward neighbours
//                              in global memory (atomicMin at agent scope)
//   canny_seed_kernel          every strong pixel: flag[find(p)] = 1
//   canny_emit_kernel          out = cls && flag[find(p)] ? 255 : 0, and the condition
//
// parent[p] <= p always (labels only decrease), so every chain of parents ends; every loop below carries a hard bound on top
// of that (the tile's pixel count in LDS, n H W in global memory): a defect gives a wrong picture, never a kernel that does
// not return.
// Built with -ffp-contract=off: the condition follows the torch operation order, as in hed.hip.
#include "common.h"

namespace fresco {

constexpr int CANNY_T = 32;                        // tile side
constexpr int CANNY_TP = CANNY_T * CANNY_T;        // pixels per tile
constexpr int CANNY_RGB = CANNY_T + 4;             // tile + 2-pixel halo
constexpr int CANNY_MAG = CANNY_T + 2;             // tile + 1-pixel halo
constexpr int CANNY_MAX_BLOCKS = 1 << 20;          // grid cap: workgroups walk the tiles (pixels) with a stride
constexpr int CANNY_BORDER = 3 * CANNY_T - 2;      // border pixels of a tile: first row, first and last column

struct CannyTiles {
    int tx, ty;         // tiles per row, per column of one frame
    int64_t total;      // n tx ty
};

static inline CannyTiles canny_tiles(int n, int H, int W) {
    CannyTiles t;
    t.tx = (W + CANNY_T - 1) / CANNY_T;
    t.ty = (H + CANNY_T - 1) / CANNY_T;
    t.total = (int64_t)n * t.tx * t.ty;
    return t;
}

__device__ __forceinline__ int canny_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// (dx, dy) of one pixel in one word: both within +-1020
__device__ __forceinline__ int canny_pack(int dx, int dy) { return (int)(((unsigned)dy << 16) | ((unsigned)dx & 0xffffu)); }
__device__ __forceinline__ int canny_dx(int g) { return (int)(short)(g & 0xffff); }
__device__ __forceinline__ int canny_dy(int g) { return g >> 16; }
__device__ __forceinline__ int canny_mag(int g) { return abs(canny_dx(g)) + abs(canny_dy(g)); }

__global__ __launch_bounds__(256) void canny_classify_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ cls,
                                                             CannyTiles tl, int H, int W, int low, int high) {
    __shared__ uint8_t rgb[CANNY_RGB * CANNY_RGB * 3];
    __shared__ int grad[CANNY_MAG * CANNY_MAG];
    const int t = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < tl.total; tile += gridDim.x) {
        const int f = (int)(tile / (tl.tx * tl.ty)), r = (int)(tile - (int64_t)f * (tl.tx * tl.ty));
        const int y0 = (r / tl.tx) * CANNY_T, x0 = (r % tl.tx) * CANNY_T;
        const uint8_t* src = frames + (int64_t)f * H * W * 3;
        // the tile and two pixels around it, coordinates clamped to the frame (BORDER_REPLICATE)
        for (int i = t; i < CANNY_RGB * CANNY_RGB; i += 256) {
            const int ly = i / CANNY_RGB, lx = i - ly * CANNY_RGB;
            const int gy = canny_clamp(y0 - 2 + ly, H - 1), gx = canny_clamp(x0 - 2 + lx, W - 1);
            const uint8_t* p = src + ((int64_t)gy * W + gx) * 3;
            rgb[i * 3 + 0] = p[0];
            rgb[i * 3 + 1] = p[1];
            rgb[i * 3 + 2] = p[2];
        }
        __syncthreads();
        // Sobel per channel on the tile and one pixel around it; the channel of the largest |dx| + |dy|, the first on ties;
        // outside the frame the magnitude is zero, not replicated
        for (int i = t; i < CANNY_MAG * CANNY_MAG; i += 256) {
            const int hy = i / CANNY_MAG, hx = i - hy * CANNY_MAG;
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
            int g = 0;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const uint8_t* r0 = rgb + (hy * CANNY_RGB + hx) * 3;  // the pixel above left
                const uint8_t* r1 = r0 + CANNY_RGB * 3;
                const uint8_t* r2 = r1 + CANNY_RGB * 3;
                int best = -1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int a00 = r0[c], a01 = r0[3 + c], a02 = r0[6 + c];
                    const int a10 = r1[c], a12 = r1[6 + c];
                    const int a20 = r2[c], a21 = r2[3 + c], a22 = r2[6 + c];
                    const int dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
                    const int dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
                    const int m = abs(dx) + abs(dy);
                    if (m > best) {
                        best = m;
                        g = canny_pack(dx, dy);
                    }
                }
            }
            grad[i] = g;
        }
        __syncthreads();
        for (int i = t; i < CANNY_TP; i += 256) {
            const int ly = i / CANNY_T, lx = i - ly * CANNY_T;
            const int gy = y0 + ly, gx = x0 + lx;
            if (gy >= H || gx >= W) continue;
            const int* gc = grad + (ly + 1) * CANNY_MAG + (lx + 1);
            const int g = *gc, m = canny_mag(g);
            uint8_t k = 0;
            if (m > low) {
                const int dx = canny_dx(g), dy = canny_dy(g);
                const int x = abs(dx), y = abs(dy) << 15;
                const int t22 = x * 13573, t67 = t22 + (x << 16);
                bool keep;
                if (y < t22)
                    keep = m > canny_mag(gc[-1]) && m >= canny_mag(gc[1]);
                else if (y > t67)
                    keep = m > canny_mag(gc[-CANNY_MAG]) && m >= canny_mag(gc[CANNY_MAG]);
                else {
                    const int s = (dx ^ dy) < 0 ? -1 : 1;
                    keep = m > canny_mag(gc[-CANNY_MAG - s]) && m > canny_mag(gc[CANNY_MAG + s]);
                }
                if (keep) k = m > high ? 2 : 1;
            }
            cls[((int64_t)f * H + gy) * W + gx] = k;
        }
        __syncthreads();  // the next tile of this workgroup overwrites rgb / grad
    }
}

__device__ __forceinline__ int canny_class(uint8_t b) { return b <= 2 ? (int)b : 0; }

// ---- union-find in LDS (workgroup scope): L[i] <= i
__device__ __forceinline__ int lds_get(int* L, int i) {
    return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int lds_find(int* L, int a) {
    for (int it = 0; it < CANNY_TP; ++it) {
        const int p = lds_get(L, a);
        if (p == a) break;
        a = p;
    }
    return a;
}

__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    for (int it = 0; it < CANNY_TP; ++it) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        // a > b: hang a under b if a is still a root; otherwise go on from what a hangs under now
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void canny_tile_union_kernel(const uint8_t* __restrict__ cls, int32_t* __restrict__ parent,
                                                               uint8_t* __restrict__ flag, CannyTiles tl, int H, int W) {
    __shared__ uint8_t C[CANNY_TP];
    __shared__ int L[CANNY_TP];
    const int t = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < tl.total; tile += gridDim.x) {
        const int f = (int)(tile / (tl.tx * tl.ty)), r = (int)(tile - (int64_t)f * (tl.tx * tl.ty));
        const int y0 = (r / tl.tx) * CANNY_T, x0 = (r % tl.tx) * CANNY_T;
        const int64_t base = (int64_t)f * H * W;
        for (int i = t; i < CANNY_TP; i += 256) {
            const int ly = i / CANNY_T, lx = i - ly * CANNY_T;
            const int gy = y0 + ly, gx = x0 + lx;
            C[i] = (gy < H && gx < W) ? (uint8_t)canny_class(cls[base + (int64_t)gy * W + gx]) : (uint8_t)0;
            L[i] = i;
        }
        __syncthreads();
        // N is a neighbour of NW, NE and W, which their own turns join to it; NW is the N of W
        for (int i = t; i < CANNY_TP; i += 256) {
            if (!C[i]) continue;
            const int ly = i / CANNY_T, lx = i - ly * CANNY_T;
            if (ly > 0 && C[i - CANNY_T]) {
                lds_union(L, i, i - CANNY_T);
                continue;
            }
            if (ly > 0 && lx + 1 < CANNY_T && C[i - CANNY_T + 1]) lds_union(L, i, i - CANNY_T + 1);
            if (ly > 0 && lx > 0 && C[i - CANNY_T - 1])
                lds_union(L, i, i - CANNY_T - 1);
            else if (lx > 0 && C[i - 1])
                lds_union(L, i, i - 1);
        }
        __syncthreads();
        for (int i = t; i < CANNY_TP; i += 256) {
            const int ly = i / CANNY_T, lx = i - ly * CANNY_T;
            const int gy = y0 + ly, gx = x0 + lx;
            if (gy >= H || gx >= W) continue;
            const int root = lds_find(L, i);  // (nothing writes L any more)
            const int ry = root / CANNY_T, rx = root - ry * CANNY_T;
            const int64_t p = base + (int64_t)gy * W + gx;
            parent[p] = (int32_t)(base + (int64_t)(y0 + ry) * W + (x0 + rx));
            flag[p] = 0;
        }
        __syncthreads();  // the next tile of this workgroup overwrites C / L
    }
}

// ---- union-find in global memory (agent scope).  The L2 of another XCD may hold an older parent: the loads bypass L1 and,
// whatever a find has read, a link is made only by an atomicMin that found its node still a root -- the value it returns is
// current, and the loop goes on from it otherwise.
__device__ __forceinline__ int32_t glb_get(int32_t* P, int32_t i) {
    return __hip_atomic_load(P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t glb_find(int32_t* P, int32_t a, uint32_t bound) {
    for (uint32_t it = 0; it < bound; ++it) {
        const int32_t p = glb_get(P, a);
        if (p == a) break;
        a = p;
    }
    return a;
}

__device__ __forceinline__ void glb_union(int32_t* P, int32_t a, int32_t b, uint32_t bound) {
    for (uint32_t it = 0; it < bound; ++it) {
        a = glb_find(P, a, bound);
        b = glb_find(P, b, bound);
        if (a == b) return;
        if (a < b) {
            const int32_t s = a;
            a = b;
            b = s;
        }
        const int32_t old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// 128 threads per tile, one per border pixel: the first row (0 .. T-1), the first column below it, the last column below it
__global__ __launch_bounds__(128) void canny_border_union_kernel(const uint8_t* __restrict__ cls, int32_t* parent, CannyTiles tl,
                                                                 int H, int W, uint32_t total) {
    const int t = threadIdx.x;
    if (t >= CANNY_BORDER) return;  // (no barrier below)
    int ly, lx;
    if (t < CANNY_T) {
        ly = 0;
        lx = t;
    } else if (t < 2 * CANNY_T - 1) {
        ly = t - CANNY_T + 1;
        lx = 0;
    } else {
        ly = t - 2 * CANNY_T + 2;
        lx = CANNY_T - 1;
    }
    for (int64_t tile = blockIdx.x; tile < tl.total; tile += gridDim.x) {
        const int f = (int)(tile / (tl.tx * tl.ty)), r = (int)(tile - (int64_t)f * (tl.tx * tl.ty));
        const int gy = (r / tl.tx) * CANNY_T + ly, gx = (r % tl.tx) * CANNY_T + lx;
        if (gy >= H || gx >= W) continue;
        const int64_t base = (int64_t)f * H * W;
        const int64_t p = base + (int64_t)gy * W + gx;
        if (!canny_class(cls[p])) continue;
        // the four backward neighbours inside the frame (a frame's first row has none above: frames stay apart); those in
        // this tile are joined already and cost two finds
        if (gx > 0 && canny_class(cls[p - 1])) glb_union(parent, (int32_t)p, (int32_t)(p - 1), total);
        if (gy > 0) {
            const int64_t q = p - W;
            if (gx > 0 && canny_class(cls[q - 1])) glb_union(parent, (int32_t)p, (int32_t)(q - 1), total);
            if (canny_class(cls[q])) glb_union(parent, (int32_t)p, (int32_t)q, total);
            if (gx + 1 < W && canny_class(cls[q + 1])) glb_union(parent, (int32_t)p, (int32_t)(q + 1), total);
        }
    }
}

// parent is read-only from here on (the launch boundary made the border pass's links visible): plain loads
__device__ __forceinline__ int32_t ro_find(const int32_t* __restrict__ P, int32_t a, uint32_t bound) {
    for (uint32_t it = 0; it < bound; ++it) {
        const int32_t p = P[a];
        if (p == a) break;
        a = p;
    }
    return a;
}

__global__ __launch_bounds__(256) void canny_seed_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ parent,
                                                         uint8_t* flag, uint32_t total) {
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u)
        if (cls[idx] == 2) flag[ro_find(parent, (int32_t)idx, total)] = 1;  // the same byte from every writer
}

// One thread per pixel.  T: element type of the optional condition.
template <typename T>
__global__ __launch_bounds__(256) void canny_emit_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ parent,
                                                         const uint8_t* __restrict__ flag, uint8_t* __restrict__ out,
                                                         T* __restrict__ cond, uint32_t total, uint32_t HW) {
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        uint8_t u = 0;
        if (canny_class(cls[idx]) && flag[ro_find(parent, (int32_t)idx, total)]) u = 255;
        out[idx] = u;
        if (cond) {
            // numpy2tensor(u) * 0.5 + 0.5 in PyTorch's fp32 order on the device, as hed_fuse_kernel writes it
            const float c = (((float)u * (1.f / 255.f)) * 2.f - 1.f) * 0.5f + 0.5f;
            const uint32_t img = idx / HW, r = idx - img * HW;
            T* o = cond + ((int64_t)img * 3 * HW + r);
            const T cv = (T)c;
            o[0] = cv;
            o[HW] = cv;
            o[2 * (int64_t)HW] = cv;
        }
    }
}

// (not common.h's stream_blocks: this caps a count of blocks at 2^20, that one a count of threads at 2048 blocks)
static inline int canny_blocks(int64_t want) { return (int)(want < CANNY_MAX_BLOCKS ? want : CANNY_MAX_BLOCKS); }

// n H W when the calls take the size, else 0
static inline int64_t canny_pixels(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t npix = (int64_t)n * H * W;
    return npix >= (int64_t)1 << 31 ? 0 : npix;
}

}  // namespace fresco

using namespace fresco;

extern "C" size_t fresco_canny_workspace_bytes(int n, int H, int W) {
    const int64_t npix = canny_pixels(n, H, W);
    if (!npix) return 0;
    return align_up((size_t)npix * sizeof(int32_t), 256) + align_up((size_t)npix, 256);  // parent, flag
}

extern "C" int fresco_canny_classify(const uint8_t* frames, uint8_t* cls, int n, int H, int W, int low, int high,
                                     void* stream) {
    if (!frames || !cls || n <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (!canny_pixels(n, H, W)) return FRESCO_EUNSUPPORTED;
    if (low > high) {
        const int s = low;
        low = high;
        high = s;
    }
    const CannyTiles tl = canny_tiles(n, H, W);
    hipLaunchKernelGGL(canny_classify_kernel, dim3(canny_blocks(tl.total)), dim3(256), 0, as_stream(stream), frames, cls, tl, H,
                       W, low, high);
    return check_launch();
}

extern "C" int fresco_canny_hysteresis(const uint8_t* cls, uint8_t* out, void* cond, int cond_dtype, void* workspace,
                                       size_t workspace_bytes, int n, int H, int W, void* stream) {
    if (!cls || !out || !workspace || n <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (cond && cond_dtype != FRESCO_F16 && cond_dtype != FRESCO_BF16 && cond_dtype != FRESCO_F32) return FRESCO_EINVAL;
    if (!aligned_to(workspace, 4) || !aligned_to(cond, cond_dtype == FRESCO_F32 ? 4 : 2)) return FRESCO_EINVAL;
    const int64_t npix = canny_pixels(n, H, W);
    if (!npix) return FRESCO_EUNSUPPORTED;
    if (workspace_bytes < fresco_canny_workspace_bytes(n, H, W)) return FRESCO_EWORKSPACE;
    char* ws = static_cast<char*>(workspace);
    int32_t* parent = carve<int32_t>(ws, (size_t)npix);
    uint8_t* flag = carve<uint8_t>(ws, (size_t)npix);
    const CannyTiles tl = canny_tiles(n, H, W);
    const uint32_t total = (uint32_t)npix, HW = (uint32_t)H * (uint32_t)W;
    const dim3 tiles(canny_blocks(tl.total)), pixels(canny_blocks((npix + 255) / 256));
    hipStream_t st = as_stream(stream);
    int rc;
    hipLaunchKernelGGL(canny_tile_union_kernel, tiles, dim3(256), 0, st, cls, parent, flag, tl, H, W);
    if ((rc = check_launch()) != FRESCO_OK) return rc;
    hipLaunchKernelGGL(canny_border_union_kernel, tiles, dim3(128), 0, st, cls, parent, tl, H, W, total);
    if ((rc = check_launch()) != FRESCO_OK) return rc;
    hipLaunchKernelGGL(canny_seed_kernel, pixels, dim3(256), 0, st, cls, (const int32_t*)parent, flag, total);
    if ((rc = check_launch()) != FRESCO_OK) return rc;
    if (cond && cond_dtype == FRESCO_F16)
        hipLaunchKernelGGL(canny_emit_kernel<half_t>, pixels, dim3(256), 0, st, cls, (const int32_t*)parent,
                           (const uint8_t*)flag, out, static_cast<half_t*>(cond), total, HW);
    else if (cond && cond_dtype == FRESCO_BF16)
        hipLaunchKernelGGL(canny_emit_kernel<bf16_t>, pixels, dim3(256), 0, st, cls, (const int32_t*)parent,
                           (const uint8_t*)flag, out, static_cast<bf16_t*>(cond), total, HW);
    else
        hipLaunchKernelGGL(canny_emit_kernel<float>, pixels, dim3(256), 0, st, cls, (const int32_t*)parent,
                           (const uint8_t*)flag, out, static_cast<float*>(cond), total, HW);
    return check_launch();
}
