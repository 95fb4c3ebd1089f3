// What a UNet ResnetBlock2D of fp16 pipelines needs beside vae.hip's convolution: include/fresco_unet.h, DESIGN.md section 19.
//
//   unet_gn_lds_kernel      GroupNorm(32) [+ SiLU] of x + addend in ONE launch and ONE read of x: the plane waits in LDS
//   unet_gn_stats_kernel / unet_gn_finish_kernel / unet_gn_apply_kernel
//                           the same in three launches where the plane does not fit: fp64 partial sums per 64 pixels, added
//                           in chunk order, then the apply pass (x is read twice)
//   unet_temb_kernel        out = bias + conv_bias + W SiLU(temb): one wave per output channel, all images at once
//
// WIDTHS.  C is a multiple of 64 (64 .. 2560), so a group is cpg = C / 32 channels, an even number of them: a PAIR of
// channels (2 c, 2 c + 1) never straddles two groups, but a 16-byte piece (8 channels) may: at C = 320 a group is 20 bytes.
// Every thread of the three GroupNorm kernels owns ONE piece COLUMN for its whole life (thread t: column t % ncols, rows
// t / ncols, t / ncols + 512 / ncols, ...; the threads beyond (512 / ncols) ncols idle), so the group of each of its four
// pairs, its addend, gamma and beta are fixed registers, and it keeps one fp64 (sum, sum of squares) per pair.
//
// SUMMATION ORDER (fixed; no atomics): a thread adds its rows in row order; the 512 x 4 pair sums go to LDS (32 KiB,
// static) and are folded in four short steps, each by many threads and each in index order, in place: (1a) per (column,
// pair) the row slots s, s + S, .. of each of S interleaved sub-ranges (S a power of two <= 16), (1b) per (column, pair) the
// S sub-ranges, (2a) per group eight interleaved shares of its pairs, (2b) per group the eight shares.  A single thread
// per sum (the first version) cost 102 + 20 dependent LDS reads at 8 x 8 and left the kernel at 10 us for 5 MB.  The
// three-launch form adds the chunks in chunk order in the finish kernel.
//
// THE LDS FORM.  Global reads must be aligned 16-byte pieces, so a workgroup takes a SLAB: the smallest run of G whole
// groups whose bytes are a multiple of 16 (G = 1, 2 or 4: C = 320: 4 groups = 80 bytes, 640: 2 = 80, 960: 4 = 240,
// 1280: 1 = 80, 1920: 2 = 240, 2560: 1 = 160), of ONE image: grid (32 / G, n).  Its plane is P x 2 G cpg bytes of dynamic
// LDS, written and read back by the same thread (no barrier for it; consecutive threads, consecutive 16 bytes).  The switch:
//   UG_LDS_PLANE_BYTES = 96 KiB: the LDS form runs where P x 2 G cpg <= 96 KiB.
// A CU has 160 KiB; beside the plane stand 32 KiB + 512 bytes + 256 bytes of static LDS (the pair sums, the group sums, mean
// and rstd).  96 KiB leaves the total at 128.75 KiB, holds every plane of the SD-1.5 UNet at 8 x 8, 16 x 16 (all six widths: at
// most 60 KiB) and 32 x 32 at 640 and 1280 (80 KiB), and one workgroup per CU is what any plane above 64 KiB leaves anyway.
// 32 x 32 at 960 and 1920 (240 KiB) and every 64 x 64 plane take the three-launch form.  Planes above 64 KiB - the static
// part go through common.h's allow_dyn_lds.
//
// THE THREE-LAUNCH FORM reads WHOLE rows (ncols = C / 8 <= 320 columns; a slab's 80-byte runs would split cache lines
// between workgroups): grid (chunks of UG_ROWS = 64 pixels, n) for the statistics and for the apply pass.
//
// unet_temb_kernel: 256 threads = four waves = four output channels.  K is walked in chunks of 512: a lane holds 8 weights
// of its channel (one 16-byte load, read ONCE), SiLU(temb) of 16 images x 512 k stands in LDS as fp32 (32 KiB, static) and
// is rebuilt per tile of 16 images under the same weights; a lane adds its 8 products in k order into one fp32 accumulator
// per image (64 registers), chunks in order, then a butterfly over the 64 lanes.
//
// The kernels' text stands in unet_body.h, once for both 16-bit element types, as templates over the element type; this
// file instantiates and launches the fp16 forms, net_bf16.hip the bf16 twins (x, y, temb and W bf16; everything else as here).
#include "common.h"
#include "unet_body.h"
#include "../../include/fresco_unet.h"

namespace fresco {

constexpr int UG_LDS_PLANE_BYTES = 96 * 1024;     // the switch between the two forms (header comment)
constexpr int UG_STATIC_LDS = 2 * UG_THREADS * 4 * 8 + 2 * UG_GROUPS * 8 + 2 * UG_GROUPS * 4;
constexpr int UG_MIN_WORKSPACE = 256;

// the fp16 instantiations of unet_body.h's kernels, under the names the launches below use
constexpr auto unet_gn_lds_kernel = unet_gn_lds_kernel_t<half_t>;
constexpr auto unet_gn_stats_kernel = unet_gn_stats_kernel_t<half_t>;
constexpr auto unet_gn_finish_kernel = unet_gn_finish_kernel_t<half_t>;
constexpr auto unet_gn_apply_kernel = unet_gn_apply_kernel_t<half_t>;
template <int TILES>
constexpr auto unet_temb_kernel = unet_temb_kernel_t<TILES, half_t>;


static inline bool ug_channels(int C) { return C >= 64 && C <= 2560 && C % 64 == 0; }

struct UgPlan {
    int cpg, G, sc, chunks;
    bool lds;
    int plane;
};

// the caller has checked n, P > 0 and ug_channels(C)
static inline UgPlan ug_plan(int P, int C) {
    UgPlan p;
    p.cpg = C / UG_GROUPS;
    p.G = p.cpg % 8 == 0 ? 1 : (p.cpg % 4 == 0 ? 2 : 4);  // the fewest groups whose 2 cpg G bytes are a multiple of 16
    p.sc = p.G * p.cpg;
    p.chunks = (P + UG_ROWS - 1) / UG_ROWS;
    const int64_t plane = (int64_t)P * p.sc * 2;
    p.lds = plane <= UG_LDS_PLANE_BYTES;
    p.plane = p.lds ? (int)plane : 0;
    return p;
}

static inline size_t ug_workspace(int n, int P, int C) {
    const UgPlan p = ug_plan(P, C);
    if (p.lds) return UG_MIN_WORKSPACE;
    return (size_t)n * p.chunks * UG_GROUPS * 2 * sizeof(double) + align_up((size_t)n * UG_GROUPS * 2 * sizeof(float), 256);
}

}  // namespace fresco

using namespace fresco;

extern "C" size_t unet_groupnorm_workspace_bytes(int n, int P, int C) {
    if (n <= 0 || P <= 0 || !ug_channels(C)) return 0;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return 0;
    return ug_workspace(n, P, C);
}

extern "C" int unet_groupnorm_lds_form(int n, int P, int C) {
    if (n <= 0 || P <= 0 || !ug_channels(C)) return -1;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return -1;
    return ug_plan(P, C).lds ? 1 : 0;
}

extern "C" int unet_groupnorm(const void* x, const float* addend, const float* gamma, const float* beta, void* y, void* workspace,
                              size_t workspace_bytes, int n, int P, int C, float eps, int silu, void* stream) {
    if (!x || !gamma || !beta || !y || !workspace || n <= 0 || P <= 0 || C <= 0 || !(eps >= 0.f)) return FRESCO_EINVAL;
    const int flags = silu;  // bit 0: SiLU, UNET_ELEM_BF16: x and y are bf16; no other bit
    if (flags & ~(1 | UNET_ELEM_BF16)) return FRESCO_EINVAL;
    if (!ug_channels(C)) return FRESCO_EUNSUPPORTED;
    if (n > 65535 || (int64_t)n * P >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(x, 16) || !aligned_to(y, 16) || !aligned_to(workspace, 8) || !aligned_to(gamma, 16) || !aligned_to(beta, 16) ||
        !aligned_to(addend, 16))
        return FRESCO_EINVAL;
    if (workspace_bytes < ug_workspace(n, P, C)) return FRESCO_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const UgPlan p = ug_plan(P, C);
    UgArgs a;
    a.x = x;
    a.addend = addend;
    a.gamma = gamma;
    a.beta = beta;
    a.y = y;
    a.part = nullptr;
    a.mean = a.rstd = nullptr;
    a.P = P;
    a.C = C;
    a.cpg = p.cpg;
    a.sc = p.sc;
    a.chunks = p.chunks;
    a.silu = flags & 1;
    a.eps = eps;
    const bool bf16 = (flags & UNET_ELEM_BF16) != 0;
    if (p.lds) {
        a.ncols = p.sc / 8;
        a.ngroups = p.G;
        if (bf16)
            return unet_groupnorm_launch_bf16(a, true, UG_GROUPS / p.G, p.plane, p.plane + UG_STATIC_LDS > 64 * 1024, n,
                                              (double)P * p.cpg, st);
        if (p.plane + UG_STATIC_LDS > 64 * 1024)
            if (int rc = allow_dyn_lds(unet_gn_lds_kernel, p.plane)) return rc;
        hipLaunchKernelGGL(unet_gn_lds_kernel, dim3(UG_GROUPS / p.G, n), dim3(UG_THREADS), p.plane, st, a);
        return check_launch();
    }
    a.ncols = C / 8;
    a.ngroups = UG_GROUPS;
    a.part = static_cast<double*>(workspace);
    a.mean = reinterpret_cast<float*>(a.part + (size_t)n * p.chunks * UG_GROUPS * 2);
    a.rstd = a.mean + (size_t)n * UG_GROUPS;
    if (bf16) return unet_groupnorm_launch_bf16(a, false, 0, 0, false, n, (double)P * p.cpg, st);
    hipLaunchKernelGGL(unet_gn_stats_kernel, dim3(p.chunks, n), dim3(UG_THREADS), 0, st, a);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(unet_gn_finish_kernel, dim3((n * UG_GROUPS + 255) / 256), dim3(256), 0, st, a.part, a.mean, a.rstd, n,
                       p.chunks, (double)P * p.cpg, eps);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(unet_gn_apply_kernel, dim3(p.chunks, n), dim3(UG_THREADS), 0, st, a);
    return check_launch();
}

extern "C" int unet_temb(const void* temb, const void* weight, const float* bias, const float* conv_bias, float* out, int n,
                         int K, int cout, void* stream) {
    return unet_temb_dt(temb, weight, bias, conv_bias, out, n, K, cout, FRESCO_F16, stream);
}

extern "C" int unet_temb_dt(const void* temb, const void* weight, const float* bias, const float* conv_bias, float* out, int n,
                            int K, int cout, int dtype, void* stream) {
    if (!temb || !weight || !bias || !conv_bias || !out || n <= 0 || K <= 0 || cout <= 0) return FRESCO_EINVAL;
    if (dtype != FRESCO_F16 && dtype != FRESCO_BF16) return FRESCO_EINVAL;
    if (n > UT_NMAX || K % 8) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(temb, 16) || !aligned_to(weight, 16) || !aligned_to(bias, 4) || !aligned_to(conv_bias, 4) || !aligned_to(out, 4))
        return FRESCO_EINVAL;
    if (dtype == FRESCO_BF16) return unet_temb_launch_bf16(temb, weight, bias, conv_bias, out, n, K, cout, as_stream(stream));
    auto kern = n <= UT_IT ? unet_temb_kernel<1> : (n <= 2 * UT_IT ? unet_temb_kernel<2> : (n <= 3 * UT_IT ? unet_temb_kernel<3> : unet_temb_kernel<4>));
    hipLaunchKernelGGL(kern, dim3((cout + 3) / 4), dim3(256), 0, as_stream(stream), static_cast<const half_t*>(temb),
                       static_cast<const half_t*>(weight), bias, conv_bias, out, n, K, cout);
    return check_launch();
}
