// The bf16 twins of the kernels a UNet ResnetBlock2D runs on: the SAME text as the fp16 kernels of
// vae.hip and unet.hip, instantiated for bf16_t from vae_conv_body.h and unet_body.h, and the launches that vae_conv,
// unet_groupnorm and unet_temb(_dt) hand over to once they have checked their arguments and made their plan.
//
//   vae_conv_kernel<9 / 1, bf16_t>  bf16 operands on v_mfma_f32_32x32x16_bf16, fp32 accumulators, one rounding to nearest
//                                   even at the store; VAE_OUT_F16 / VAE_OUT_F16_NCHW give bf16, VAE_OUT_F32 fp32
//   unet_gn_lds_kernel_t<bf16_t>, unet_gn_stats_kernel_t / unet_gn_finish_kernel_t / unet_gn_apply_kernel_t<bf16_t>
//                                   x and y bf16; addend, gamma, beta fp32; statistics fp64 in the fixed order
//   unet_temb_kernel_t<1..4, bf16_t> temb and W bf16; SiLU, the sums and the output fp32
//
// They stand in a file of their own because vae.hip and unet.hip are listed kernel by kernel (tests/test_kernel_resources_
// vae.py, _unet.py); this file's listing is tests/test_bf16_net_cpu.py's.  LDS, grids and workgroup sizes are the fp16
// kernels': both element types are 2 bytes wide.  No split-K, no atomics: same inputs, same bits.
#include "common.h"
#include "vae_conv_body.h"
#include "unet_body.h"

namespace fresco {

// (vae.hip's VC_LDS: two window slots and conv_tile.h's two weight slots, 40 KiB)
constexpr int NB_CONV_LDS = 2 * VC_A_BYTES + 2 * CT_B_BYTES;

// the bf16 instantiations, under the names the launches below use
template <int TAPS>
constexpr auto vae_conv_bf16_kernel = vae_conv_kernel<TAPS, bf16_t>;
constexpr auto unet_gn_lds_bf16_kernel = unet_gn_lds_kernel_t<bf16_t>;
constexpr auto unet_gn_stats_bf16_kernel = unet_gn_stats_kernel_t<bf16_t>;
constexpr auto unet_gn_finish_bf16_kernel = unet_gn_finish_kernel_t<bf16_t>;
constexpr auto unet_gn_apply_bf16_kernel = unet_gn_apply_kernel_t<bf16_t>;
template <int TILES>
constexpr auto unet_temb_bf16_kernel = unet_temb_kernel_t<TILES, bf16_t>;

int vae_conv_launch_bf16(const VaeConv& a, int ksize, unsigned grid, hipStream_t st) {
    if (ksize == 3)
        hipLaunchKernelGGL(vae_conv_bf16_kernel<9>, dim3(grid), dim3(256), NB_CONV_LDS, st, a);
    else
        hipLaunchKernelGGL(vae_conv_bf16_kernel<1>, dim3(grid), dim3(256), NB_CONV_LDS, st, a);
    return check_launch();
}

int unet_groupnorm_launch_bf16(const UgArgs& a, bool lds_form, int slabs, int plane, bool plane_needs_leave, int n, double count,
                               hipStream_t st) {
    if (lds_form) {
        if (plane_needs_leave)
            if (int rc = allow_dyn_lds(unet_gn_lds_bf16_kernel, plane)) return rc;
        hipLaunchKernelGGL(unet_gn_lds_bf16_kernel, dim3(slabs, n), dim3(UG_THREADS), plane, st, a);
        return check_launch();
    }
    hipLaunchKernelGGL(unet_gn_stats_bf16_kernel, dim3(a.chunks, n), dim3(UG_THREADS), 0, st, a);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(unet_gn_finish_bf16_kernel, dim3((n * UG_GROUPS + 255) / 256), dim3(256), 0, st, a.part, a.mean, a.rstd, n,
                       a.chunks, count, a.eps);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(unet_gn_apply_bf16_kernel, dim3(a.chunks, n), dim3(UG_THREADS), 0, st, a);
    return check_launch();
}

int unet_temb_launch_bf16(const void* temb, const void* weight, const float* bias, const float* conv_bias, float* out, int n, int K,
                          int cout, hipStream_t st) {
    auto kern = n <= UT_IT ? unet_temb_bf16_kernel<1>
                           : (n <= 2 * UT_IT ? unet_temb_bf16_kernel<2> : (n <= 3 * UT_IT ? unet_temb_bf16_kernel<3> : unet_temb_bf16_kernel<4>));
    hipLaunchKernelGGL(kern, dim3((cout + 3) / 4), dim3(256), 0, st, static_cast<const bf16_t*>(temb),
                       static_cast<const bf16_t*>(weight), bias, conv_bias, out, n, K, cout);
    return check_launch();
}

}  // namespace fresco
