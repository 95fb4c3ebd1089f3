// The DDPM step's three formulas (src/pipe_FRESCO.py:35, :56 + :75, :214), fp32, written once: warp.hip's ddpm_x0_kernel /
// ddpm_prev_kernel and loop.hip's loop_update_kernel all call these, and both files are built with -ffp-contract=off, so the
// fused kernel rounds where the two-kernel route rounds (in fp32 nothing is rounded in between: the bits are the same).
#pragma once
#include <hip/hip_runtime.h>

namespace fresco {

// classifier-free guidance: eps = e_u + g (e_c - e_u)
__device__ __forceinline__ float ddpm_guided_eps(float e_u, float e_c, float g) { return e_u + g * (e_c - e_u); }

// formula (12) of DDIM: x0 = (x_t - sqrt(1 - abar_t) eps) / sqrt(abar_t)
__device__ __forceinline__ float ddpm_pred_x0(float xt, float e, float sqrt_beta, float sqrt_alpha) {
    return (xt - sqrt_beta * e) / sqrt_alpha;
}

// formula (7) of DDPM plus the variance term: x_{t-1} = (c0 x0 + c1 x_t) + sigma z
__device__ __forceinline__ float ddpm_posterior(float x0, float xt, float z, float c_x0, float c_xt, float sigma) {
    const float mean = c_x0 * x0 + c_xt * xt;
    return mean + sigma * z;
}

}  // namespace fresco
