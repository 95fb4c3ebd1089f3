// The denoising loop's glue (src/pipe_FRESCO.py:166-228, src/utils.py:17-21), fresco_amd/loop.py; ABI in
// include/fresco_loop.h; DESIGN.md section 25.
//
//   loop_update_kernel<T>  one plain step's whole update in one launch: classifier-free guidance (:212-214), predicted x0
//     (:35), the posterior mean and the noise term (:56, :75) in fp32 through ddpm_math.h with one rounding of the result;
//     then what the reference does to the new latents at the top of the next step: the rows restored from the previous
//     batch (:176), the recorded first and last frame (:177 / :179), and both halves of torch.cat([latents] * 2) (:182).
//     One thread per element; every thread reads its inputs before it writes, and writes only its own element (and that
//     element's copies), so out may be xt.  The latents of a batch are 131072 elements: the launch is the cost, the
//     kernel is not vectorised and takes any element count and any element-aligned pointer.
//   loop_frames_kernel<T>  tensor2numpy's arithmetic, operation for operation with the rounding of each torch / numpy step
//     in the input's own format, NCHW in, NHWC bytes out; one thread per pixel, the planes read coalesced.
//
// Built with -ffp-contract=off: b + 0.5 must not fuse with the halving, nor the posterior's products with its sums.
// Registers (VGPRs / AGPRs): loop_update_kernel and loop_frames_kernel stay far below one wave's budget; no spill, no
// scratch, no LDS (tests/test_kernel_resources_loop.py reads the metadata).
#include "common.h"
#include "ddpm_math.h"
#include "../../include/fresco_loop.h"

namespace fresco {

template <typename T>
__global__ __launch_bounds__(256) void loop_update_kernel(const T* xt, const T* eps, const T* x0_in, const T* noise,
                                                           const T* restore, T* out, T* model_input, T* record,
                                                           int frames, int64_t frame_elems, int64_t text_offset,
                                                           int64_t noise_period, int copies, float guidance,
                                                           float sqrt_beta, float sqrt_alpha, float c_x0, float c_xt,
                                                           float sigma) {
    const int64_t n = (int64_t)frames * frame_elems;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t f = i / frame_elems, j = i - f * frame_elems;
    T y;
    if (restore && f < 2) {
        y = restore[i];  // (f * frame_elems + j == i: the two restored rows are the first two frames)
    } else {
        const float x = (float)xt[i];
        float x0;
        if (x0_in) {
            x0 = (float)x0_in[i];
        } else {
            float e = (float)eps[i];
            if (text_offset) e = ddpm_guided_eps(e, (float)eps[text_offset + i], guidance);
            x0 = ddpm_pred_x0(x, e, sqrt_beta, sqrt_alpha);
        }
        y = (T)ddpm_posterior(x0, x, (float)noise[i % noise_period], c_x0, c_xt, sigma);
    }
    out[i] = y;
    if (model_input) {
        model_input[i] = y;
        if (copies == 2) model_input[n + i] = y;
    }
    if (record) {
        if (f == 0) record[j] = y;
        if (f == frames - 1) record[frame_elems + j] = y;
    }
}

template <typename T>
__device__ __forceinline__ unsigned char frame_byte(T x) {
    const T b = (T)((float)x * 0.5f);                           // img / 2
    const T c = (T)((float)b + 0.5f);                           // + 0.5
    if (c != c) return 0;                                       // NaN: numpy's cast is undefined, 0 here
    const T d = c < (T)0.f ? (T)0.f : (c > (T)1.f ? (T)1.f : c);  // clamp(0, 1)
    const T e = (T)((float)d * 255.f);                          // * 255 in the array's format
    return (unsigned char)rintf((float)e);                      // round(): ties to even; astype("uint8")
}

template <typename T>
__global__ __launch_bounds__(256) void loop_frames_kernel(const T* __restrict__ x, unsigned char* __restrict__ out, int C,
                                                           int64_t hw, int64_t pixels) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const int64_t img = p / hw, q = p - img * hw;
    const T* src = x + img * C * hw + q;
    unsigned char* dst = out + p * C;
    for (int c = 0; c < C; ++c) dst[c] = frame_byte<T>(src[(int64_t)c * hw]);
}

}  // namespace fresco

using namespace fresco;

extern "C" int loop_update(const void* xt, const void* eps, const void* x0_in, const void* noise, const void* restore,
                           void* out, void* model_input, void* record, int frames, int64_t frame_elems,
                           int64_t text_offset, int64_t noise_period, int copies, float guidance, float sqrt_beta,
                           float sqrt_alpha, float c_x0, float c_xt, float sigma, int dtype, void* stream) {
    if (!xt || !noise || !out || (!eps && !x0_in)) return FRESCO_EINVAL;
    if (frames <= 0 || frame_elems <= 0 || noise_period <= 0 || text_offset < 0) return FRESCO_EINVAL;
    if (copies != 1 && copies != 2) return FRESCO_EINVAL;
    if (restore && frames < 2) return FRESCO_EINVAL;  // the reference's latents[0:2] = ... fails there
    if (!x0_in && !(sqrt_alpha > 0.f)) return FRESCO_EINVAL;
    if (dtype != FRESCO_F16 && dtype != FRESCO_BF16 && dtype != FRESCO_F32) return FRESCO_EUNSUPPORTED;
    if (frame_elems > ((int64_t)1 << 38) / frames) return FRESCO_EUNSUPPORTED;  // the grid's x extent
    const int64_t n = (int64_t)frames * frame_elems;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t st = as_stream(stream);
#define LOOP_UPDATE_LAUNCH(T)                                                                                              \
    hipLaunchKernelGGL((loop_update_kernel<T>), grid, dim3(256), 0, st, (const T*)xt, (const T*)eps, (const T*)x0_in,     \
                       (const T*)noise, (const T*)restore, (T*)out, (T*)model_input, (T*)record, frames, frame_elems,       \
                       text_offset, noise_period, copies, guidance, sqrt_beta, sqrt_alpha, c_x0, c_xt, sigma)
    if (dtype == FRESCO_F16)
        LOOP_UPDATE_LAUNCH(half_t);
    else if (dtype == FRESCO_BF16)
        LOOP_UPDATE_LAUNCH(bf16_t);
    else
        LOOP_UPDATE_LAUNCH(float);
#undef LOOP_UPDATE_LAUNCH
    return check_launch();
}

extern "C" int loop_image_to_frames(const void* x, void* out, int n, int C, int H, int W, int dtype, void* stream) {
    if (!x || !out || n <= 0 || C <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (dtype != FRESCO_F16 && dtype != FRESCO_F32) return FRESCO_EUNSUPPORTED;  // (.numpy() raises on bf16)
    if (C > 4) return FRESCO_EUNSUPPORTED;
    const int64_t hw = (int64_t)H * W;
    if (hw > ((int64_t)1 << 38) / n) return FRESCO_EUNSUPPORTED;  // the grid's x extent
    const int64_t pixels = hw * n;
    const dim3 grid((unsigned)((pixels + 255) / 256));
    hipStream_t st = as_stream(stream);
    if (dtype == FRESCO_F16)
        hipLaunchKernelGGL((loop_frames_kernel<half_t>), grid, dim3(256), 0, st, (const half_t*)x, (unsigned char*)out, C, hw,
                           pixels);
    else
        hipLaunchKernelGGL((loop_frames_kernel<float>), grid, dim3(256), 0, st, (const float*)x, (unsigned char*)out, C, hw,
                           pixels);
    return check_launch();
}
