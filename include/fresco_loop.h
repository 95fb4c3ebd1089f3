/* The glue of the denoising loop (fresco_amd/loop.py: inference and tensor2numpy; src/pipe_FRESCO.py:80-234,
 * src/utils.py:17-21).  DESIGN.md section 25.
 *
 * The entry points live in libfresco_hip.so and share its error codes (fresco_hip.h), its last-error string and its stream
 * convention (`stream` is a hipStream_t, null for the default stream; nothing synchronises); they are declared beside
 * fresco_hip.h, whose surface is pinned to its fresco_* names.  No atomics: same inputs give the same bits.  Every argument
 * check answers before any HIP call.  dtype is FRESCO_F16 / FRESCO_BF16 / FRESCO_F32; a code that names no element type is
 * FRESCO_EUNSUPPORTED.
 *
 *   loop_update : one DDPM step's update of `frames` frames of `frame_elems` elements each, and what the loop does to the
 *     new latents before the next UNet call, in one launch.  With i = f * frame_elems + j and n = frames * frame_elems:
 *
 *       e  = eps[i]                                  ; text_offset != 0: e + guidance * (eps[text_offset + i] - e)
 *       x0 = x0_in ? x0_in[i] : (xt[i] - sqrt_beta * e) / sqrt_alpha
 *       y  = round((c_x0 * x0 + c_xt * xt[i]) + sigma * noise[i % noise_period])
 *       if restore and f < 2:  y = restore[f * frame_elems + j]
 *       out[i] = y ; model_input[i] = y ; copies == 2: model_input[n + i] = y
 *       record: f == 0 -> record[j] = y ; f == frames - 1 -> record[frame_elems + j] = y
 *
 *     fp32 math (the formulas of csrc/ddpm_math.h, which fresco_ddpm_x0 / fresco_ddpm_prev use too), one rounding of y to
 *     the element type.  eps is the UNet's output as it comes: the uncond half first and the text half text_offset
 *     elements behind it; text_offset 0 means no guidance.  x0_in, restore (2 * frame_elems), model_input (copies * n) and
 *     record (2 * frame_elems) may each be null; eps may be null when x0_in is given.  With frames == 1 both record rows
 *     are frame 0; with frames == 2 record row 1 is the restored frame 1.  out == xt is allowed (every thread reads before
 *     it writes); every other overlap is the caller's error.  All tensors dense, aligned to their element size only.
 *     FRESCO_EINVAL: xt, noise or out null, eps and x0_in both null, a non-positive frames / frame_elems / noise_period, a
 *     negative text_offset, copies other than 1 or 2, restore with frames < 2, sqrt_alpha <= 0 (or NaN) without x0_in.
 *     FRESCO_EUNSUPPORTED: a dtype code that names no type, n above 2^38.
 *
 *   loop_image_to_frames : (n, C, H, W) fp16 or fp32 NCHW, C <= 4, to (n, H, W, C) uint8 with the arithmetic of the
 *     reference's tensor2numpy, each step rounded in the input's format as torch and numpy round it:
 *     b = x / 2; c = b + 0.5; d = clamp(c, 0, 1); e = d * 255; r = rint(e) (ties to even); uint8(r).  A NaN writes 0.
 *     FRESCO_EINVAL: a null pointer, a non-positive size.  FRESCO_EUNSUPPORTED: a dtype other than FRESCO_F16 / FRESCO_F32
 *     (FRESCO_BF16 too: the reference's .numpy() raises on it), C above 4, n * H * W above 2^38.
 */
#ifndef FRESCO_LOOP_H
#define FRESCO_LOOP_H

#include <stddef.h>
#include <stdint.h>

#include "fresco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int loop_update(const void* xt, const void* eps, const void* x0_in, const void* noise, const void* restore, void* out,
                void* model_input, void* record, int frames, int64_t frame_elems, int64_t text_offset, int64_t noise_period,
                int copies, float guidance, float sqrt_beta, float sqrt_alpha, float c_x0, float c_xt, float sigma, int dtype,
                void* stream);

int loop_image_to_frames(const void* x, void* out, int n, int C, int H, int W, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_LOOP_H */
