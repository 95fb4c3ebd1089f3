// The VAE encoder of fp16 pipelines (diffusers AutoencoderKL.encode, SD-1.5 VAE): what the decoder's kernels (vae.hip) lack.
// include/fresco_vae_enc.h, DESIGN.md section 18.
//
//   vaeenc_input_kernel      image NCHW fp16 -> fp16 NHWC rows padded to conv_in's K chunk
//   vaeenc_conv_down_kernel  Downsample2D(padding=0): 3 x 3, stride 2, zero pad on the right and bottom only
//   vaeenc_moments_kernel    conv_out's fp32 rows -> quant_conv (8 -> 8, fp32) -> parameters NCHW fp16
//   vaeenc_sample_kernel     scale (mean + exp(0.5 clamp(logvar, -30, 20)) noise), fp32, one rounding
//
// vaeenc_conv_down_kernel is conv_tile.h's fp16 implicit-GEMM tile (operands, wave layout, weight ring, XCD deal, epilogue
// map) on 8 x 16 output pixels, the nine taps inner.  What differs from vae_conv_kernel (vae.hip) is how the pixels
// arrive.  At stride 2 the tile's taps share little: its 17 x 33 source window (561 rows of 64 bytes,
// 35 KiB per slot) holds each source pixel for 2.25 taps on average where the stride-1 window holds it for 7.1, and two
// such slots beside the weights leave one workgroup per CU and need allow_dyn_lds.  So there is NO window: every (chunk,
// tap) step gathers its own 128 pixel rows, source pixel (2 yo + ky, 2 xo + kx), exactly as the 1 x 1 form of vae_conv
// gathers its rows -- 2.05 x the window's bytes, read from L2, for a third of its LDS.  LDS (dynamic, 32 KiB):
//   * two slots of 8 KiB for the pixels of one step: 128 rows of 64 bytes in tile order (row r = pixel (r >> 4, r & 15)),
//     swizzled as GEMM rows;
//   * conv_tile.h's two weight slots of 8 KiB.
// Five workgroups fit a CU's 160 KiB by LDS; the register file (144 of 512 per lane) keeps three.  Everything arrives by
// LDS-DMA (lds_dma.h).  Step s: every wave waits for its own copies (vmcnt(0)), barrier -- step s is in LDS and step s - 1
// has been read -- then the pixels and weights of step s + 1 are issued into the other slots and fly under the MFMAs of
// step s.  Source rows y = H and columns x = W (the pad) and output pixels past the plane come from the zero page.
#include "common.h"
#include "lds_dma.h"
#include "conv_tile.h"
#include "../../include/fresco_vae_enc.h"

namespace fresco {

constexpr int VD_A_BYTES = 8 * 1024;  // 128 pixel rows of 64 bytes
constexpr int VD_LDS = 2 * VD_A_BYTES + 2 * CT_B_BYTES;

struct VaeDown {
    const half_t* x;
    const half_t* w;
    const float* bias;
    half_t* out;
    int n, H, W, Ho, Wo, cin, cout;
    int tiles_x, tiles_per_img;
};

__global__ __launch_bounds__(256) void vaeenc_conv_down_kernel(const VaeDown a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const CtTile t = ct_deal(a.n, a.tiles_per_img);
    const int img = t.img, co0 = t.col_tile * CT_BN;
    const int ty0 = (t.t_in / a.tiles_x) * CT_TH, tx0 = (t.t_in % a.tiles_x) * CT_TW;
    const uint32_t lds0 = lds_addr(smem);
    const char* zp = reinterpret_cast<const char*>(ct_zero_page);

    // ---- DMA sources, pixel rows laid out as the weight rows are (ct_gemm_slot).
    // a_src: tap (0, 0) of the row's output pixel, chunk 0 (always inside the image where the pixel is); a_ok: bit t set
    // where tap t of that pixel is inside the image.  Only taps with ky = 2 or kx = 2 can reach the pad.
    const char* a_src[2];
    int a_ok[2];
    const char* b_src[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int R, pc;
        ct_gemm_slot(wave, p, lane, R, pc);
        const int yo = ty0 + (R >> 4), xo = tx0 + (R & 15);
        const bool ok = yo < a.Ho && xo < a.Wo;
        const int rows_ok = 2 * yo + 2 < a.H ? 0x1FF : 0x03F, cols_ok = 2 * xo + 2 < a.W ? 0x1FF : 0x0DB;
        a_ok[p] = ok ? (rows_ok & cols_ok) : 0;
        a_src[p] = reinterpret_cast<const char*>(a.x + (((int64_t)img * a.H + 2 * yo) * a.W + 2 * xo) * a.cin + pc * 8);
        b_src[p] = ct_weight_src(a.w, co0, R, pc, a.cout, 9 * a.cin);
    }
    // step (chunk, tap): pixels at a_off bytes from the lane's tap-(0, 0) address, weights at column k0
    auto issue = [&](int s, int tap, int64_t a_off, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            lds_dma16((a_ok[p] >> tap) & 1 ? static_cast<const void*>(a_src[p] + a_off) : static_cast<const void*>(zp),
                      lds0 + (uint32_t)((s & 1) * VD_A_BYTES + (wave * 2 + p) * 1024));
        ct_issue_weights(b_src, s, k0, lds0 + 2 * VD_A_BYTES, wave);
    };

    const int nbv = ct_live_blocks(a.cout, co0, wn);
    floatx16 acc[2][2] = {};  // [channel block j][pixel block i]

    const int chunks = a.cin / CT_BK, steps = chunks * 9;
    const int sw = (l31 >> 2) & 3;  // rows wm 64 + i 32 + l31 and wn 64 + j 32 + l31 share it
    issue(0, 0, 0, 0);
    int chunk = 0, tap = 0;
    for (int s = 0; s < steps; ++s) {
        dma_wait_barrier<0>();
        if (s + 1 < steps) {
            const int t1 = tap + 1 == 9 ? 0 : tap + 1, c1 = tap + 1 == 9 ? chunk + 1 : chunk;
            const int ky = t1 / 3, kx = t1 - ky * 3;
            issue(s + 1, t1, (((int64_t)ky * a.W + kx) * a.cin + c1 * CT_BK) * 2, t1 * a.cin + c1 * CT_BK);
        }
        const char* pa = smem + (s & 1) * VD_A_BYTES + (wm * 64 + l31) * 64;
        const char* pb = smem + 2 * VD_A_BYTES + (s & 1) * CT_B_BYTES + (wn * 64 + l31) * 64;
#pragma unroll
        for (int ks = 0; ks < CT_BK / 16; ++ks) {
            const int piece = ((ks * 2 + hi) ^ sw) * 16;
            half8_t px[2], wt[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) px[i] = *reinterpret_cast<const half8_t*>(pa + i * 32 * 64 + piece);
#pragma unroll
            for (int j = 0; j < 2; ++j) wt[j] = *reinterpret_cast<const half8_t*>(pb + j * 32 * 64 + piece);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j < nbv) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[j], px[i], acc[j][i], 0, 0, 0);
                }
        }
        if (++tap == 9) {
            tap = 0;
            ++chunk;
        }
    }

    // ---- epilogue (conv_tile.h's map).  Every address is computed before the first store.
    int64_t opix[2];  // pixel index over all images, -1: outside the plane
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = ct_row(wm, i, l31);
        const int yo = ty0 + (r >> 4), xo = tx0 + (r & 15);
        opix[i] = (yo < a.Ho && xo < a.Wo) ? ((int64_t)img * a.Ho + yo) * a.Wo + xo : -1;
    }
    if (!(a.cout & 3)) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = ct_channel(co0, wn, j, hi, 4 * g);
                if (co >= a.cout) continue;
                const floatx4 bv = *reinterpret_cast<const floatx4*>(a.bias + co);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (opix[i] < 0) continue;
                    half4_t o4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o4[e] = (half_t)(acc[j][i][4 * g + e] + bv[e]);
                    *reinterpret_cast<half4_t*>(a.out + opix[i] * a.cout + co) = o4;
                }
            }
    } else {
        // a channel count that is no multiple of four: one element per store
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (opix[i] < 0) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct_channel(co0, wn, j, hi, r);
                    if (co < a.cout) a.out[opix[i] * a.cout + co] = (half_t)(acc[j][i][r] + a.bias[co]);
                }
            }
    }
}

// One thread per pixel.
__global__ __launch_bounds__(256) void vaeenc_input_kernel(const half_t* __restrict__ img, half_t* __restrict__ out, int n,
                                                           int hw, int cpad) {
    const int64_t total = (int64_t)n * hw;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx / hw, p = idx - i * hw;
        half8_t o8;
#pragma unroll
        for (int e = 0; e < 8; ++e) o8[e] = (half_t)0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) o8[c] = img[(i * 3 + c) * hw + p];
        ct_store_padded_row(out + idx * cpad, o8, cpad);
    }
}

// One thread per latent pixel: its eight fp32 values, the 8 x 8 product in fp32 (o ascending, c ascending), eight fp16 stores
// that run along x in their planes.
__global__ __launch_bounds__(256) void vaeenc_moments_kernel(const float* __restrict__ h, const float* __restrict__ wq,
                                                             const float* __restrict__ bq, half_t* __restrict__ params, int n,
                                                             int hw) {
    const int64_t total = (int64_t)n * hw;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx / hw, p = idx - i * hw;
        const floatx4 v0 = *reinterpret_cast<const floatx4*>(h + idx * 8), v1 = *reinterpret_cast<const floatx4*>(h + idx * 8 + 4);
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            float s = bq[o];
#pragma unroll
            for (int c = 0; c < 8; ++c) s += wq[o * 8 + c] * (c < 4 ? v0[c & 3] : v1[c & 3]);
            params[(i * 8 + o) * hw + p] = (half_t)s;
        }
    }
}

// One thread per latent element.
__global__ __launch_bounds__(256) void vaeenc_sample_kernel(const half_t* __restrict__ params, const half_t* __restrict__ noise,
                                                            half_t* __restrict__ out, int n, int hw, float scale) {
    const int64_t per = (int64_t)4 * hw, total = (int64_t)n * per;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx / per, r = idx - i * per;
        const float mean = (float)params[i * 2 * per + r];
        const float logvar = fminf(fmaxf((float)params[i * 2 * per + per + r], -30.f), 20.f);
        out[idx] = (half_t)(scale * (mean + expf(0.5f * logvar) * (float)noise[idx]));
    }
}

}  // namespace fresco

using namespace fresco;

extern "C" int vaeenc_input(const void* image, void* out, int n, int H, int W, int cpad, void* stream) {
    if (!image || !out || n <= 0 || H <= 0 || W <= 0) return FRESCO_EINVAL;
    if (cpad < 8 || cpad > 64 || cpad % 8) return FRESCO_EINVAL;
    if (!aligned_to(image, 2) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    if ((int64_t)n * H * W >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(vaeenc_input_kernel, dim3(stream_blocks((int64_t)n * H * W)), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t*>(image), static_cast<half_t*>(out), n, H * W, cpad);
    return check_launch();
}

extern "C" int vaeenc_conv_down(const void* x, const void* w, const float* bias, void* out, int n, int H, int W, int cin,
                                int cout, void* stream) {
    if (!x || !w || !bias || !out || n <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0) return FRESCO_EINVAL;
    if (!aligned_to(x, 16) || !aligned_to(w, 16) || !aligned_to(bias, 16) || !aligned_to(out, 8)) return FRESCO_EINVAL;
    if (H < 2 || W < 2 || !ct_supported(n, H, W, cin)) return FRESCO_EUNSUPPORTED;
    VaeDown a;
    a.x = static_cast<const half_t*>(x);
    a.w = static_cast<const half_t*>(w);
    a.bias = bias;
    a.out = static_cast<half_t*>(out);
    a.n = n;
    a.H = H;
    a.W = W;
    a.Ho = H / 2;
    a.Wo = W / 2;
    a.cin = cin;
    a.cout = cout;
    a.tiles_x = ct_tiles_x(a.Wo);
    a.tiles_per_img = ct_plane_tiles(a.Ho, a.Wo);
    const unsigned grid = ct_grid(n, a.tiles_per_img, cout);
    if (!grid) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(vaeenc_conv_down_kernel, dim3(grid), dim3(256), VD_LDS, as_stream(stream), a);
    return check_launch();
}

extern "C" int vaeenc_moments(const float* h, const float* weight, const float* bias, void* params, int n, int hh, int ww,
                              void* stream) {
    if (!h || !weight || !bias || !params || n <= 0 || hh <= 0 || ww <= 0) return FRESCO_EINVAL;
    if (!aligned_to(h, 16) || !aligned_to(weight, 4) || !aligned_to(bias, 4) || !aligned_to(params, 2)) return FRESCO_EINVAL;
    if ((int64_t)n * hh * ww >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(vaeenc_moments_kernel, dim3(stream_blocks((int64_t)n * hh * ww)), dim3(256), 0, as_stream(stream), h, weight,
                       bias, static_cast<half_t*>(params), n, hh * ww);
    return check_launch();
}

extern "C" int vaeenc_sample(const void* params, const void* noise, void* out, int n, int hh, int ww, float scale, void* stream) {
    if (!params || !noise || !out || n <= 0 || hh <= 0 || ww <= 0 || !(scale == scale)) return FRESCO_EINVAL;
    if (!aligned_to(params, 2) || !aligned_to(noise, 2) || !aligned_to(out, 2)) return FRESCO_EINVAL;
    if ((int64_t)n * hh * ww >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(vaeenc_sample_kernel, dim3(stream_blocks((int64_t)n * 4 * hh * ww)), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t*>(params), static_cast<const half_t*>(noise), static_cast<half_t*>(out), n,
                       hh * ww, scale);
    return check_launch();
}
