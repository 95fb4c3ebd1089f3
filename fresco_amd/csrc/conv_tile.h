// The plain-fp16 implicit-GEMM convolution tile that vae.hip (vae_conv_kernel<TAPS, T> of vae_conv_body.h, which net_bf16.hip
// instantiates for bf16 too: nothing below but the MFMA and the fragment types depends on the 2-byte element type) and
// vae_enc.hip (vaeenc_conv_down_kernel) share.  Each kernel keeps how its pixels reach LDS, its output kinds, and the MFMA step and
// half4_t store written out (see below): whoever changes the swizzle, the fragment layout or the channel map changes it here.
//
// Plain fp16 operands, one v_mfma_f32_32x32x16_f16 per product, fp32 accumulators.  A workgroup of four waves owns 128
// output pixels x 128 output channels (waves 2 x 2: wm = wave >> 1 the pixel half, wn = wave & 1 the channel half, each
// 64 x 64 = 2 x 2 MFMA blocks); the WEIGHTS are the MFMA's row operand and the pixels its column operand, so lane
// (l31, hi) ends up with pixel .. + l31 and, in registers 4 g .. 4 g + 3 of a block, the four CONSECUTIVE channels
// 8 g + 4 hi .. + 3: fp16 NHWC results leave as 8-byte stores.  The K loop is channel chunks (32) OUTER, taps INNER;
// weights are packed (cout, K) fp16 with k = (tap, ci) (vae.py's pack_conv_weight), so step (chunk, tap) reads weight
// columns tap cin + 32 chunk .. + 31.
// LDS: behind the caller's pixel slots, two slots of 8 KiB for the weights of one step, 128 rows of 64 bytes.  A GEMM row's
// four 16-byte pieces sit at piece ^ ((row >> 2) & 3) (flownet.hip's map), and lane l of a wave's 1 KiB DMA piece owns
// LDS piece (slot & 3) of row slot >> 2, so it fetches source piece (slot & 3) ^ swizzle(row).  Weight rows >= cout, and
// whatever pixels a caller has nothing to read for, come from a zero page: a select on the source address, no branch in
// the loop.  A wave whose 32-channel block lies wholly beyond cout skips its MFMAs.
// Workgroups: the 1-D grid is dealt to the 8 XCDs in turn; XCD x walks a contiguous range of (column tile, pixel tile)
// with the pixel tile fastest, so one column tile's weights (1.2 MB at K = 4608) stay in that XCD's L2.
// No split-K, no atomics: same inputs, same bits.
//
// LINKAGE: the zero page sits in an unnamed namespace (as groupnorm_stats.h's kernels do): it is written once here and
// every file that includes this header gets its own 16 bytes, so the library links without a duplicate symbol.
#pragma once
#include "common.h"
#include "lds_dma.h"

namespace fresco {

constexpr int CT_BM = 128, CT_BN = 128, CT_BK = 32;  // pixels, channels, K chunk of a tile
constexpr int CT_TH = 8, CT_TW = 16;                 // the 128 pixels of a tile in a plane
constexpr int CT_B_BYTES = 8 * 1024;                 // 128 weight rows of 64 bytes
// (vae_conv_body.h's window slot, here so that vae.hip and net_bf16.hip add up one pair of constants)
constexpr int VC_A_BYTES = 12 * 1024;  // 12 pieces of 64 lanes x 16 bytes = 192 window rows of 64 bytes (180 used)

namespace {
// what the LDS-DMA reads where there is nothing to read
__device__ __attribute__((aligned(16))) unsigned int ct_zero_page[4] = {0u, 0u, 0u, 0u};
}  // namespace

struct CtTile {
    int col_tile, img, t_in;  // 128-channel column, image, tile in the image
};

// XCD x = block % 8 owns the logical range [x q + min(x, rem), ..) of q + (x < rem) tiles, T = 8 q + rem
__device__ __forceinline__ CtTile ct_deal(int n, int tiles_per_img) {
    const int T = gridDim.x, b = blockIdx.x, x = b & 7, q = T >> 3, rem = T & 7;
    const int L = x * q + min(x, rem) + (b >> 3);
    const int PT = n * tiles_per_img;
    CtTile t;
    t.col_tile = L / PT;
    const int pt = L - t.col_tile * PT;
    t.img = pt / tiles_per_img;
    t.t_in = pt - t.img * tiles_per_img;
    return t;
}

// the source piece that lane `lane` of DMA piece p of `wave` (two pieces per wave and slot) fetches for GEMM row R
__device__ __forceinline__ void ct_gemm_slot(int wave, int p, int lane, int& R, int& pc) {
    const int slot = (wave * 2 + p) * 64 + lane;
    R = slot >> 2;
    pc = (slot & 3) ^ ((R >> 2) & 3);
}

// weight row co0 + R at column 0 (w: this image's (cout, K) matrix of 2-byte elements), null for rows >= cout
template <typename T>
__device__ __forceinline__ const char* ct_weight_src(const T* w, int co0, int R, int pc, int cout, int K) {
    static_assert(sizeof(T) == 2, "a piece is eight 2-byte elements");
    return co0 + R < cout ? reinterpret_cast<const char*>(w + (int64_t)(co0 + R) * K + pc * 8) : nullptr;
}

// step s's weights, columns k0 .. k0 + 31, into weight slot s & 1 (lds_b: the LDS address of weight slot 0)
__device__ __forceinline__ void ct_issue_weights(const char* const (&b_src)[2], int s, int k0, uint32_t lds_b, int wave) {
    const char* zp = reinterpret_cast<const char*>(ct_zero_page);
#pragma unroll
    for (int p = 0; p < 2; ++p)
        lds_dma16(b_src[p] ? static_cast<const void*>(b_src[p] + (int64_t)k0 * 2) : static_cast<const void*>(zp),
                  lds_b + (uint32_t)((s & 1) * CT_B_BYTES + (wave * 2 + p) * 1024));
}

// this wave's 32-channel blocks that hold a channel < cout (wave-uniform): the others are skipped, not multiplied
__device__ __forceinline__ int ct_live_blocks(int cout, int co0, int wn) {
    const int nbv = (cout - co0 - wn * 64 + 31) / 32;
    return nbv < 0 ? 0 : (nbv > 2 ? 2 : nbv);
}

// (The MFMA step itself -- two half8_t pixel fragments, two weight fragments at pb + j 32 64 + (piece ^ swizzle) 16, 2 x 2
// MFMAs under j < nbv -- stands in each kernel: as a function of this header it compiles to the same register counts, but
// hipcc then copies one accumulator block from VGPRs into AGPRs every step, and every 3 x 3 form measured 5 - 18 % slower.
// The epilogue's half4_t store likewise: through a helper it costs four VGPRs in two of the three kernels.)

// ---- the accumulators' map: this lane's tile row in pixel block i, and the channel of register r of channel block j
// (registers 4 g .. 4 g + 3 are consecutive channels: ct_channel(.., 4 g) is where quad g's 8-byte store begins)
__device__ __forceinline__ int ct_row(int wm, int i, int l31) { return wm * 64 + i * 32 + l31; }
__device__ __forceinline__ int ct_channel(int co0, int wn, int j, int hi, int r) {
    return co0 + wn * 64 + j * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
}

// An input kernel's NHWC row, padded to the convolution's K chunk: eight real lanes, then zero pieces up to cpad.
__device__ __forceinline__ void ct_store_padded_row(half_t* row, const half8_t& o8, int cpad) {
    *reinterpret_cast<half8_t*>(row) = o8;
    const half8_t z8 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
    for (int c = 8; c < cpad; c += 8) *reinterpret_cast<half8_t*>(row + c) = z8;
}

// ---- host side
static inline int ct_tiles_x(int W) { return (W + CT_TW - 1) / CT_TW; }
static inline int ct_plane_tiles(int H, int W) { return ct_tiles_x(W) * ((H + CT_TH - 1) / CT_TH); }
// n images of H x W pixels and cin channels: whole K chunks, at most 65535 images, int32 pixel indices
static inline bool ct_supported(int n, int H, int W, int cin) {
    return cin % CT_BK == 0 && n <= 65535 && (int64_t)n * H * W < (int64_t)1 << 31;
}
// the 1-D grid of ct_deal, or 0 where it does not fit 31 bits
static inline unsigned ct_grid(int n, int tiles_per_img, int cout) {
    const int64_t grid = (int64_t)n * tiles_per_img * ((cout + CT_BN - 1) / CT_BN);
    return grid < (int64_t)1 << 31 ? (unsigned)grid : 0u;
}

}  // namespace fresco
