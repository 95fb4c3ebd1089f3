// Configuration of the dense-attention kernels of attn.hip (packed key-image geometry, softmax thresholds).  Not part of
// the public ABI.
#pragma once
#include "common.h"

namespace fresco {

template <int D>
struct AttnCfg {
    static constexpr int DPK = (D + 15) / 16 * 16;  // head dim padded for the QK^T contraction
    static constexpr int DPV = (D + 31) / 32 * 32;  // head dim padded to whole 32-row blocks of O^T
    static constexpr int NKS = DPK / 16;            // MFMA k-steps per QK^T block
    static constexpr int NDB = DPV / 32;            // 32-row blocks of O^T
    // LDS / packed image of one 64-key tile, in 16-byte chunks (8 halfs):
    //   K  : chunk ((ks*2 + c)*64 + key)   = K[key][ks*16 + c*8 .. +8]                     (c = MFMA k-chunk)
    //   V^T: chunk ((kc*2 + c)*DPV + d)    = V[kc*16 + slot(c, e)][d],  e = 0..7           (kc = 16-key MFMA step)
    //        slot(c, e) = (e & 3) + 8*(e >> 2) + 4*c: the order in which a lane's C-tile registers hold the keys
    // A 16-lane ds_read_b128 group reads 16 different keys (or 16 different d) at a chunk stride of 1 and one
    // c: conflict-free without padding.
    static constexpr int KTILE = DPK * 128;  // bytes
    static constexpr int VTILE = DPV * 128;
    static constexpr int TILE = KTILE + VTILE;
    static constexpr int NP = TILE / 1024;  // 1 KiB DMA pieces per tile
    static constexpr int NBUF = 4;          // ring slots
    static constexpr int LDS_BYTES = NBUF * TILE;
    static constexpr bool ONES = DPV > D;  // spare V^T row D holds ones: the PV MFMA also yields the row sum
    static constexpr bool MCOL = DPK > D;  // spare K column D holds ones: Q column D carries -m_run, so the
                                           // QK MFMA subtracts the running max (no C operand to keep around)
};

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// (tools/flash_regime.py restates the two per-wave decisions these thresholds drive on the CPU)
// online softmax: skip the O rescale while the tile max grows by less than this (log2 units);
// P then reaches at most 2^8 = 256, far inside fp16 range, and stays exactly normalised by the row sum
constexpr float RESCALE_THR = 8.0f;
// no running max at all when |c q| max|k| - m_run stays below this (P <= 2^14 = 16384 < 65504)
constexpr float NOMAX_THR = 14.0f;
// largest Cauchy-Schwarz logit bound c |q| max|k| (log2 units) for which the scale is folded into the fp16 Q.  Measured
// margin (tools/fold_margin.py, CPU emulation of the kernel's arithmetic against fp64): with N(0,1) keys the folded
// form's worst error is 0.30 of the 1e-3 parity bar for bounds up to 24 (0.09 for the exact form), 0.42 up to 32; with
// keys ALIGNED to the query (logit = bound) both forms sit at the same error, set by P's own fp16 rounding.  Round 2
// used 16: N(0,1) q, k (bound up to 23) then ran the exact pass on every workgroup, 11 % slower (r03_ab_variants.txt).
constexpr float FOLD_MAX = 24.0f;
// Whether an element type folds the scale at all.  bf16 does not: one bf16 rounding of c*q perturbs an exponent by up to
// 2^-9 c|q||k| (log2 units), 8x the fp16 figure.  Measured (tools/fold_margin.py --dtype bf16: the same CPU emulation with
// bf16 operands, bf16 P and m_run on the bf16 grid, worst error as a fraction of the bf16 bar 2^-7 (rms(v) + |ref|) of
// tests/test_gpu_bf16_attention.py), folded / exact: keys at 6 x N(0,1), (200, 333): D = 40 3.72 / 0.69, D = 80 3.66 / 0.56;
// N(0,1) keys by bound bucket: (4, 8] 0.018 / 0.017, (8, 16] 0.044 / 0.026, (16, 24] 0.40 / 0.11, (24, 32] 0.52 / 0.13,
// (32, 48] 1.11 / 0.30, > 48 1.52 / 0.32.  A fold limit near the fp16 one would cost a factor 4 of the bar's margin, one
// that costs nothing (<= 8) would rarely be met by N(0,1)-scale activations (bound 8 - 23 at D = 40) and would put a
// second, folded form of every pass into the bf16 instantiations.  So they keep Q exact and multiply every score by c in
// fp32: flash_body's "exact" pass unconditionally, and the same multiplication in flash_body_halves.
template <typename T>
struct FoldCfg {
    static constexpr bool ENABLE = true;
};
template <>
struct FoldCfg<bf16_t> {
    static constexpr bool ENABLE = false;
};

static inline int ntiles_of(int M) { return (M + 63) / 64; }

}  // namespace fresco
