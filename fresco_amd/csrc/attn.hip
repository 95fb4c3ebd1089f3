// Dense fp16 / bf16 attention with shared key groups for FRESCO's spatial-guided and efficient
// cross-frame passes (reference: src/diffusion_hacked.py:225-247, 250-254, 281-285, 303-305, 371).
//
// Two kernels:
//   kv_pack_kernel  : gathers the selected K / V rows of one key group and writes, per 64-key tile, the
//                     exact LDS image the MFMA loop consumes (K fragments ‖ V^T fragments, 16-byte chunks
//                     in ds_read_b128-conflict-free order).  HBM-bound, a few MB.
//   attn_flash_kernel: flash-style attention on v_mfma_f32_32x32x16_f16.  One wave owns 32*QB query rows, a
//                     workgroup 8 waves = two per SIMD, 256 registers each.  S^T = K Q^T is computed
//                     "swapped", so every lane holds the scores of ONE query (its column of the 32x32 C tile):
//                     the softmax needs no cross-lane traffic and the exponentiated scores, packed to fp16,
//                     already ARE the B operand of O^T = V^T P^T (the key order inside each 16-key MFMA step is
//                     the C-tile row order; kv_pack writes V^T in it).
//
// What bounds this kernel on gfx950 (tools/ubench_rates.hip, profiles/r02_attn_experiments.txt): not the matrix
// pipe alone but the SIMD's one VALU/issue port, which v_exp_f32 holds for 8.25 cycles, v_cvt_pk_f16_f32 for
// 4.3 and every MFMA issue for ~7 -- from either of the two waves of the SIMD; MFMA execution (32 cycles per
// 32x32x16) overlaps with the partner wave's VALU work, but two waves left to themselves run in lockstep
// (both in their MFMA block, then both in their softmax block: MFMA time + VALU time, no overlap).  Per 64 keys
// x 64 queries at D = 40: port = 64 exp + 32 cvt + 28 MFMA issues ~ 880 cycles, matrix pipe = 28 x 32 = 896.
// Hence: as few and as large MFMAs as possible (32x32x16 for both products; a 16x16x32 PV product would save
// pipe time but costs more issues plus a permlane per P register: measured slower), no per-score VALU besides
// exp and cvt (the scale is folded into Q, the running max rides in the QK product, the row sum in the PV
// product, see below), and an explicit PING-PONG of the two waves of a SIMD:
//   * waves 0-3 (group A) and 4-7 (group B) run the same loop body  [ring barrier | V^T reads, softmax(u) |
//     K reads, PV(u), QK(u+1)], but A passes the workgroup barrier AFTER its softmax and B BEFORE it: the
//     barrier therefore releases A's matrix block together with B's softmax block and vice versa, and keeps
//     them half a step apart for the whole key loop (s_setprio raises the matrix block);
//   * key packs (K of tile u+1 next to V^T of tile u: exactly what one loop body reads) arrive by DMA
//     (lds_dma.h: linear 1 KiB copies) into a 4-slot LDS ring, three steps ahead, behind counted
//     vmcnt waits and that ONE barrier per step;
//   * K fragments are read under the PV MFMAs, V^T fragments under the softmax: no MFMA waits on LDS;
//   * two query blocks per wave at D <= 48, and at D = 80 with the loop in half tiles (flash_body_halves): every
//     fragment read feeds two MFMAs;
//   * the common case (no diagonal bias, scale folded, >= 3 tiles ahead) is an instantiation of its own without
//     the scalar branches of the rare passes (a taken branch costs an instruction-fetch bubble).
// The softmax bookkeeping rides in the MFMAs wherever the head dim leaves room: a ones ROW in V^T makes the
// PV product deliver the row sum, a ones COLUMN in K against -m in Q's spare column makes the QK product
// subtract the running max.  Per wave, from the key norms kv_pack records (Cauchy-Schwarz bound on the
// logits): the max search is dropped when no exponent can leave fp16 range, and the exponent scale is folded
// into the fp16 Q only while that costs no more than P's own rounding.
//
// MFMA 32x32x16 f16 operand layout (gfx950): lane l supplies 8 consecutive k for row/col (l & 31), k-chunk
// (l >> 5); C/D: col = l & 31, row = (r & 3) + 8*(r >> 2) + 4*(l >> 5), r = 0..15.
#include "attn_cfg.h"
#include "lds_dma.h"
#include <type_traits>

namespace fresco {

// ---------------------------------------------------------------------------------------------
// pack: grid (nT, H, G), 256 threads.  Pack p of the image = K fragments of tile p || V^T fragments of tile p - 1: what
// ONE loop step of attn_flash_kernel reads (PV(u) next to QK(u+1)); nT + 1 packs.
// ---------------------------------------------------------------------------------------------
template <typename T, int D>
__device__ __forceinline__ void kv_pack_body(const T* __restrict__ k, const T* __restrict__ v,
                                             const int32_t* __restrict__ kv_rows, char* __restrict__ img,
                                             float* __restrict__ ktmax, int H, int M, int nT, int64_t group_rows,
                                             int64_t kv_ld) {
    using Cfg = AttnCfg<D>;
    typedef typename Elem<T>::x8 X8;
    const int tile = blockIdx.x, h = blockIdx.y, g = blockIdx.z;
    __shared__ int32_t rows[64];
    __shared__ __attribute__((aligned(16))) T ks[64][D + 8];  // +8 halfs: 16-B aligned rows
    __shared__ __attribute__((aligned(16))) T vs[64][D + 8];

    if (threadIdx.x < 64) {
        const int m = tile * 64 + threadIdx.x;
        int32_t r = -1;
        if (m < M) r = kv_rows ? kv_rows[m] : m;
        rows[threadIdx.x] = r;
    }
    __syncthreads();

    // stage the 64 x D slabs of K and V (each row D halfs contiguous in global memory)
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (int c = threadIdx.x; c < 64 * (D / 8); c += 256) {
        const int row = c / (D / 8), dc = c % (D / 8);
        uint4 kv = zero, vv = zero;
        const int32_t r = rows[row];
        if (r >= 0) {
            const int64_t off = ((int64_t)g * group_rows + r) * kv_ld + h * D + dc * 8;
            kv = *reinterpret_cast<const uint4*>(k + off);
            vv = *reinterpret_cast<const uint4*>(v + off);
        }
        *reinterpret_cast<uint4*>(&ks[row][dc * 8]) = kv;
        *reinterpret_cast<uint4*>(&vs[row][dc * 8]) = vv;
    }
    __syncthreads();

    char* dst = img + ((int64_t)(g * H + h) * (nT + 1) + tile) * Cfg::TILE;
    // K chunks
    for (int c = threadIdx.x; c < Cfg::NKS * 128; c += 256) {
        const int key = c & 63, d0 = (c >> 6) * 8;
        uint4 val = zero;
        if (d0 < D)
            val = *reinterpret_cast<const uint4*>(&ks[key][d0]);
        else if (Cfg::MCOL && d0 == D && rows[key] >= 0)
            val.x = Elem<T>::ONE_BITS;  // K[key][D] = 1.0: with Q[query][D] = -m the QK MFMA delivers  q.k - m
        *reinterpret_cast<uint4*>(dst + (int64_t)c * 16) = val;
    }
    // V^T chunks
    for (int c = threadIdx.x; c < 8 * Cfg::DPV; c += 256) {
        const int d = c % Cfg::DPV, cc = (c / Cfg::DPV) & 1, kc = c / (2 * Cfg::DPV);
        X8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int key = kc * 16 + (e & 3) + 8 * (e >> 2) + 4 * cc;
            T val = (T)0;
            if (d < D)
                val = vs[key][d];
            else if (Cfg::ONES && d == D && rows[key] >= 0)
                val = (T)1;  // ones row: only real keys count towards the softmax denominator
            o[e] = val;
        }
        *reinterpret_cast<X8*>(dst + Cfg::TILE + Cfg::KTILE + (int64_t)c * 16) = o;
    }
    // largest squared key norm of the tile (four threads per key, fixed summation order): the flash kernel
    // bounds every logit of a query by |q| max|k| (Cauchy-Schwarz) and drops the running-max search when
    // that bound cannot leave fp16 range
    {
        const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
        float n2 = 0.f;
        for (int dc = part; dc < D / 8; dc += 4) {
            const X8 kk = *reinterpret_cast<const X8*>(&ks[row][dc * 8]);
#pragma unroll
            for (int e = 0; e < 8; ++e) n2 = fmaf((float)kk[e], (float)kk[e], n2);
        }
        n2 += __shfl_xor(n2, 1, 64);
        n2 += __shfl_xor(n2, 2, 64);
#pragma unroll
        for (int off = 32; off >= 4; off >>= 1) n2 = fmaxf(n2, __shfl_xor(n2, off, 64));
        __shared__ float wmax[4];
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = n2;
        __syncthreads();
        if (threadIdx.x == 0)
            ktmax[(int64_t)(g * H + h) * nT + tile] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    }
}

#define FRESCO_KV_PACK_KERNEL(NAME, T)                                                                            \
    template <int D>                                                                                              \
    __global__ __launch_bounds__(256) void NAME(const T* __restrict__ k, const T* __restrict__ v,                  \
                                                const int32_t* __restrict__ kv_rows, char* __restrict__ img,       \
                                                float* __restrict__ ktmax, int H, int M, int nT,                   \
                                                int64_t group_rows, int64_t kv_ld) {                               \
        kv_pack_body<T, D>(k, v, kv_rows, img, ktmax, H, M, nT, group_rows, kv_ld);                                \
    }
FRESCO_KV_PACK_KERNEL(kv_pack_kernel, half_t)
FRESCO_KV_PACK_KERNEL(kv_pack_bf16_kernel, bf16_t)
#undef FRESCO_KV_PACK_KERNEL

// ---------------------------------------------------------------------------------------------
// kvproj_pack: the K | V projection of the SELECTED rows and the pack in ONE launch, for layer calls whose K and V are
// read through the cross-frame pass's key image (V by nothing else).  The two-launch form is fresco_linear with x_rows (K | V of
// the 2 x M gathered hidden rows -> HBM) then kv_pack_kernel (gather again, transpose, pad -> image), two latency-bound
// launches in front of the flash kernel.  K and V never exist in HBM here.
//
// A workgroup (5 waves) owns one CFG half, 160 output features of K OR of V (4 heads at D = 40, 2 at D = 80) and a
// contiguous range of TILES 64-key tiles:
//   * weights ONCE: a wave's 32 weight rows (all of K_in) are its MFMA fragments for the whole range and stay in registers
//     (80 VGPRs at K_in = 320, 160 at 640).  They arrive coalesced -- consecutive lanes copy consecutive 16-byte pieces of
//     a row by LDS-DMA into a wave-private staging slot (rows of 320 k at an odd 16-byte stride; two rounds at 640) and are
//     read from there in fragment order.  (The first form had every lane walk its own row straight from L2: 16 bytes of
//     64 different lines per instruction, which a CU serves at ~9 B/clk, and every one of the 264 / 136 single-tile
//     workgroups paid that for both matrices -- 10 us of its 22.)
//   * hidden rows: the 64 (K_in = 320) or 32 (640: half tiles) gathered rows of a block are copied by LDS-DMA into one of two
//     buffers, one block ahead: the gather of block u + 1 is in flight under block u's products and stores, ONE barrier per
//     block.  A DMA piece is 64 consecutive 16-byte chunks of the buffer, so the pad chunk of a row is written too (with a
//     copy of its neighbour; never read), and rows past M are copied from a valid row and zeroed on the way out.
//   * the accumulators ARE the image's pieces -- K as C[feature][key] (A = W_k, B = x: a lane's 4 consecutive features of a
//     key are 8 bytes of the key's chunk), V^T as C[key][feature] (A = x, B = W_v: a lane's registers 8 kc' .. 8 kc' + 7
//     are the 8 keys of one 16-byte V^T chunk, in the C-tile key order the flash kernel's PV product consumes).  The
//     constant parts of the image (ones column of K, ones row / zero rows of V^T) and max |k|^2 per (head, tile) are
//     written alongside (partial sums per 4 features in LDS, added in a fixed order: run-to-run identical).
// LDS: buffer 0 | staging slots (later: buffer 1, the |k|^2 parts of two tiles) | row table = 150 KB, one workgroup per CU.
// Numerics: one fp32 accumulation chain per output; MFMA step (st, i) contracts k = 64 st + 8 i + {0..7, 32..39} (the order
// of the single-tile form this replaces: same image, bit for bit).  linear_kernel uses two chains and another order, so the
// fp16 K / V values can differ from the two-launch path's in the last place; parity is against the oracle, as everywhere.
// grid (ceil(nT / TILES), 2 * H*D/160, G), 320 threads; blockIdx.y = 2 * feature group + (0: K, 1: V).
// ---------------------------------------------------------------------------------------------
template <int KIN, int D>
struct KvProjCfg {
    // key tiles per workgroup, chosen from the sweep in EXPERIMENTS.md section 7 (3 at up_blocks.3: 23 ranges x 4 x 2 = 184
    // workgroups, one round on 256 CUs; 2 would be 272.  2 at up_blocks.2: 144 workgroups; 1 would be 272)
    static constexpr int TILES = KIN == 320 ? 3 : 2;
    static constexpr int XR = 64 * 320 / KIN;    // hidden rows per block (a whole tile, or half of one)
    static constexpr int BPT = 64 / XR;          // blocks per tile
    static constexpr int NB = XR / 32;           // 32-key MFMA blocks per block
    static constexpr int CPR = KIN / 8;          // 16-byte chunks per hidden row
    static constexpr int ROWB = KIN * 2 + 16;    // LDS bytes per staged hidden row: an odd number of 16-byte chunks
    static constexpr int XPIECES = (XR * (CPR + 1) + 63) / 64;  // 1 KiB DMA pieces per buffer
    static constexpr int XBUF = XPIECES * 1024;
    static constexpr int WK = 320;               // k per weight round
    static constexpr int WROWB = WK * 2 + 16;    // LDS bytes per staged weight row: odd too
    static constexpr int WPIECES = (32 * (WK / 8 + 1) + 63) / 64;
    static constexpr int WSLOT = WPIECES * 1024;  // one wave's staging slot
    static constexpr int NWR = KIN / WK;         // weight rounds
    static constexpr int HPW = 160 / D;          // heads per workgroup
    static constexpr int NPART = D / 4;          // partial sums of |k|^2 per key and head (one per 4 features)
    static constexpr int N2P = HPW * NPART * 64; // floats per tile
    static constexpr int STAGE_BYTES = 5 * WSLOT;
    static constexpr int LDS_BYTES = XBUF + STAGE_BYTES + TILES * 64 * 4;
    static_assert(XBUF + 2 * N2P * 4 <= STAGE_BYTES, "buffer 1 and the |k|^2 parts live in the staging area");
    static_assert(KIN % WK == 0 && 64 % XR == 0 && XR % 32 == 0 && 160 % D == 0 && D % 8 == 0 && TILES >= 1, "shapes");
};

// (one body for both element types, Elem<T> of common.h: fragment types, the MFMA, the conversions and the bit pattern of 1.0
// are all that differs; grid, LDS plan, DMA ring and the counted waits are common)
template <typename T, int KIN, int D>
__device__ __forceinline__ void kvproj_pack_body(const T* x, int64_t x_ld, const int32_t* x_rows, const T* Wk, const T* Wv,
                                                 char* img, float* ktmax, int H, int M, int nT) {
    typedef typename Elem<T>::x4 X4;
    typedef typename Elem<T>::x8 X8;
    using Cfg = AttnCfg<D>;
    using PC = KvProjCfg<KIN, D>;
    constexpr int ROWB = PC::ROWB, HPW = PC::HPW, NPART = PC::NPART, CPR = PC::CPR, XR = PC::XR, NB = PC::NB, BPT = PC::BPT;
    constexpr int NKS = KIN / 16;  // MFMA k-steps
    constexpr int SK = 4;          // k-steps per 64-k stage: lane (row, hi) holds k = 64 st + 32 hi + 8 i + (0..7) for step (st, i)
    constexpr int WST = PC::WK / 64;  // stages per weight round
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* stage = smem + PC::XBUF;
    float* n2p = reinterpret_cast<float*>(stage + PC::XBUF);
    int32_t* rows = reinterpret_cast<int32_t*>(stage + PC::STAGE_BYTES);
    const int tile0 = blockIdx.x * PC::TILES, fg = blockIdx.y >> 1, g = blockIdx.z;
    const bool kv = blockIdx.y & 1;  // 0: this workgroup makes K pieces, 1: V^T pieces
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int nt = min(PC::TILES, nT - tile0);  // tiles of this range
    const int nblk = nt * BPT;
    const uint32_t lds0 = lds_addr(smem);
    const int ft = fg * 5 + wave;  // this wave's 32-feature tile
    const T* wsrc = (kv ? Wv : Wk) + (int64_t)ft * 32 * KIN;

    // one round of this wave's weight rows -> its staging slot, consecutive lanes on consecutive chunks of a row
    auto weight_dma = [&](int round) __attribute__((always_inline)) {
#pragma unroll 1  // (unrolled, hipcc keeps all 21 addresses live at once)
        for (int j = 0; j < PC::WPIECES; ++j) {
            const int c = j * 64 + lane;
            const int row = min(c / (PC::WK / 8 + 1), 31), dc = min(c % (PC::WK / 8 + 1), PC::WK / 8 - 1);
            lds_dma16(wsrc + (int64_t)row * KIN + round * PC::WK + dc * 8, lds0 + PC::XBUF + wave * PC::WSLOT + j * 1024);
        }
    };
    X8 fw[NKS];
    auto weight_frags = [&](int round) __attribute__((always_inline)) {
        const char* slot = stage + wave * PC::WSLOT + l31 * PC::WROWB + hi * 64;
#pragma unroll
        for (int s = 0; s < WST; ++s)
#pragma unroll
            for (int i = 0; i < SK; ++i)
                fw[(round * WST + s) * SK + i] = *reinterpret_cast<const X8*>(slot + s * 128 + i * 16);
    };
    // the gathered hidden rows of block u -> buffer u & 1 (buffer 1 is the head of the staging area)
    auto gather_dma = [&](int u) __attribute__((always_inline)) {
        const uint32_t dst = lds0 + (u & 1) * PC::XBUF;
#pragma unroll 1
        for (int j = wave; j < PC::XPIECES; j += 5) {
            const int c = j * 64 + lane;
            const int row = min(c / (CPR + 1), XR - 1), dc = min(c % (CPR + 1), CPR - 1);
            const int32_t r = max(rows[u * XR + row], 0);
            lds_dma16(x + (int64_t)r * x_ld + dc * 8, dst + j * 1024);
        }
    };
    // max |k|^2 of local tile tl per head: parts added in a fixed order, maximum over the 64 keys
    auto reduce_ktmax = [&](int tl) __attribute__((always_inline)) {
        if (!kv && wave < HPW) {
            const float* part = n2p + (tl & 1) * PC::N2P + wave * NPART * 64 + lane;
            float n2 = 0.f;
#pragma unroll
            for (int p_ = 0; p_ < NPART; ++p_) n2 += part[p_ * 64];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) n2 = fmaxf(n2, __shfl_xor(n2, off, 64));
            if (lane == 0) ktmax[(int64_t)(g * H + fg * HPW + wave) * nT + tile0 + tl] = n2;
        }
    };

    weight_dma(0);
    for (int i = tid; i < nt * 64; i += 320) {
        const int m = tile0 * 64 + i;
        rows[i] = m < M ? x_rows[(int64_t)g * M + m] : -1;
    }
    dma_wait_barrier<0>();  // rows[]; this wave's weight round 0 has landed
    gather_dma(0);
    weight_frags(0);
#pragma unroll
    for (int round = 1; round < PC::NWR; ++round) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot has been read
        weight_dma(round);
        dma_wait<0>();
        weight_frags(round);
    }

    // the block loop, once per role (a compile-time role: with a run-time one hipcc hoists the two branches' common fragment
    // reads, all 20 k-steps of them, in front of the branch and spills)
    auto blocks = [&](auto role) __attribute__((always_inline)) {
        constexpr bool KV = decltype(role)::value;
        for (int u = 0; u < nblk; ++u) {
            // block u's rows have landed (every wave waited for its own pieces); everyone is done with the other buffer -- and,
            // at u = 0, with the staging slots under it.  The wait is counted: the NST image stores of block u - 1 are this
            // wave's only vector-memory operations younger than its pieces of block u, and stay in flight
            // NST MUST equal the number of global store instructions the epilogue below issues per block (K: NB x 4 x4
            // stores, V: NB x 2 x8 stores) and nothing else may touch vector memory after gather_dma: with fewer stores
            // than NST the wait returns before the rows have landed.  Check the listing's vmcnt against its stores after any
            // edit of the epilogue.
            constexpr int K_STORES = NB * 4, V_STORES = NB * 2;
            constexpr int NST = KV ? V_STORES : K_STORES;
            if (u == 0) dma_wait_barrier<0>(); else dma_wait_barrier<NST>();
            if (u > 0 && u % BPT == 0) reduce_ktmax(u / BPT - 1);  // (its store: in front of the next pieces, not behind)
            if (u + 1 < nblk) gather_dma(u + 1);
            const char* xs = smem + (u & 1) * PC::XBUF + l31 * ROWB + hi * 64;
            const int tl = u / BPT, kbase = (u % BPT) * XR;
            const int32_t* trow = rows + tl * 64;
            floatx16 acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
            // the products, hidden-row fragments one group of four ahead of their MFMAs (left alone, hipcc issues
            // read -> wait -> MFMA: an LDS round trip per step)
            constexpr int GS = 4 / NB, NG = NKS / GS;  // k-steps per group, groups
            X8 xq[2][4];
            auto xfetch = [&](int q) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < GS; ++i)
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const int s = q * GS + i;
                        xq[q & 1][i * NB + b] = *reinterpret_cast<const X8*>(xs + b * 32 * ROWB + (s / SK) * 128 + (s % SK) * 16);
                    }
            };
            xfetch(0);
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                if (q + 1 < NG) xfetch(q + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < GS; ++i)
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const X8 xb = xq[q & 1][i * NB + b], wf = fw[q * GS + i];
                        acc[b] = KV ? Elem<T>::mfma32x32x16(xb, wf, acc[b]) : Elem<T>::mfma32x32x16(wf, xb, acc[b]);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
            // (the image addresses below are loop-invariant per lane; hoisted out of the block loop they cost more registers
            // than the K_in = 320 budget has left.  Laundering the lane coordinates keeps them inside the iteration.)
            int l31e = l31, hie = hi;
            asm volatile("" : "+v"(l31e), "+v"(hie));
            if (!KV) {
                // ---- K pieces: lane (key l31 of block b, hi), registers 4j .. 4j+3 = features 32 ft + 8 j + 4 hi + (0..3)
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const int key = kbase + b * 32 + l31e;
                    const bool real = trow[key] >= 0;
#pragma unroll
                    for (int j = 0; j < K_STORES / NB; ++j) {  // one store each: K_STORES per block
                        const int f0 = ft * 32 + 8 * j + 4 * hie;
                        const int head = f0 / D, dd = f0 - head * D;
                        X4 w;
                        float n2 = 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            w[e] = real ? (T)acc[b][4 * j + e] : (T)0;
                            n2 = fmaf((float)w[e], (float)w[e], n2);
                        }
                        char* dst = img + ((int64_t)(g * H + head) * (nT + 1) + tile0 + tl) * Cfg::TILE;
                        *reinterpret_cast<X4*>(dst + ((dd >> 3) * 64 + key) * 16 + (dd & 7) * 2) = w;
                        n2p[(tl & 1) * PC::N2P + ((head - fg * HPW) * NPART + (dd >> 2)) * 64 + key] = n2;
                    }
                }
            } else {
                // ---- V^T pieces: lane (feature 32 ft + l31, hi), registers 8 kq .. 8 kq + 7 = keys of chunk (kc, cc = hi)
                const int f = ft * 32 + l31e;
                const int head = f / D, d = f - head * D;
                char* dst = img + ((int64_t)(g * H + head) * (nT + 1) + tile0 + tl + 1) * Cfg::TILE + Cfg::KTILE;
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int kq = 0; kq < V_STORES / NB; ++kq) {  // one store each: V_STORES per block
                        const int kc = kbase / 16 + 2 * b + kq;
                        X8 w;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int key = kc * 16 + (e & 3) + 8 * (e >> 2) + 4 * hie;
                            w[e] = trow[key] >= 0 ? (T)acc[b][8 * kq + e] : (T)0;
                        }
                        *reinterpret_cast<X8*>(dst + ((kc * 2 + hie) * Cfg::DPV + d) * 16) = w;
                    }
            }
        }
    };
    if (kv) blocks(std::true_type{}); else blocks(std::false_type{});
    // ---- constant parts of the image for this workgroup's heads and tiles: the K pads by the K workgroup, V^T's by V's
    {
        constexpr int KPAD = (Cfg::DPK - D) / 8;         // pad chunks of K per key (the first one carries the ones column)
        constexpr int VPAD = Cfg::DPV - D;               // pad rows of V^T (the first one is all ones)
        const int per_head = kv ? VPAD * 8 : KPAD * 64;
        for (int i = tid; per_head > 0 && i < nt * HPW * per_head; i += 320) {
            const int c = i % per_head, hl = (i / per_head) % HPW, tl = i / (per_head * HPW);
            const int head = fg * HPW + hl;
            const int32_t* trow = rows + tl * 64;
            char* base = img + ((int64_t)(g * H + head) * (nT + 1) + tile0 + tl) * Cfg::TILE;
            if (!kv) {
                const int pc = c / 64, key = c % 64;
                uint4 val = make_uint4(0, 0, 0, 0);
                if (Cfg::MCOL && pc == 0 && trow[key] >= 0) val.x = Elem<T>::ONE_BITS;  // K[key][D] = 1.0 (running max rides in the QK MFMA)
                *reinterpret_cast<uint4*>(base + ((D / 8 + pc) * 64 + key) * 16) = val;
            } else {
                const int pr = c / 8, kcc = c % 8;       // pad row, (kc, cc) chunk
                const int kc = kcc >> 1, cc = kcc & 1;
                X8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int key = kc * 16 + (e & 3) + 8 * (e >> 2) + 4 * cc;
                    o[e] = (Cfg::ONES && pr == 0 && trow[key] >= 0) ? (T)1 : (T)0;
                }
                *reinterpret_cast<X8*>(base + Cfg::TILE + Cfg::KTILE + (kcc * Cfg::DPV + D + pr) * 16) = o;
            }
        }
    }
    __syncthreads();
    reduce_ktmax(nt - 1);
}

// __launch_bounds__' second argument is used as a REGISTER CAP here, not as an occupancy: by its LDS one workgroup fits a CU at
// either width (5 waves on 4 SIMDs: at most 2 per SIMD).  "3" at K_in = 320 means <= 168 registers, the budget
// tests/test_kernel_resources.py pins for this instantiation, and the build sits exactly on it (80 weight + 32 accumulator
// + 32 hidden-row fragment registers + addresses; the lane coordinates of the epilogue are laundered to keep its addresses
// out of the loop-invariant set): an edit that adds live registers will spill -- that test says so.  "2" at 640: <= 256 (228).
// The bf16 instantiations take the same caps (tests/test_kernel_resources_kvproj_bf16.py; counts in EXPERIMENTS.md section 8).
template <int KIN, int D>
__global__ __launch_bounds__(320, KIN == 320 ? 3 : 2) void kvproj_pack_kernel(const half_t* __restrict__ x, int64_t x_ld,
                                                             const int32_t* __restrict__ x_rows,
                                                             const half_t* __restrict__ Wk,
                                                             const half_t* __restrict__ Wv, char* __restrict__ img,
                                                             float* __restrict__ ktmax, int H, int M, int nT) {
    kvproj_pack_body<half_t, KIN, D>(x, x_ld, x_rows, Wk, Wv, img, ktmax, H, M, nT);
}
template <int KIN, int D>
__global__ __launch_bounds__(320, KIN == 320 ? 3 : 2) void kvproj_pack_bf16_kernel(const bf16_t* __restrict__ x, int64_t x_ld,
                                                                  const int32_t* __restrict__ x_rows,
                                                                  const bf16_t* __restrict__ Wk,
                                                                  const bf16_t* __restrict__ Wv, char* __restrict__ img,
                                                                  float* __restrict__ ktmax, int H, int M, int nT) {
    kvproj_pack_body<bf16_t, KIN, D>(x, x_ld, x_rows, Wk, Wv, img, ktmax, H, M, nT);
}
template <typename T, int KIN, int D>
static auto kvproj_pack_kernel_of() {
    if constexpr (std::is_same<T, bf16_t>::value)
        return &kvproj_pack_bf16_kernel<KIN, D>;
    else
        return &kvproj_pack_kernel<KIN, D>;
}

// ---------------------------------------------------------------------------------------------
// flash attention: grid (H * nQblk * B), 512 threads = 8 waves x QB blocks of 32 query rows
// blockIdx.x = (b * nQblk + qblk) * H + h   -> head h lands on XCD (h % 8): each XCD's L2 holds
// only its own heads' packed key images.
//
// Two waves share every SIMD, and what they share is the matrix pipe and the VALU port: left alone, the two
// run their MFMA phases together (each at half rate) and then their softmax phases together, in lockstep
// (measured: MFMA time + softmax time, no overlap).  So the workgroup is two groups of four waves (one per
// SIMD each) that are held half a tile apart by WHERE in the tile they execute the workgroup's one barrier:
//     group A:  softmax(u) | barrier | PV(u)  QK(u+1)            -> its MFMA block follows the barrier
//     group B:  barrier | softmax(u)  PV(u)  QK(u+1)             -> its softmax follows the barrier
// between two barriers a SIMD sees [A: 28 MFMAs || B: exp/cvt] and then [A: exp/cvt || B: 28 MFMAs].  The
// softmax block (64 exp + 32 cvt, plus the issue slots the partner's MFMAs take) is a little shorter than the
// MFMA block (28 x 32 cycles), so the matrix pipe is the pacing resource of both halves.
//
// Key tiles: pack p of the image = K fragments of tile p ‖ V^T fragments of tile p-1, what step u = p-1 of the
// loop reads (PV(u), QK(u+1)).  Packs arrive by DMA into a 4-slot LDS ring, three steps ahead; a wave waits for
// its own pieces of the pack after next (counted vmcnt) before the barrier, so every fragment read finds its
// data landed one barrier earlier and no MFMA waits on global memory.
// ---------------------------------------------------------------------------------------------
// a, b = this lane's value and lane (l ^ 32)'s, in either order: v_permlane32_swap (VALU) instead of a ds_bpermute
// through the LDS pipe (the builtin inserts the wait state the swap needs)
__device__ __forceinline__ void both_halves(float v, float& a, float& b) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    a = __builtin_bit_cast(float, (unsigned)sw[0]);
    b = __builtin_bit_cast(float, (unsigned)sw[1]);
}
// a row maximum over both half-waves: each holds 32 of the query's 64 keys of a tile
__device__ __forceinline__ float max_both_halves(float v) {
    float a, b;
    both_halves(v, a, b);
    return fmaxf(a, b);
}

// The pack ring of a workgroup (head h of key group g): a pack IS its LDS image, so it is NP linear 1 KiB copies
// (lds_dma.h); wave w issues pieces w, w + 8, ... (destination = wave-uniform base + lane * 16, source = scalar base + one
// per-lane offset).  Ordering is by the counted waits + barrier of the bodies' `ring_sync`.
template <int D>
struct PackRing {
    using Cfg = AttnCfg<D>;
    static constexpr int NPW_LO = Cfg::NP / 8, NPW_HI = (Cfg::NP + 7) / 8, NREM = Cfg::NP % 8;
    const int wave_s;
    const int many;  // this wave issues NPW_HI pieces per pack (else NPW_LO)
    const uint32_t lds0;
    const char* const src;
    const uint32_t lane_off;
    __device__ __forceinline__ PackRing(const char* img, int g, int H, int h, int nT, const char* smem, int wave_s_,
                                        int tid)
        : wave_s(wave_s_), many(wave_s_ < NREM ? 1 : 0), lds0(lds_addr(smem)),
          src(img + (int64_t)(g * H + h) * (nT + 1) * Cfg::TILE), lane_off(tid * 16) {}
    __device__ __forceinline__ void stage(int p, int slot) const {  // pack p -> ring slot
        const char* sp = src + (int64_t)p * Cfg::TILE;
        const uint32_t dstb = lds0 + slot * Cfg::TILE + wave_s * 1024;
#pragma unroll
        for (int i = 0; i < NPW_HI; ++i) {
            if (i < NPW_LO || many) {
                lds_dma16(lane_off, sp, dstb + i * 8192);
                sp += 8192;
            }
        }
    }
    // wait until at most `keep` of this wave's newest packs are still in flight, then the workgroup barrier
    __device__ __forceinline__ void wait_barrier(int keep) const { dma_wait_barrier_keep<NPW_LO, NPW_HI>(keep, many); }
};

// ---- epilogue: normalise, store O[q][h*D + d]  (row0 = b * Lq; l_run is read only where V^T has no ones row)
template <typename T, int D, int QB>
__device__ __forceinline__ void flash_store(const floatx16 (&o)[QB][AttnCfg<D>::NDB], const float (&l_run)[QB],
                                            T* __restrict__ out, int64_t row0, int Lq, int C, int h, int qrow0,
                                            int l31, int hi) {
    using Cfg = AttnCfg<D>;
    typedef typename Elem<T>::x4 X4;
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        float l_tot;
        if (Cfg::ONES) {
            // O^T row D: C-tile row rr = D % 32 lives in register (rr&3) + 4*(rr>>3) of lanes with hi = (rr>>2)&1
            constexpr int rr = D % 32;
            l_tot = __shfl(o[j][D / 32][(rr & 3) + 4 * (rr >> 3)], l31 + 32 * ((rr >> 2) & 1), 64);
        } else {
            l_tot = l_run[j] + __shfl_xor(l_run[j], 32, 64);
        }
        const float inv = 1.f / l_tot;
        const int qr = qrow0 + 32 * j;
        // A row's 8-column groups sit split over the two half-waves (lane l31: columns 8k .. 8k+3, lane
        // l31 + 32: 8k+4 .. 8k+7).  One v_permlane32_swap per dword of a PAIR of groups leaves lanes 0-31 with the 16
        // contiguous bytes of group k and lanes 32-63 with those of group k+1: one 16-byte store per pair instead of
        // two 8-byte ones (the store tail of a row-per-lane epilogue is bound by store instructions, not bytes).
        {
            T* op = out + (row0 + (qr < Lq ? qr : 0)) * C + h * D;
#pragma unroll
            for (int db = 0; db < Cfg::NDB; ++db)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    const int dA = db * 32 + gp * 16;  // first column of the pair
                    if (dA >= D) continue;
                    X4 wa, wb;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        wa[jj] = (T)(o[j][db][(2 * gp) * 4 + jj] * inv);
                        wb[jj] = (T)(o[j][db][(2 * gp + 1) * 4 + jj] * inv);
                    }
                    if (dA + 8 < D) {
                        const u32x2 a = __builtin_bit_cast(u32x2, wa), bb = __builtin_bit_cast(u32x2, wb);
                        const auto s0 = __builtin_amdgcn_permlane32_swap(a[0], bb[0], false, false);
                        const auto s1 = __builtin_amdgcn_permlane32_swap(a[1], bb[1], false, false);
                        u32x4 st;
                        st[0] = s0[0]; st[1] = s1[0]; st[2] = s0[1]; st[3] = s1[1];
                        if (qr < Lq) *reinterpret_cast<u32x4*>(op + dA + hi * 8) = st;
                    } else if (qr < Lq) {  // a lone 8-column group (D % 16 == 8): the two 8-byte halves as before
                        *reinterpret_cast<X4*>(op + dA + hi * 4) = wa;
                    }
                }
        }
    }
}

// <D, QB> pairs that run flash_body_halves (below) instead of flash_body
template <int D, int QB>
struct FlashHalves : std::integral_constant<bool, D == 80 && QB == 2> {};

// The body of one workgroup: head h, batch row b, query rows [qblk * 256 QB, (qblk + 1) * 256 QB).
template <typename T, int D, int QB>
__device__ __forceinline__ void flash_body(const T* __restrict__ q, const char* __restrict__ img,
                                           const float* __restrict__ ktmax, T* __restrict__ out, int H, int Lq,
                                           int M, int nT, int batch_per_group, float scale_log2,
                                           float diag_bias_log2, int64_t q_ld, int h, int qblk, int b, int tid) {
    using Cfg = AttnCfg<D>;
    typedef typename Elem<T>::x8 X8;
    constexpr bool FOLD = FoldCfg<T>::ENABLE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ROWS = 256 * QB;  // query rows per workgroup
    const int g = b / batch_per_group;
    const int C = H * D;

    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow0 = qblk * ROWS + wave * 32 * QB + l31;  // row of query block 0; block j: + 32*j
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int grpB = wave_s >= 4 ? 1 : 0;  // (flags are ints from scalar values: the branches on them stay scalar)

    // Q fragments (B operand of S^T = K Q^T), resident for the whole kernel
    X8 qf[QB][Cfg::NKS];
    float q2[QB];  // |q|^2 of this lane's query
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        const int qr = qrow0 + 32 * j;
        const T* qp = q + ((int64_t)b * Lq + (qr < Lq ? qr : Lq - 1)) * q_ld + h * D;
        q2[j] = 0.f;
#pragma unroll
        for (int ks = 0; ks < Cfg::NKS; ++ks) {
            const int d0 = ks * 16 + hi * 8;
            X8 t = {0, 0, 0, 0, 0, 0, 0, 0};
            if (d0 < D) t = *reinterpret_cast<const X8*>(qp + d0);
#pragma unroll
            for (int e = 0; e < 8; ++e) q2[j] = fmaf((float)t[e], (float)t[e], q2[j]);
            qf[j][ks] = t;
        }
        q2[j] += __shfl_xor(q2[j], 32, 64);
    }

    // Cauchy-Schwarz: every logit of this lane's query is bounded by |q| max|k| (max|k|^2 per key tile comes
    // from kv_pack).  Two per-wave decisions hang on it:
    //  * FOLDED scale: the exponent scale c = softmax scale * log2 e is multiplied into Q once (one fp16
    //    rounding of c*q) and the MFMA delivers exponent arguments directly.  That rounding perturbs an
    //    exponent by at most 2^-12 * c|q||k|: at FOLD_MAX = 24 a WORST-CASE 0.6 % of P, ~12 x P's own fp16 rounding.
    //    The limit is therefore empirical, not derived: tools/fold_margin.py emulates the kernel's arithmetic and
    //    finds the folded form at 0.30 of the 1e-3 parity bar for N(0,1) keys and at the exact form's error for keys
    //    aligned to the query (attn_cfg.h); test_attention_fold_limit_structured covers non-Gaussian q, k (a few
    //    dominant channels, correlated q / k) at the limit.  Beyond FOLD_MAX Q stays exact and every score is
    //    multiplied by c in fp32.
    //  * no running-max search (nomax, below) when the bound cannot leave fp16 range.
    // Accumulator units u: exponent argument = cmul * u, with (qs, cmul) = (c, 1) folded or (1, c) exact.
    float kmax;
    {
        const float* km = ktmax + (int64_t)(g * H + h) * nT;
        float k2 = 0.f;
        for (int i = lane; i < nT; i += 64) k2 = fmaxf(k2, km[i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) k2 = fmaxf(k2, __shfl_xor(k2, off, 64));
        kmax = sqrtf(k2);
    }
    bool fold_ok = true;
#pragma unroll
    for (int j = 0; j < QB; ++j) fold_ok = fold_ok && (scale_log2 * sqrtf(q2[j]) * kmax <= FOLD_MAX);
    // (flags are ints read from scalar values: the branches on them stay scalar branches)
    // (bf16 never folds, FoldCfg in attn_cfg.h: the folded passes are compiled out and every score is scaled in fp32)
    const int folded = FOLD ? __builtin_amdgcn_readfirstlane((int)__all(fold_ok)) : 0;
    const float qs = folded ? scale_log2 : 1.f;
    const float cmul = folded ? 1.f : scale_log2;
    float qbound[QB];  // bound on the accumulators (units u), with a margin for the roundings above
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        qbound[j] = qs * sqrtf(q2[j]) * kmax * 1.001f + 1e-3f;
        if (folded) {
#pragma unroll
            for (int ks = 0; ks < Cfg::NKS; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[j][ks][e] = (T)((float)qf[j][ks][e] * scale_log2);
        }
    }
    const float resc_thr = RESCALE_THR / cmul;  // thresholds and the diagonal bias in accumulator units
    const float diag_u = diag_bias_log2 / cmul;

    // ---- staging: global -> LDS by DMA, no register round trip
    const PackRing<D> ring(img, g, H, h, nT, smem, wave_s, tid);

    floatx16 o[QB][Cfg::NDB];
    // The accumulators must come out as  c*s - m_run  (no per-score subtraction).  MCOL: -m_run rides in Q's
    // spare column D against the ones column of the packed K (m_run is kept on the fp16 grid so that the
    // value the MFMA subtracts is exactly the one the rescale factors are computed from).  Otherwise
    // -m_run sits in all 16 registers of `negm`, the C operand of the first QK MFMA.
    constexpr int MKS = Cfg::MCOL ? D / 16 : 0, MHI = (D % 16) / 8, ME = D % 8;
    floatx16 negm[QB];
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        m_run[j] = 0.f;  // reference point of the exponent (log2 domain); tile 0 moves it to the row max
        l_run[j] = 0.f;  // row sum when V^T has no spare row for the ones-trick (this lane's keys)
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[j][r] = 0.f;
#pragma unroll
        for (int db = 0; db < Cfg::NDB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[j][db][r] = 0.f;
    }

    // per-lane fragment offset inside a ring slot (K: + (ks*128 + kb*32)*16; V^T: + KTILE + (kc*2*DPV + db*32)*16)
    const int koff = (hi * 64 + l31) * 16;
    const int voff = Cfg::KTILE + (hi * Cfg::DPV + l31) * 16;
    auto read_k = [&](X8 (&kf)[2][Cfg::NKS], int slot) __attribute__((always_inline)) {
        const char* kb_ = smem + slot * Cfg::TILE + koff;
#pragma unroll
        for (int ks = 0; ks < Cfg::NKS; ++ks)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
                kf[kb][ks] = *reinterpret_cast<const X8*>(kb_ + (ks * 128 + kb * 32) * 16);
    };

    floatx16 s[QB][2];  // S^T of the tile whose softmax comes next
    auto qk = [&](X8 (&kf)[2][Cfg::NKS]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < QB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[j][0][r] = Cfg::MCOL ? 0.f : negm[j][r];
                s[j][1][r] = Cfg::MCOL ? 0.f : negm[j][r];
            }
#pragma unroll
        for (int ks = 0; ks < Cfg::NKS; ++ks)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    s[j][kb] = Elem<T>::mfma32x32x16(kf[kb][ks], qf[j][ks], s[j][kb]);
                }
    };

    // ---- prologue: packs 0 .. 3 in flight (pack p = step p-1, slot (p+3) & 3), packs 0 and 1 landed,
    // S^T of tile 0 computed
    ring.stage(0, 3);
    ring.stage(1, 0);
    if (nT > 1) ring.stage(2, 1);
    if (nT > 2) ring.stage(3, 2);
    ring.wait_barrier(nT > 2 ? 2 : (nT > 1 ? 1 : 0));
    {
        X8 kf[2][Cfg::NKS];
        read_k(kf, 3);
        qk(kf);
    }
    __builtin_amdgcn_sched_barrier(0);

    const int need_diag = diag_bias_log2 != 0.f ? 1 : 0;

    // Step u: softmax of tile u, O^T += V^T(u) P^T(u), S^T(u+1) = K(u+1) Q^T.  One loop body; what differs
    // between tiles and waves is three wave-uniform (scalar-branch) passes in front of the exponentials:
    //  * fix   : per-element fix-ups -- padded keys of the last tile, diagonal bias (then on every tile);
    //  * search: running-max search + deferred rescale.  Dropped (nomax) after tile 0 has anchored m_run when
    //            `qbound` proves that no exponent argument can exceed NOMAX_THR: P is then at most
    //            2^NOMAX_THR, inside fp16 range, and the row sum normalises it exactly as before;
    //  * exact : the wave keeps Q unscaled: scores are multiplied by c in fp32 before the exponential.
    // LAST = the final tile: no S^T to compute for a next one.
    // FAST = the common case as an instantiation of its own: no fix-ups (only the max search and the exact-scale
    // pass keep their scalar branches), and (u + 3 < nT) so that the ring handling is unconditional.  (A taken scalar branch costs a wave an
    // instruction-fetch bubble; the generic body skips over its rare passes with a dozen of them per tile.)
    int nomax = 0;
    auto step = [&](int u, auto last_c, auto fast_c) __attribute__((always_inline)) {
        constexpr bool LAST = decltype(last_c)::value;
        constexpr bool FAST = decltype(fast_c)::value;
        const int slot = u & 3;
        const int fix = FAST ? 0 : (LAST ? 1 : need_diag);
        const int search = !nomax;
        const int exact = !folded;
        // barrier u: pack u+2 (step u+1) has landed for everyone; its predecessor's slot takes pack u+4
        auto ring_sync = [&]() __attribute__((always_inline)) {
            if (FAST) {
                dma_wait_barrier<PackRing<D>::NPW_LO>();  // (waves with an extra piece per pack wait for one piece more)
                ring.stage(u + 4, (u + 3) & 3);
            } else {
                ring.wait_barrier(u + 2 < nT ? 1 : 0);
                if (u + 3 < nT) ring.stage(u + 4, (u + 3) & 3);
            }
        };
        if (grpB) ring_sync();
        __builtin_amdgcn_sched_barrier(0);

        // ---- V^T fragments of tile u -> registers (landed one barrier ago), in flight under the softmax
        X8 vf[4][Cfg::NDB];
        {
            const char* vb_ = smem + slot * Cfg::TILE + voff;
#pragma unroll
            for (int kc = 0; kc < 4; ++kc)
#pragma unroll
                for (int db = 0; db < Cfg::NDB; ++db)
                    vf[kc][db] = *reinterpret_cast<const X8*>(vb_ + (kc * 2 * Cfg::DPV + db * 32) * 16);
        }
        __builtin_amdgcn_sched_barrier(0);

        // ---- online softmax, one query per lane; the packed P registers are the PV B operands
        X8 pf[QB][4];
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            if (fix) {
                const int qr = qrow0 + 32 * j;
                int kbase = u * 64 + 4 * hi;
                asm volatile("" : "+v"(kbase));  // keeps the index arithmetic of this rare pass inside its branch
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key0 = kbase + (r & 3) + 8 * (r >> 2);
                    if (need_diag && key0 == qr) s[j][0][r] += diag_u;
                    if (need_diag && key0 + 32 == qr) s[j][1][r] += diag_u;
                    if (key0 >= M) s[j][0][r] = -1e30f;
                    if (key0 + 32 >= M) s[j][1][r] = -1e30f;
                }
            }
            // s = exponent argument (units u) relative to m_run; the reference point moves (and O, l are
            // rescaled) only when the tile max exceeds it by more than RESCALE_THR -- or on tile 0, which
            // anchors it at the row's first-tile max.
            if (search) {
                float mt = fmaxf(s[j][0][0], s[j][1][0]);
#pragma unroll
                for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[j][0][r]), s[j][1][r]);  // v_max3_f32
                mt = max_both_halves(mt);  // the other half of the wave holds the query's other 32 keys of the tile
                if (u == 0 || __builtin_amdgcn_readfirstlane((int)__any(mt > resc_thr)) != 0) {
                    float delta = (u == 0) ? mt : fmaxf(mt, 0.f);
                    if (Cfg::MCOL) {
                        // stays representable in T (and finite: logits beyond +-6e4 units saturate)
                        const float m_new = (float)(T)fminf(fmaxf(m_run[j] + delta, -6.0e4f), 6.0e4f);
                        delta = m_new - m_run[j];
                        m_run[j] = m_new;
                        const T nm = (T)(-m_new);
                        qf[j][MKS][ME] = (hi == MHI) ? nm : qf[j][MKS][ME];
                    } else {
                        m_run[j] += delta;
                    }
                    const float alpha = __builtin_amdgcn_exp2f(-delta * cmul);
                    l_run[j] *= alpha;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if (!Cfg::MCOL) negm[j][r] = -m_run[j];
                        s[j][0][r] -= delta;
                        s[j][1][r] -= delta;
                    }
#pragma unroll
                    for (int db = 0; db < Cfg::NDB; ++db)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[j][db][r] *= alpha;
                }
            }
            if (exact) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[j][0][r] *= cmul;
                    s[j][1][r] *= cmul;
                }
            }
            float psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const float p0 = __builtin_amdgcn_exp2f(s[j][kb][r]);
                    const float p1 = __builtin_amdgcn_exp2f(s[j][kb][r + 1]);
                    if (!Cfg::ONES) psum += p0 + p1;
                    pf[j][kb * 2 + (r >> 3)][r & 7] = (T)p0;
                    pf[j][kb * 2 + (r >> 3)][(r & 7) + 1] = (T)p1;
                }
            if (!Cfg::ONES) l_run[j] += psum;
            // (pins the exponentials in front of group A's barrier below: being free of side effects they would
            // otherwise be sunk behind the inline-asm barrier, into the MFMA block)
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) asm volatile("" : "+v"(pf[j][kc]));
        }
        __builtin_amdgcn_sched_barrier(0);

        if (!grpB) ring_sync();
        __builtin_amdgcn_sched_barrier(0);

        // ---- K fragments of tile u+1 (same pack), in flight under the PV MFMAs
        X8 kf[2][Cfg::NKS];
        if (!LAST) read_k(kf, slot);
        __builtin_amdgcn_sched_barrier(0);

        // The MFMA block runs at raised priority: against a partner wave in its softmax, an MFMA wave that loses the
        // issue arbitration (it does when it is the younger one) leaves the matrix pipe idle between MFMAs
        // (tools/ubench_rates.hip: 28 MFMAs beside a prioritised exp/cvt stream take 1590 cycles instead of 900).
        __builtin_amdgcn_s_setprio(1);
        // ---- O^T += V^T P^T  (row D of V^T is all ones when it is spare: O^T[D] = row sum)
#pragma unroll
        for (int kc = 0; kc < 4; ++kc)
#pragma unroll
            for (int db = 0; db < Cfg::NDB; ++db)
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    o[j][db] = Elem<T>::mfma32x32x16(vf[kc][db], pf[j][kc], o[j][db]);
                }
        __builtin_amdgcn_sched_barrier(0);
        // ---- S^T of tile u+1
        if (!LAST) qk(kf);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };

    const std::integral_constant<bool, true> yes;
    const std::integral_constant<bool, false> no_last, no;
    const std::integral_constant<bool, true> fast;
    {
        int u = 0;
        if (nT > 1) {
            step(0, no_last, no);
            u = 1;
            if (!need_diag) {
                bool safe = true;
#pragma unroll
                for (int j = 0; j < QB; ++j) safe = safe && (cmul * (qbound[j] - m_run[j]) <= NOMAX_THR);
                nomax = __builtin_amdgcn_readfirstlane((int)__all(safe));
            }
            if (!need_diag)
                for (; u + 3 < nT; ++u) step(u, no_last, fast);
            for (; u < nT - 1; ++u) step(u, no_last, no);
        }
        nomax = 0;  // the last tile has padded keys at -1e30: its maximum must be looked at
        step(u, yes, no);
    }

    flash_store<T, D, QB>(o, l_run, out, (int64_t)b * Lq, Lq, C, h, qrow0, l31, hi);
}

// ---------------------------------------------------------------------------------------------
// Two query blocks per wave where a whole tile's fragments no longer fit beside them (D = 80: O alone is 96 registers).
// flash_body holds a 64-key tile per step: S 32 QB, P 16 QB, V^T 48, K 40 -- at QB = 2 that is past 256.  Here the
// loop runs in HALF tiles of 32 keys with the same phase structure and the same ping-pong:
//     phase (u, f):  [V^T fragments of keys 32 f .. 32 f + 31 of tile u | exp, pack S -> P]  barrier (group A; B has it in front)
//                    [K fragments of the NEXT 32 keys | O^T += V^T P^T (2 k-steps), S^T of the next 32 keys]
// so S is 32 registers, P 16 (packed into S's), the fragments of a phase 24 + 20, every fragment feeds two MFMAs, and a
// 512-row workgroup makes the up_blocks.2 launch one round of 256.  With O 96, Q 40 and the two -m_run splats that hipcc
// keeps as the C operands of the QK chains (32: no v_mov per tile) the kernel is at 251 registers, nothing in scratch.  Key order and k-step order of both products are flash_body's: per output
// element the accumulation order is the same, and on operands that take this path the result is bit-equal to <D, 1>'s.
//
// Ring: packs are the same (K(p) || V^T(p - 1)).  Phase (u, 0) reads K of tile u's second half from pack u, one pack
// behind the one the step reads, so pack u's slot is refilled (pack u + 4) after barrier (u, 1) instead of barrier u:
// by then both groups are through the MFMA block of phase (u, 0).  Barrier (u, 0) keeps the counted wait (pack u + 2
// landed), 2.5 steps ahead of its first reader.
//
// Only the common case lives here: scale folded, no max search after tile 0, no diagonal bias, two tiles or more.  The
// rare passes would need `negm` (32 registers) and their branches in this body, so the WORKGROUP votes after tile 0's
// scores: all eight waves common-case -> this body; otherwise flash_body<D, 1> runs once per 256-row half over the same
// ring (a workgroup-level choice: all waves share one staging protocol).  The last tile (padded keys, and the max
// looked at again as flash_body does) is handled as a whole tile: Q is dead by then and S of both halves fits.
// bf16 (FoldCfg: no fold at all) runs the same body with Q exact and every score multiplied by c in fp32 in front of its
// exponential; "common case" then means no max search after tile 0, no diagonal bias, two tiles or more.
// ---------------------------------------------------------------------------------------------
// Cross-lane reads without a lane-index register (__shfl_xor keeps one per distance; flash_body_halves has none to
// spare and would share them with the flash_body it falls back to): the value of lane (l ^ X), X < 32, by ds_swizzle,
// and that of lane (l ^ 32) by v_permlane32_swap (both_halves, above).
template <int X>
__device__ __forceinline__ float lane_xor(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (X << 10) | 0x1f));
}

template <typename T, int D>
__device__ __forceinline__ void flash_body_halves(const T* __restrict__ q, const char* __restrict__ img,
                                                  const float* __restrict__ ktmax, T* __restrict__ out, int H,
                                                  int Lq, int M, int nT, int batch_per_group, float scale_log2,
                                                  float diag_bias_log2, int64_t q_ld, int h, int qblk, int b) {
    using Cfg = AttnCfg<D>;
    typedef typename Elem<T>::x8 X8;
    constexpr bool FOLD = FoldCfg<T>::ENABLE;
    static_assert(!Cfg::MCOL && Cfg::ONES, "head dims with a spare V^T row and no spare K column (D = 80)");
    constexpr int NKS = Cfg::NKS, NDB = Cfg::NDB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = b / batch_per_group;
    const int C = H * D;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow0 = qblk * 512 + wave * 64 + l31;  // row of query block 0; block 1: + 32
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int grpB = wave_s >= 4 ? 1 : 0;

    // Q fragments, scaled as if folded (a wave that may not fold sends the workgroup to flash_body, which reloads them)
    X8 qf[2][NKS];
    float q2[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int qr = qrow0 + 32 * j;
        const T* qp = q + ((int64_t)b * Lq + (qr < Lq ? qr : Lq - 1)) * q_ld + h * D;
        q2[j] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const X8 t = *reinterpret_cast<const X8*>(qp + ks * 16 + hi * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) q2[j] = fmaf((float)t[e], (float)t[e], q2[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[j][ks][e] = FOLD ? (T)((float)t[e] * scale_log2) : t[e];
        }
        float qa, qb;
        both_halves(q2[j], qa, qb);
        q2[j] = qa + qb;
    }
    float kmax;
    {
        const float* km = ktmax + (int64_t)(g * H + h) * nT;
        float k2 = 0.f;
        for (int i = lane; i < nT; i += 64) k2 = fmaxf(k2, km[i]);
        k2 = fmaxf(k2, lane_xor<16>(k2));
        k2 = fmaxf(k2, lane_xor<8>(k2));
        k2 = fmaxf(k2, lane_xor<4>(k2));
        k2 = fmaxf(k2, lane_xor<2>(k2));
        k2 = fmaxf(k2, lane_xor<1>(k2));
        kmax = sqrtf(max_both_halves(k2));
    }
    bool common = diag_bias_log2 == 0.f && nT >= 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) common = common && (!FOLD || scale_log2 * sqrtf(q2[j]) * kmax <= FOLD_MAX);
    // exponent argument = cmul * accumulator: T that never folds keeps Q exact and scales every score in fp32, as
    // flash_body's exact pass does (m_run, the chains' start values and the thresholds are then in accumulator units)
    const float cmul = FOLD ? 1.f : scale_log2;

    // ---- staging (flash_body's; the fallback below constructs its own ring over the same slots)
    const PackRing<D> ring(img, g, H, h, nT, smem, wave_s, tid);

    const int koff = (hi * 64 + l31) * 16;
    const int voff = Cfg::KTILE + (hi * Cfg::DPV + l31) * 16;
    floatx16 s[2];  // S^T of the 32 keys whose softmax comes next
    // S^T of keys 32 f .. 32 f + 31 of the tile whose K sits in `slot`; the chains start at c0 / c1
    auto qk_half = [&](floatx16 (&acc)[2], int slot, int f, float c0, float c1) __attribute__((always_inline)) {
        X8 kf[NKS];
        const char* kb_ = smem + slot * Cfg::TILE + koff + f * 512;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) kf[ks] = *reinterpret_cast<const X8*>(kb_ + ks * 2048);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[0][r] = c0;
            acc[1][r] = c1;
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[j] = Elem<T>::mfma32x32x16(kf[ks], qf[j][ks], acc[j]);
    };

    // ---- prologue: packs 0 .. 3 in flight, packs 0 and 1 landed; tile 0's row max (flash_body's anchor of m_run) from
    // both halves of its scores, the first half's kept in `s`
    ring.stage(0, 3);
    ring.stage(1, 0);
    if (nT > 1) ring.stage(2, 1);
    if (nT > 2) ring.stage(3, 2);
    ring.wait_barrier(nT > 2 ? 2 : (nT > 1 ? 1 : 0));
    float m_run[2];
    {
        floatx16 t[2];
        qk_half(t, 3, 1, 0.f, 0.f);
        qk_half(s, 3, 0, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float mt = fmaxf(s[j][0], t[j][0]);
#pragma unroll
            for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[j][r]), t[j][r]);
            m_run[j] = max_both_halves(mt);
            // flash_body's nomax test (folded: accumulator units are exponent units)
            if constexpr (FOLD)
                common = common && (scale_log2 * sqrtf(q2[j]) * kmax * 1.001f + 1e-3f - m_run[j] <= NOMAX_THR);
            else
                common = common && (cmul * (sqrtf(q2[j]) * kmax * 1.001f + 1e-3f - m_run[j]) <= NOMAX_THR);
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- the vote
    {
        int* votes = reinterpret_cast<int*>(smem + Cfg::LDS_BYTES);
        const int mine = __builtin_amdgcn_readfirstlane((int)__all(common));
        if (lane == 0) votes[wave] = mine;
        __syncthreads();
        int all = 1;
#pragma unroll
        for (int w = 0; w < 8; ++w) all &= votes[w];
        if (__builtin_amdgcn_readfirstlane(all) == 0) {
#pragma nounroll
            for (int half = 0; half < 2; ++half) {
                dma_wait_barrier<0>();  // the ring is idle: every pack in flight has landed, nobody reads
                // (thread and block indices go in through empty asm: otherwise hipcc shares flash_body's index arithmetic
                // with the code above and carries it, in scratch, through the half-tile loop)
                int tid_ = tid, h_ = h, qb_ = qblk * 2 + half, b_ = b;
                asm volatile("" : "+v"(tid_), "+s"(h_), "+s"(qb_), "+s"(b_));
                if (qb_ * 256 < Lq)
                    flash_body<T, D, 1>(q, img, ktmax, out, H, Lq, M, nT, batch_per_group, scale_log2, diag_bias_log2, q_ld,
                                     h_, qb_, b_, tid_);
            }
            return;
        }
    }

    floatx16 o[2][NDB];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[j][db][r] = 0.f;

    // Phase (u, F).  FIRST = tile 0: its scores were accumulated from zero and the anchor is subtracted afterwards, as
    // flash_body's search pass does on tile 0 (later tiles start their chains at -m_run).  FULL: (u + 3 < nT), the ring
    // handling is unconditional.
    auto phase = [&](int u, auto f_c, auto first_c, auto full_c) __attribute__((always_inline)) {
        constexpr int F = decltype(f_c)::value;
        constexpr bool FIRST = decltype(first_c)::value;
        constexpr bool FULL = decltype(full_c)::value;
        const int slot = u & 3;
        auto ring_sync = [&]() __attribute__((always_inline)) {
            if (F == 0) {  // pack u + 2 (step u + 1) has landed for everyone
                if (FULL) dma_wait_barrier<PackRing<D>::NPW_LO>(); else ring.wait_barrier(u + 2 < nT ? 1 : 0);
            } else {       // everyone is through phase (u, 0): pack u's slot takes pack u + 4
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if (FULL || u + 3 < nT) ring.stage(u + 4, (u + 3) & 3);
            }
        };
        if (grpB) ring_sync();
        __builtin_amdgcn_sched_barrier(0);

        // ---- V^T fragments of the phase's two k-steps, in flight under the softmax
        X8 vf[2][NDB];
        {
            const char* vb_ = smem + slot * Cfg::TILE + voff + F * (4 * Cfg::DPV * 16);
#pragma unroll
            for (int kc = 0; kc < 2; ++kc)
#pragma unroll
                for (int db = 0; db < NDB; ++db)
                    vf[kc][db] = *reinterpret_cast<const X8*>(vb_ + (kc * 2 * Cfg::DPV + db * 32) * 16);
        }
        __builtin_amdgcn_sched_barrier(0);

        X8 pf[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (FIRST) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[j][r] -= m_run[j];
            }
            if constexpr (!FOLD) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[j][r] *= cmul;
            }
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(s[j][r]);
                const float p1 = __builtin_amdgcn_exp2f(s[j][r + 1]);
                pf[j][r >> 3][r & 7] = (T)p0;
                pf[j][r >> 3][(r & 7) + 1] = (T)p1;
            }
            // (pins the exponentials in front of group A's barrier, as in flash_body)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) asm volatile("" : "+v"(pf[j][kc]));
        }
        __builtin_amdgcn_sched_barrier(0);

        if (!grpB) ring_sync();
        __builtin_amdgcn_sched_barrier(0);

        // ---- K fragments of the next 32 keys (second half of tile u: pack u; first half of tile u + 1: this pack)
        X8 kf[NKS];
        {
            const char* kb_ = smem + (F == 0 ? ((u + 3) & 3) * Cfg::TILE + 512 : slot * Cfg::TILE) + koff;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) kf[ks] = *reinterpret_cast<const X8*>(kb_ + ks * 2048);
        }
        __builtin_amdgcn_sched_barrier(0);

        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kc = 0; kc < 2; ++kc)
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    o[j][db] = Elem<T>::mfma32x32x16(vf[kc][db], pf[j][kc], o[j][db]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[j][r] = (FIRST && F == 0) ? 0.f : -m_run[j];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                s[j] = Elem<T>::mfma32x32x16(kf[ks], qf[j][ks], s[j]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };

    const std::integral_constant<int, 0> f0;
    const std::integral_constant<int, 1> f1;
    const std::integral_constant<bool, true> yes;
    const std::integral_constant<bool, false> no;
    phase(0, f0, yes, no);
    phase(0, f1, yes, no);
    int u = 1;
    for (; u + 3 < nT; ++u) {
        phase(u, f0, no, yes);
        phase(u, f1, no, yes);
    }
    for (; u < nT - 1; ++u) {
        phase(u, f0, no, no);
        phase(u, f1, no, no);
    }

    // ---- the last tile, whole: padded keys masked, the max looked at (flash_body's fix and search passes)
    // (what only the last tile and the epilogue need of the lane's indices is derived again from here on, not carried in
    // registers through the loop above, which has none to spare)
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int l31e = tid2 & 31, hie = (tid2 >> 5) & 1;
    {
        const int slot = u & 3;
        if (grpB) dma_wait_barrier<0>();
        __builtin_amdgcn_sched_barrier(0);
        floatx16 s1[2];  // the tile's second half (its K: pack u)
        qk_half(s1, (u + 3) & 3, 1, -m_run[0], -m_run[1]);
        __builtin_amdgcn_sched_barrier(0);
        X8 pf[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int kbase = u * 64 + 4 * hie;
            asm volatile("" : "+v"(kbase));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key0 = kbase + (r & 3) + 8 * (r >> 2);
                if (key0 >= M) s[j][r] = -1e30f;
                if (key0 + 32 >= M) s1[j][r] = -1e30f;
            }
            float mt = fmaxf(s[j][0], s1[j][0]);
#pragma unroll
            for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[j][r]), s1[j][r]);
            mt = max_both_halves(mt);
            const float resc_thr = FOLD ? RESCALE_THR : RESCALE_THR / cmul;
            if (__builtin_amdgcn_readfirstlane((int)__any(mt > resc_thr)) != 0) {
                const float delta = fmaxf(mt, 0.f);
                const float alpha = __builtin_amdgcn_exp2f(FOLD ? -delta : -delta * cmul);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[j][r] -= delta;
                    s1[j][r] -= delta;
                }
#pragma unroll
                for (int db = 0; db < NDB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[j][db][r] *= alpha;
            }
            if constexpr (!FOLD) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[j][r] *= cmul;
                    s1[j][r] *= cmul;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(s[j][r]);
                const float p1 = __builtin_amdgcn_exp2f(s[j][r + 1]);
                const float p2 = __builtin_amdgcn_exp2f(s1[j][r]);
                const float p3 = __builtin_amdgcn_exp2f(s1[j][r + 1]);
                pf[j][r >> 3][r & 7] = (T)p0;
                pf[j][r >> 3][(r & 7) + 1] = (T)p1;
                pf[j][2 + (r >> 3)][r & 7] = (T)p2;
                pf[j][2 + (r >> 3)][(r & 7) + 1] = (T)p3;
            }
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) asm volatile("" : "+v"(pf[j][kc]));
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!grpB) dma_wait_barrier<0>();
        __builtin_amdgcn_sched_barrier(0);
        const char* vb_ = smem + slot * Cfg::TILE + voff;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            X8 vf[NDB];
#pragma unroll
            for (int db = 0; db < NDB; ++db)
                vf[db] = *reinterpret_cast<const X8*>(vb_ + (kc * 2 * Cfg::DPV + db * 32) * 16);
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    o[j][db] = Elem<T>::mfma32x32x16(vf[db], pf[j][kc], o[j][db]);
        }
    }

    const float no_l[2] = {0.f, 0.f};  // (the row sum is O^T row D)
    flash_store<T, D, 2>(o, no_l, out, (int64_t)b * Lq, Lq, C, h, qblk * 512 + (tid2 >> 6) * 64 + l31e, l31e, hie);
}

#define FRESCO_FLASH_KERNEL(NAME, T)                                                                                  \
    template <int D, int QB>                                                                                          \
    __global__ __launch_bounds__(512, 2) void NAME(const T* __restrict__ q, const char* __restrict__ img,             \
                                                   const float* __restrict__ ktmax, T* __restrict__ out, int B,        \
                                                   int H, int Lq, int M, int nT, int batch_per_group,                  \
                                                   float scale_log2, float diag_bias_log2, int64_t q_ld) {             \
        const int nQblk = (Lq + 256 * QB - 1) / (256 * QB);                                                           \
        const unsigned blk = blockIdx.x;                                                                              \
        const int h = blk % H;                                                                                        \
        const int qblk = (blk / H) % nQblk;                                                                           \
        const int b = blk / (H * nQblk);                                                                              \
        if constexpr (FlashHalves<D, QB>::value)                                                                      \
            flash_body_halves<T, D>(q, img, ktmax, out, H, Lq, M, nT, batch_per_group, scale_log2, diag_bias_log2,     \
                                    q_ld, h, qblk, b);                                                                \
        else                                                                                                          \
            flash_body<T, D, QB>(q, img, ktmax, out, H, Lq, M, nT, batch_per_group, scale_log2, diag_bias_log2, q_ld,  \
                                 h, qblk, b, threadIdx.x);                                                            \
    }
FRESCO_FLASH_KERNEL(attn_flash_kernel, half_t)
FRESCO_FLASH_KERNEL(attn_flash_bf16_kernel, bf16_t)
#undef FRESCO_FLASH_KERNEL

template <typename T, int D, int QB>
static auto flash_kernel_of() {
    if constexpr (std::is_same<T, bf16_t>::value)
        return &attn_flash_bf16_kernel<D, QB>;
    else
        return &attn_flash_kernel<D, QB>;
}
template <typename T, int D>
static auto kv_pack_kernel_of() {
    if constexpr (std::is_same<T, bf16_t>::value)
        return &kv_pack_bf16_kernel<D>;
    else
        return &kv_pack_kernel<D>;
}

template <typename T, int D, int QB>
static int launch_flash(const T* q, const char* img, T* out, int B, int H, int Lq, int M, int nT,
                        int n_groups, float scale, float diag_bias, int64_t q_ld, const float* ktmax,
                        hipStream_t st) {
    using Cfg = AttnCfg<D>;
    constexpr int lds = Cfg::LDS_BYTES + (FlashHalves<D, QB>::value ? 64 : 0);  // + the eight waves' votes
    auto kern = flash_kernel_of<T, D, QB>();
    if (int rc = allow_dyn_lds(kern, lds)) return rc;
    const int nQblk = (Lq + 256 * QB - 1) / (256 * QB);
    const float log2e = 1.4426950408889634f;
    ProfScope ps(FRESCO_PROF_ATTN_FLASH, B * H, Lq, M, D, st);
    const int grid = H * nQblk * B;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, q, img,
                       ktmax, out, B, H, Lq, M, nT, B / n_groups, scale * log2e, diag_bias * log2e, q_ld);
    return check_launch();
}

// Two query blocks (64 rows) per wave while the accumulators leave room (two waves per SIMD = 256
// registers each): every K / V^T fragment read from LDS then feeds two (four) MFMAs.  Exception: a launch whose
// 512-row workgroups would leave CUs idle (a frame shard of a multi-GPU run: 2 batch rows x 8 heads x 8 query blocks
// = 128 workgroups for 256 CUs) takes 256-row workgroups instead -- twice as many, each half as long.  D = 80 (the
// half-tile body) follows the same rule, and keeps 256-row workgroups for launches of at most 256 queries.
template <typename T, int D>
static int launch_flash_auto(const T* q, const char* img, T* out, int B, int H, int Lq, int M, int nT,
                             int n_groups, float scale, float diag_bias, int64_t q_ld, const float* ktmax,
                             hipStream_t st) {
    using Cfg = AttnCfg<D>;
    if constexpr ((D <= 48 && Cfg::MCOL) || FlashHalves<D, 2>::value) {
        const int grid2 = H * ((Lq + 511) / 512) * B;
        const bool idle = grid2 < device_cus();
        if (FlashHalves<D, 2>::value ? (idle || Lq <= 256) : (idle && Lq > 256))
            return launch_flash<T, D, 1>(q, img, out, B, H, Lq, M, nT, n_groups, scale, diag_bias, q_ld, ktmax, st);
        return launch_flash<T, D, 2>(q, img, out, B, H, Lq, M, nT, n_groups, scale, diag_bias, q_ld, ktmax, st);
    } else {
        return launch_flash<T, D, 1>(q, img, out, B, H, Lq, M, nT, n_groups, scale, diag_bias, q_ld, ktmax, st);
    }
}

template <typename T, int D>
static int launch_attn(const T* q, const T* k, const T* v, const int32_t* kv_rows,
                       T* out, char* ws, int B, int H, int Lq, int n_groups, int M,
                       int64_t group_rows, float scale, float diag_bias, int64_t q_ld, int64_t kv_ld,
                       hipStream_t st) {
    using Cfg = AttnCfg<D>;
    const int nT = ntiles_of(M);
    char* img = ws;
    float* ktmax = reinterpret_cast<float*>(ws + align_up((size_t)n_groups * H * (nT + 1) * Cfg::TILE, 256));
    dim3 pg(nT, H, n_groups);
    {
        ProfScope ps(FRESCO_PROF_KV_PACK, n_groups, H, M, D, st);
        hipLaunchKernelGGL((kv_pack_kernel_of<T, D>()), pg, dim3(256), 0, st, k, v, kv_rows, img, ktmax, H, M, nT, group_rows,
                           kv_ld);
    }
    return launch_flash_auto<T, D>(q, img, out, B, H, Lq, M, nT, n_groups, scale, diag_bias, q_ld, ktmax, st);
}

static size_t attn_ws_bytes(int n_groups, int H, int M, int D) {
    const size_t nT = ntiles_of(M);
    const size_t dpk = (D + 15) / 16 * 16, dpv = (D + 31) / 32 * 32;
    return align_up((size_t)n_groups * H * (nT + 1) * ((dpk + dpv) * 128), 256) +
           align_up((size_t)n_groups * H * nT * sizeof(float), 256);
}

}  // namespace fresco

using namespace fresco;

extern "C" size_t fresco_attn_workspace_bytes(int n_groups, int H, int M, int D) {
    if (n_groups <= 0 || H <= 0 || M <= 0 || D <= 0) return 0;
    return attn_ws_bytes(n_groups, H, M, D);
}

extern "C" int fresco_attn_fwd(const void* q, const void* k, const void* v, const int32_t* kv_rows,
                               void* out, void* workspace, size_t workspace_bytes, int B, int H,
                               int Lq, int D, int n_groups, int M, int64_t group_rows, float scale,
                               float diag_bias, int64_t q_ld, int64_t kv_ld, int dtype, void* stream) {
    if (dtype != FRESCO_F16 && dtype != FRESCO_BF16) return FRESCO_EINVAL;
    if (!q || !k || !v || !out || !workspace) return FRESCO_EINVAL;
    if (q_ld < (int64_t)H * D || kv_ld < (int64_t)H * D || q_ld % 8 != 0 || kv_ld % 8 != 0) return FRESCO_EINVAL;
    if (B <= 0 || H <= 0 || Lq <= 0 || D <= 0 || n_groups <= 0 || M <= 0 || group_rows <= 0)
        return FRESCO_EINVAL;
    if (B % n_groups != 0 || !(scale > 0.f)) return FRESCO_EINVAL;
    if (workspace_bytes < attn_ws_bytes(n_groups, H, M, D)) return FRESCO_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    return with_elem(dtype, [&](auto e) {
        using T = decltype(e);
        const T* qh = static_cast<const T*>(q);
        const T* kh = static_cast<const T*>(k);
        const T* vh = static_cast<const T*>(v);
        T* oh = static_cast<T*>(out);
#define FRESCO_ATTN_CASE(DD)                                                                       \
    case DD:                                                                                       \
        return launch_attn<T, DD>(qh, kh, vh, kv_rows, oh, ws, B, H, Lq, n_groups, M, group_rows, scale, \
                                  diag_bias, q_ld, kv_ld, st);
        switch (D) {
            FRESCO_ATTN_CASE(8)
            FRESCO_ATTN_CASE(16)
            FRESCO_ATTN_CASE(32)
            FRESCO_ATTN_CASE(40)
            FRESCO_ATTN_CASE(64)
            FRESCO_ATTN_CASE(80)
            FRESCO_ATTN_CASE(96)
            FRESCO_ATTN_CASE(128)
            default:
                return FRESCO_EUNSUPPORTED;
        }
#undef FRESCO_ATTN_CASE
    });
}

namespace fresco {
template <typename T, int KIN, int D>
static int launch_kvproj_attn(const T* q, const T* x, int64_t x_ld, const int32_t* x_rows, const T* Wk, const T* Wv, T* out,
                              char* ws, int B, int H, int Lq, int n_groups, int M, float scale, int64_t q_ld,
                              hipStream_t st) {
    using Cfg = AttnCfg<D>;
    const int nT = ntiles_of(M);
    char* img = ws;
    float* ktmax = reinterpret_cast<float*>(ws + align_up((size_t)n_groups * H * (nT + 1) * Cfg::TILE, 256));
    {
        ProfScope ps(FRESCO_PROF_KV_PACK, n_groups, H, M, -D, st);  // (d < 0: the fused projection + pack launch)
        constexpr int lds = KvProjCfg<KIN, D>::LDS_BYTES;
        const auto kern = kvproj_pack_kernel_of<T, KIN, D>();
        if (int rc = allow_dyn_lds(kern, lds)) return rc;  // (every launch: the attribute is per device)
        constexpr int TL = KvProjCfg<KIN, D>::TILES;
        hipLaunchKernelGGL(kern, dim3((nT + TL - 1) / TL, 2 * (H * D / 160), n_groups), dim3(320), lds, st, x, x_ld, x_rows,
                           Wk, Wv, img, ktmax, H, M, nT);
    }
    return launch_flash_auto<T, D>(q, img, out, B, H, Lq, M, nT, n_groups, scale, 0.f, q_ld, ktmax, st);
}
}  // namespace fresco

extern "C" int fresco_attn_kvproj_supported(int H, int D, int K_in) {
    return (H > 0 && (int64_t)H * D == K_in && ((D == 40 && K_in == 320) || (D == 80 && K_in == 640))) ? 1 : 0;
}

extern "C" int fresco_attn_fwd_kvproj(const void* q, const void* x, int64_t x_ld, const int32_t* x_rows, const void* Wk,
                                      const void* Wv, void* out, void* workspace, size_t workspace_bytes, int B, int H,
                                      int Lq, int D, int n_groups, int M, int K_in, float scale, int64_t q_ld, int dtype,
                                      void* stream) {
    if (dtype != FRESCO_F16 && dtype != FRESCO_BF16) return FRESCO_EINVAL;
    if (!q || !x || !x_rows || !Wk || !Wv || !out || !workspace) return FRESCO_EINVAL;
    if (B <= 0 || H <= 0 || Lq <= 0 || D <= 0 || n_groups <= 0 || M <= 0 || K_in <= 0) return FRESCO_EINVAL;
    if (B % n_groups != 0 || !(scale > 0.f)) return FRESCO_EINVAL;
    if (q_ld < (int64_t)H * D || q_ld % 8 != 0 || x_ld < K_in || x_ld % 8 != 0) return FRESCO_EINVAL;
    if (!fresco_attn_kvproj_supported(H, D, K_in)) return FRESCO_EUNSUPPORTED;
    if (workspace_bytes < attn_ws_bytes(n_groups, H, M, D)) return FRESCO_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    return with_elem(dtype, [&](auto e) {
        using T = decltype(e);
        const T* qh = static_cast<const T*>(q);
        const T* xh = static_cast<const T*>(x);
        const T* wk = static_cast<const T*>(Wk);
        const T* wv = static_cast<const T*>(Wv);
        T* oh = static_cast<T*>(out);
        if (D == 40)
            return launch_kvproj_attn<T, 320, 40>(qh, xh, x_ld, x_rows, wk, wv, oh, ws, B, H, Lq, n_groups, M, scale, q_ld, st);
        return launch_kvproj_attn<T, 640, 80>(qh, xh, x_ld, x_rows, wk, wv, oh, ws, B, H, Lq, n_groups, M, scale, q_ld, st);
    });
}
