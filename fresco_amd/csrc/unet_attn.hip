// Flash attention at head dim 160 for the UNet's 1280-wide transformer blocks: include/fresco_unet_attn.h, DESIGN.md
// section 21.
//
//   unet_attn160_kernel   out = softmax(scale q k^T) v per (batch, head), D = 160, fp16, any Lq and Lk
//
// Built for FEW QUERY ROWS AND SHORT KEY SETS (64 .. 448 tokens, the 77-token text), not for attn.hip's long key streams: at
// (16 images, 8 heads, 64 queries) the launch has only 256 blocks of 32 queries, so a workgroup takes ONE block of 32 queries
// of one (batch, head) and its FOUR WAVES SPLIT THE KEYS: of every 128-key tile, wave w owns keys 32 w .. 32 w + 31, keeps
// its own running maximum, row sum and O^T, and the four partial results are merged once at the end, in wave order.
// grid (H, B, ceil(Lq / 32)), 256 threads.  No pre-pass, no workspace, one launch.
//
// Per wave, the 32 x 32 x 16 fp16 MFMA both times, transposed as in attn.hip (the query on the lane, keys / features in the
// registers), so the softmax of a query is 16 registers of one lane and its partner lane (l ^ 32), and the rounded P is the
// B operand of the second product as it stands:
//   S^T (32 keys x 32 queries)   = K Q^T      10 k-steps; A = 16 bytes of a K row from LDS, B = Q, 40 registers, loaded per tile
//   O^T (160 features x 32 q.)  += V^T P^T    5 blocks x 2 k-steps, 80 accumulator registers; A = V^T from LDS
// Element j of lane half h of a P fragment of k-step s is key 16 s + 8 (j >> 2) + 4 h + (j & 3) of the wave's 32 (the
// accumulator's row order), so the V^T fragment is keys 16 s + 4 h .. + 3 and 16 s + 8 + 4 h .. + 3: two 8-byte reads of a
// [feature][key] image.  AttnCfg<160> pads nothing (160 = 10 x 16 = 5 x 32): no spare ones row, no max column; the row sum
// is a VALU sum of the ROUNDED P, so the normalisation matches what P.V saw.
//
// LDS (dynamic, 81920 bytes = half a CU's 160 KiB: TWO workgroups per CU, one stages while the other multiplies; one tile at
// a time, staged by all 256 threads with plain loads and stores -- no LDS-DMA: the V image is a transpose and the ragged tail
// is written as zeros.  A tile's loads are all issued before its first store: one memory latency):
//   K   [128 keys][320 bytes]      40960   16-byte piece c of row r sits at piece c ^ ((r >> 2) & 3): the 16 rows a
//                                          ds_read_b128 lane group reads (4 of every 8) land on 16 different bank quads
//   V^T [160 features][256 bytes]  40960   the 8-byte granule g (keys 4 g .. 4 g + 3) of row d sits at granule g ^ (d & 31):
//                                          the 32 rows of a ds_read_b64 are 32 different granules; written as (key, key + 1)
//                                          pairs of 4 bytes, 64 consecutive pairs of one row per instruction (2-way, free)
// After the last tile the region is reused twice: for the waves' (m, l), fp32 [2][4][32], and then for the four waves' scaled
// O^T, fp32 [4][160][32] = 81920 bytes.
// Registers: 179 VGPRs (O^T in them: no separate accumulation registers), no spill, no scratch; __launch_bounds__(256, 2)
// holds the kernel to the 256 that two waves per SIMD leave each.
//
// RAGGED EDGES.  A tile stages round-up-to-32 of its keys; rows at or past Lk are never read from memory: K and V^T get
// zeros there, and their scores are set to -inf before the maximum, so P is exactly 0 and 0 x 0 reaches the MFMA.  A wave
// whose 32 keys all lie past the tile's end skips the tile; one that never had a key merges with weight exp2(-inf) = 0.  A
// staged block of 32 always holds at least its first key, so the running maximum is finite after a wave's first block and
// no inf - inf arises.  Query rows at or past Lq are zeros in Q and are not stored.
// ORDER (fixed, no atomics): keys in tile order per wave; the merge adds waves 0, 1, 2, 3 in that order; one rounding.
#include "common.h"
#include "../../include/fresco_unet_attn.h"

namespace fresco {

constexpr int UA_D = 160;
constexpr int UA_THREADS = 256;
constexpr int UA_QROWS = 32;              // queries per workgroup
constexpr int UA_KT = 128;                // keys per tile: 32 per wave
constexpr int UA_NKS = UA_D / 16;         // k-steps of K Q^T
constexpr int UA_NDB = UA_D / 32;         // 32-row blocks of O^T
constexpr int UA_CH = UA_D / 8;           // 16-byte pieces of a head's row
constexpr int UA_KPITCH = UA_D * 2;       // bytes
constexpr int UA_VPITCH = UA_KT * 2;
constexpr int UA_K_BYTES = UA_KT * UA_KPITCH;
constexpr int UA_V_BYTES = UA_D * UA_VPITCH;
constexpr int UA_O_WAVE = UA_D * UA_QROWS;  // floats
constexpr int UA_K_ITERS = UA_KT * UA_CH / UA_THREADS;        // 10 pieces of K per thread and tile
constexpr int UA_V_ITERS = UA_KT / 2 * UA_CH / UA_THREADS;    // 5 (key pair, piece) items of V
constexpr int UA_LDS = UA_K_BYTES + UA_V_BYTES;
static_assert(4 * UA_O_WAVE * 4 <= UA_LDS, "the merge reuses the tile's LDS");
static_assert(UA_LDS == 81920, "the header comment states it: two workgroups per CU");
static_assert(UA_KT * UA_CH % UA_THREADS == 0 && UA_KT / 2 == 64, "whole staging rounds; a wave's 64 lanes are a row's 64 key pairs");

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

struct UaArgs {
    const half_t* q;
    const half_t* k;
    const half_t* v;
    half_t* out;
    int64_t q_ld, kv_ld, out_ld;
    int Lq, Lk;
    float sl2;  // scale * log2(e)
};

// byte offsets of the swizzled images.  K: piece c = 2 j + h of row `key`; with j a constant this is one of two lane values
// (j even, j odd) plus 64 (j >> 1), an immediate.  V^T: granule g of row d
__device__ __forceinline__ int ua_k_off(int key, int j, int h) {
    return key * UA_KPITCH + 64 * (j >> 1) + (((2 * (j & 1) + h) ^ ((key >> 2) & 3)) << 4);
}
__device__ __forceinline__ int ua_v_off(int d, int g) { return d * UA_VPITCH + ((g ^ (d & 31)) << 3); }

__global__ __launch_bounds__(UA_THREADS, 2) void unet_attn160_kernel(const UaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ksm = smem;
    char* vsm = smem + UA_K_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (the head is the fastest grid index: workgroups 8 apart share an XCD, so with 8 heads every query block and every
    // image of a head reads its K and V through ONE L2 -- for speed only, nothing depends on the placement)
    const int q0 = blockIdx.z * UA_QROWS;
    const int64_t col0 = (int64_t)blockIdx.x * UA_D;
    const int64_t b = blockIdx.y;
    const float ninf = -__builtin_inff();
    const half8_t z8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // this lane's query: the 8 values of its half of every k-step (rows at or past Lq: zeros, nothing is read)
    const int qrow = q0 + (lane & 31);
    const half_t* qp = a.q + (b * a.Lq + (qrow < a.Lq ? qrow : 0)) * a.q_ld + col0 + 8 * (lane >> 5);

    floatx16 o[UA_NDB] = {};
    float m_run = ninf, l_run = 0.f;
    const half_t* kb = a.k + b * a.Lk * a.kv_ld + col0;
    const half_t* vb = a.v + b * a.Lk * a.kv_ld + col0;

    for (int t0 = 0; t0 < a.Lk; t0 += UA_KT) {
        const int nk = a.Lk - t0 < UA_KT ? a.Lk - t0 : UA_KT;  // keys of this tile
        const int nk32 = (nk + 31) & ~31;                       // staged: whole blocks of 32
        __syncthreads();                                        // the previous tile's fragment reads are over
        // (the lane index is made opaque per tile: the tile's LDS addresses are computed here, a few operations each, and not
        // hoisted out of the loop as a hundred loop-invariant registers)
        int ln = lane, wv = wave;
        asm volatile("" : "+v"(ln), "+s"(wv));
        const int l31 = ln & 31, hi = ln >> 5;
        // ---- every load of the tile before its first store: one memory latency.  K rows as they are: thread t takes row
        // t >> 1 and its pieces 2 i + (t & 1), i = 0 .. 9.  V transposed: a thread takes 8 features (piece c) of keys 2 kp and
        // 2 kp + 1 and writes 8 (key, key + 1) pairs; a wave's lanes are the 64 pairs of one piece
        {
            half8_t kx[UA_K_ITERS], x0[UA_V_ITERS], x1[UA_V_ITERS];
            const int kp = ln, key = 32 * wv + (ln >> 1), h2 = ln & 1;
            // (a wave-uniform tile base and 32-bit lane offsets: the host keeps 128 rows of kv_ld below 2^31 bytes)
            const half_t* kt = kb + (int64_t)t0 * a.kv_ld;
            const half_t* vt = vb + (int64_t)t0 * a.kv_ld;
            const int ld = (int)a.kv_ld;
#pragma unroll
            for (int i = 0; i < UA_K_ITERS; ++i)
                kx[i] = key < nk ? *reinterpret_cast<const half8_t*>(kt + (unsigned)(key * ld + h2 * 8 + i * 16)) : z8;
#pragma unroll
            for (int i = 0; i < UA_V_ITERS; ++i) {
                const unsigned off = (unsigned)(2 * kp * ld + (wv + 4 * i) * 8);
                x0[i] = 2 * kp < nk ? *reinterpret_cast<const half8_t*>(vt + off) : z8;
                x1[i] = 2 * kp + 1 < nk ? *reinterpret_cast<const half8_t*>(vt + (off + (unsigned)ld)) : z8;
            }
            __builtin_amdgcn_sched_barrier(0);   // (loads above, stores below: the compiler keeps the phases apart)
            if (32 * wv < nk32) {                // (a wave stages the K rows of its own 32 keys)
#pragma unroll
                for (int i = 0; i < UA_K_ITERS; ++i) *reinterpret_cast<half8_t*>(ksm + ua_k_off(key, i, h2)) = kx[i];
            }
            if (2 * kp < nk32) {
#pragma unroll
                for (int i = 0; i < UA_V_ITERS; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const half2_t pr = {x0[i][e], x1[i][e]};
                        *reinterpret_cast<half2_t*>(vsm + ua_v_off((wv + 4 * i) * 8 + e, kp >> 1) + (kp & 1) * 4) = pr;
                    }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- Q again for every tile (10 KiB from L2 per wave): its 40 registers are free while the tile is staged
        half8_t qf[UA_NKS];
#pragma unroll
        for (int ks = 0; ks < UA_NKS; ++ks) qf[ks] = qrow < a.Lq ? *reinterpret_cast<const half8_t*>(qp + 16 * ks) : z8;
        __syncthreads();
        if (32 * wave >= nk32) continue;  // (wave-uniform; the barriers above are outside)

        // ---- S^T = K Q^T for this wave's 32 keys
        floatx16 s = {};
        {
            const int key = 32 * wave + l31;
#pragma unroll
            for (int ks = 0; ks < UA_NKS; ++ks)
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t*>(ksm + ua_k_off(key, ks, hi)), qf[ks], s,
                                                           0, 0, 0);
        }
        // ---- scale, mask the keys past Lk, running maximum (log2 units)
        const int key0 = t0 + 32 * wave + 4 * hi;
        float mx = ninf;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + (r & 3) + 8 * (r >> 2);
            const float x = key < a.Lk ? s[r] * a.sl2 : ninf;
            s[r] = x;
            mx = fmaxf(mx, x);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                      // finite: the block's first key is a real one
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // 0 on the wave's first block (m_run = -inf)
        m_run = m_new;
        half8_t p[2];
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const half_t ph = (half_t)__builtin_amdgcn_exp2f(s[r] - m_new);
            p[r >> 3][r & 7] = ph;
            psum += (float)ph;
        }
        l_run = l_run * alpha + psum;  // (this lane's 16 keys; the two halves are added at the merge)
#pragma unroll
        for (int db = 0; db < UA_NDB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
        // ---- O^T += V^T P^T
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < UA_NDB; ++db) {
                const int d = 32 * db + l31, g = 8 * wave + 4 * s2 + hi;   // granule g: keys 4 g .. 4 g + 3 of the tile
                const half4_t lo = *reinterpret_cast<const half4_t*>(vsm + ua_v_off(d, g));
                const half4_t up = *reinterpret_cast<const half4_t*>(vsm + ua_v_off(d, g + 2));
                const half8_t vf = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, p[s2], o[db], 0, 0, 0);
            }
    }

    // ---- merge the four waves: m* = max m_w, L = sum_w l_w 2^(m_w - m*), out = sum_w O_w 2^(m_w - m*) / L, waves in order
    float* ml = reinterpret_cast<float*>(smem);
    float* osm = reinterpret_cast<float*>(smem);
    const int l31 = lane & 31, hi = lane >> 5;
    l_run += __shfl_xor(l_run, 32, 64);
    __syncthreads();  // every wave is past its last fragment read: the tile's LDS may be overwritten
    if (hi == 0) {
        ml[wave * UA_QROWS + l31] = m_run;
        ml[(4 + wave) * UA_QROWS + l31] = l_run;
    }
    __syncthreads();
    float mstar = ml[l31];
#pragma unroll
    for (int w = 1; w < 4; ++w) mstar = fmaxf(mstar, ml[w * UA_QROWS + l31]);  // finite: wave 0 holds key 0
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) L += ml[(4 + w) * UA_QROWS + l31] * __builtin_amdgcn_exp2f(ml[w * UA_QROWS + l31] - mstar);
    const float f = __builtin_amdgcn_exp2f(m_run - mstar) / L;  // L >= 1: the maximum's own P is 1
    __syncthreads();  // (m, l) are read: their bytes become O^T
#pragma unroll
    for (int db = 0; db < UA_NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            osm[wave * UA_O_WAVE + (32 * db + (r & 3) + 8 * (r >> 2) + 4 * hi) * UA_QROWS + l31] = o[db][r] * f;
    __syncthreads();
    // thread (query tid & 31, pieces tid >> 5, + 8, + 16): a wave's reads of one feature are 32 consecutive floats
    const int qr = tid & 31;
    if (q0 + qr < a.Lq) {
        half_t* op = a.out + (b * a.Lq + q0 + qr) * a.out_ld + col0;
        for (int c = tid >> 5; c < UA_CH; c += UA_THREADS / 32) {
            half8_t o8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* pp = osm + (c * 8 + e) * UA_QROWS + qr;
                o8[e] = (half_t)(((pp[0] + pp[UA_O_WAVE]) + pp[2 * UA_O_WAVE]) + pp[3 * UA_O_WAVE]);
            }
            *reinterpret_cast<half8_t*>(op + c * 8) = o8;
        }
    }
}

}  // namespace fresco

using namespace fresco;

extern "C" int unet_attention(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out,
                              int64_t out_ld, int B, int H, int Lq, int Lk, int D, float scale, int dtype, void* stream) {
    if (!q || !k || !v || !out || B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || D <= 0 || !(scale > 0.f)) return FRESCO_EINVAL;
    if (dtype != FRESCO_F16 && dtype != FRESCO_BF16) return FRESCO_EINVAL;
    const int64_t C = (int64_t)H * D;
    if (q_ld < C || q_ld % 8 || kv_ld < C || kv_ld % 8 || out_ld < C || out_ld % 8) return FRESCO_EINVAL;
    if (!aligned_to(q, 16) || !aligned_to(k, 16) || !aligned_to(v, 16) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    const int64_t nq = ((int64_t)Lq + UA_QROWS - 1) / UA_QROWS;
    if (D != UA_D || dtype != FRESCO_F16 || B > 65535 || nq > 65535 || kv_ld >= 1 << 22) return FRESCO_EUNSUPPORTED;
    UaArgs a;
    a.q = static_cast<const half_t*>(q);
    a.k = static_cast<const half_t*>(k);
    a.v = static_cast<const half_t*>(v);
    a.out = static_cast<half_t*>(out);
    a.q_ld = q_ld;
    a.kv_ld = kv_ld;
    a.out_ld = out_ld;
    a.Lq = Lq;
    a.Lk = Lk;
    a.sl2 = scale * 1.4426950408889634f;
    if (int rc = allow_dyn_lds(unet_attn160_kernel, UA_LDS)) return rc;
    const dim3 grid((unsigned)H, (unsigned)B, (unsigned)nq);
    hipLaunchKernelGGL(unet_attn160_kernel, grid, dim3(UA_THREADS), UA_LDS, as_stream(stream), a);
    return check_launch();
}
