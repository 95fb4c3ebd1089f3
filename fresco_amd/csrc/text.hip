// What the CLIP text model of fp16 pipelines needs beside unet_layernorm and vae_conv: include/fresco_text.h, DESIGN.md
// section 24.
//
//   clip_embed_kernel    out[b, t, :] = tok[ids[b, t], :] + pos[t, :], one fp16 addition per element
//   clip_attn64_kernel   out = causal softmax(scale q k^T) v per (sequence, head), D = 64, L <= 128, fp16
//   clip_fc1_kernel      out = quick_gelu(x W^T + b) on conv_tile.h's tile with the rows flat: the pre-activation is never
//                        written
//
// clip_embed_kernel.  One thread per 16-byte piece of an output row, grid-stride over rows x C / 8 pieces.  The id is read as
// int64; one outside [0, vocab) reads NOTHING from the table and its row is written as NaN (0x7E00), so it shows downstream.
// The addition is the fp16 one (v_pk_add_f16): the exact sum rounded once, what torch computes for fp16 + fp16.
//
// clip_attn64_kernel.  grid (H, B), 256 threads = four waves; ONE WORKGROUP PER (sequence, head).  K and a transposed V of
// the whole sequence are staged ONCE by all 256 threads with plain loads and stores (every load before the first store: one
// memory latency); rows at or past L are written as zeros and never read from memory.  WAVE w OWNS QUERIES 32 w .. 32 w + 31
// and walks key blocks 0 .. w only: the blocks right of its diagonal are never multiplied.  A wave whose queries all lie at
// or past L leaves after the staging barrier.  The 32 x 32 x 16 fp16 MFMA both times, transposed as in unet_attn.hip (the
// query on the lane, keys / features in the registers):
//   S^T (32 keys x 32 queries) = K Q^T      4 k-steps per key block; A = 16 bytes of a K row from LDS, B = Q, 16 registers
//   O^T (64 features x 32 q.) += V^T P^T    2 blocks x 2 k-steps per key block, 32 accumulator registers; A = V^T from LDS
// THE WHOLE ROW OF SCORES IS IN REGISTERS (4 blocks x 16): one pass, no running maximum, no rescaling.  THE MASK IS A
// SELECTION on the fp32 scores: key > query gives -inf before the row maximum, so P is exactly 0 there and the result does
// not depend on what the future keys hold (they are finite: 0 x finite = 0 in the MFMA).  Key 0 <= every query, so the
// maximum is finite.  Scale and softmax in fp32 (log2 units), P rounded to fp16, the row sum is the sum of the ROUNDED P,
// fp32 accumulators, one rounding of the output; stored from the registers as 8-byte pieces (four consecutive features).
// Element j of lane half h of a P fragment of k-step s is key 16 s + 8 (j >> 2) + 4 h + (j & 3) of the block (the
// accumulator's row order), so the V^T fragment is two 8-byte reads of a [feature][key] image, as in unet_attn.hip.
// LDS (static, 32768 bytes):
//   K   [128 keys][128 bytes]      16384   16-byte piece c of row r sits at piece c ^ (r & 7)
//   V^T [64 features][256 bytes]   16384   the 8-byte granule g (keys 4 g .. 4 g + 3) of row d sits at granule g ^ (d & 31)
// ORDER (fixed, no atomics): key blocks in order, k-steps in order; the row sum adds a lane's 16 values per block in register
// order, blocks in order, then the partner lane's.
//
// clip_fc1_kernel.  unet_geglu_kernel's main loop (unet_tf.hip) with the weights in their own order: LDS (static, 32768
// bytes): two slots of 8 KiB for the tile's 128 rows of x, 32 columns deep, and conv_tile.h's two weight slots; the same ring
// (step s: wait, barrier, issue step s + 1, MFMAs).  N is a multiple of 64, so a wave's two channel blocks are live or dead
// together.  Epilogue: g = acc + bias in fp32, g / (1 + exp(-1.702 g)) in fp32, ONE rounding, four consecutive channels as
// 8 bytes.  No split-K, no atomics: same inputs, same bits.
//
// Registers (VGPRs / AGPRs): clip_embed_kernel 20 / 0, clip_attn64_kernel 123 / 0, clip_fc1_kernel 152 / 64; no spill, no
// scratch.  LDS (static bytes): clip_embed_kernel 0, clip_attn64_kernel 32768, clip_fc1_kernel 32768.
#include "common.h"
#include "lds_dma.h"
#include "conv_tile.h"
#include "../../include/fresco_text.h"

namespace fresco {

// ---------------------------------------------------------------------------------------------------------------------
// clip_embed
// ---------------------------------------------------------------------------------------------------------------------
struct CeArgs {
    const half_t* tok;
    const half_t* pos;
    const int64_t* ids;
    half_t* out;
    int64_t items;  // rows x pieces
    int L, npieces, vocab;
};

__global__ __launch_bounds__(256) void clip_embed_kernel(const CeArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < a.items; it += stride) {
        const int64_t row = it / a.npieces;
        const int p = (int)(it - row * a.npieces);
        const int t = (int)(row % a.L);
        const int64_t id = a.ids[row];
        half8_t o8;
        if (id >= 0 && id < a.vocab) {
            const half8_t e8 = *reinterpret_cast<const half8_t*>(a.tok + id * (int64_t)(a.npieces * 8) + p * 8);
            const half8_t p8 = *reinterpret_cast<const half8_t*>(a.pos + (int64_t)t * (a.npieces * 8) + p * 8);
            o8 = e8 + p8;
        } else {
            const half_t nan = __builtin_bit_cast(half_t, (unsigned short)0x7E00);
            o8 = half8_t{nan, nan, nan, nan, nan, nan, nan, nan};
        }
        *reinterpret_cast<half8_t*>(a.out + row * (int64_t)(a.npieces * 8) + p * 8) = o8;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// clip_attention
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CA_D = 64;
constexpr int CA_THREADS = 256;
constexpr int CA_LMAX = 128;                  // keys staged: the whole sequence
constexpr int CA_NKS = CA_D / 16;             // k-steps of K Q^T
constexpr int CA_NDB = CA_D / 32;             // 32-row blocks of O^T
constexpr int CA_NKB = CA_LMAX / 32;          // key blocks = query blocks = waves
constexpr int CA_CH = CA_D / 8;               // 16-byte pieces of a head's row
constexpr int CA_KPITCH = CA_D * 2;           // bytes
constexpr int CA_VPITCH = CA_LMAX * 2;
constexpr int CA_K_BYTES = CA_LMAX * CA_KPITCH;
constexpr int CA_V_BYTES = CA_D * CA_VPITCH;
constexpr int CA_LDS = CA_K_BYTES + CA_V_BYTES;
constexpr int CA_K_ITERS = CA_LMAX * CA_CH / CA_THREADS;       // 4 pieces of K per thread
constexpr int CA_V_ITERS = CA_LMAX / 2 * CA_CH / CA_THREADS;   // 2 (key pair, piece) items of V
static_assert(CA_LDS == 32768, "the header comment states it");
static_assert(CA_NKB == CA_THREADS / 64, "one wave per block of 32 queries");
static_assert(CA_LMAX / 2 == 64, "a wave's 64 lanes are a row's 64 key pairs");

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

struct CaArgs {
    const half_t* q;
    const half_t* k;
    const half_t* v;
    half_t* out;
    int64_t ld, out_ld;
    int L;
    float sl2;  // scale * log2(e)
};

__device__ __forceinline__ int ca_k_off(int key, int c) { return key * CA_KPITCH + ((c ^ (key & 7)) << 4); }
__device__ __forceinline__ int ca_v_off(int d, int g) { return d * CA_VPITCH + ((g ^ (d & 31)) << 3); }

__global__ __launch_bounds__(CA_THREADS, 2) void clip_attn64_kernel(const CaArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[CA_LDS];
    char* ksm = smem;
    char* vsm = smem + CA_K_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t col0 = (int64_t)blockIdx.x * CA_D;
    const int64_t row0 = (int64_t)blockIdx.y * a.L;
    const int L = a.L;
    const float ninf = -__builtin_inff();
    const half8_t z8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- stage K as it is and V transposed; rows at or past L are zeros and are not read.  K: thread t takes row t >> 1
    // and its pieces 2 i + (t & 1).  V: a thread takes 8 features (piece wave + 4 i) of keys 2 kp and 2 kp + 1 and writes 8
    // (key, key + 1) pairs; a wave's lanes are the 64 pairs of one piece
    {
        half8_t kx[CA_K_ITERS], x0[CA_V_ITERS], x1[CA_V_ITERS];
        const int key = 32 * wave + (lane >> 1), h2 = lane & 1, kp = lane;
        const half_t* kb = a.k + row0 * a.ld + col0;
        const half_t* vb = a.v + row0 * a.ld + col0;
#pragma unroll
        for (int i = 0; i < CA_K_ITERS; ++i)
            kx[i] = key < L ? *reinterpret_cast<const half8_t*>(kb + (int64_t)key * a.ld + (2 * i + h2) * 8) : z8;
#pragma unroll
        for (int i = 0; i < CA_V_ITERS; ++i) {
            const half_t* vp = vb + (int64_t)(2 * kp) * a.ld + (wave + 4 * i) * 8;
            x0[i] = 2 * kp < L ? *reinterpret_cast<const half8_t*>(vp) : z8;
            x1[i] = 2 * kp + 1 < L ? *reinterpret_cast<const half8_t*>(vp + a.ld) : z8;
        }
#pragma unroll
        for (int i = 0; i < CA_K_ITERS; ++i) *reinterpret_cast<half8_t*>(ksm + ca_k_off(key, 2 * i + h2)) = kx[i];
#pragma unroll
        for (int i = 0; i < CA_V_ITERS; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const half2_t pr = {x0[i][e], x1[i][e]};
                *reinterpret_cast<half2_t*>(vsm + ca_v_off((wave + 4 * i) * 8 + e, kp >> 1) + (kp & 1) * 4) = pr;
            }
    }
    // this lane's query: the 8 values of its half of every k-step (rows at or past L: zeros, nothing is read)
    const int qrow = 32 * wave + l31;
    half8_t qf[CA_NKS];
    {
        const half_t* qp = a.q + (row0 + (qrow < L ? qrow : 0)) * a.ld + col0 + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < CA_NKS; ++ks) qf[ks] = qrow < L ? *reinterpret_cast<const half8_t*>(qp + 16 * ks) : z8;
    }
    __syncthreads();
    if (32 * wave >= L) return;  // (wave-uniform; no barrier follows)

    // ---- S^T = K Q^T for key blocks 0 .. wave, the mask as a selection, the row maximum (log2 units)
    floatx16 s[CA_NKB];
    float mx = ninf;
#pragma unroll
    for (int kb = 0; kb < CA_NKB; ++kb) {
        if (kb > wave) continue;
        floatx16 acc = {};
        const int key = 32 * kb + l31;
#pragma unroll
        for (int ks = 0; ks < CA_NKS; ++ks)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t*>(ksm + ca_k_off(key, 2 * ks + hi)), qf[ks],
                                                         acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const float x = kr <= qrow ? acc[r] * a.sl2 : ninf;
            acc[r] = x;
            mx = fmaxf(mx, x);
        }
        s[kb] = acc;
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // finite: key 0 is at or before every query

    // ---- P = 2^(s - max) rounded to fp16, its sum, and O^T += V^T P^T
    floatx16 o[CA_NDB] = {};
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < CA_NKB; ++kb) {
        if (kb > wave) continue;
        half8_t p[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const half_t ph = (half_t)__builtin_amdgcn_exp2f(s[kb][r] - mx);
            p[r >> 3][r & 7] = ph;
            psum += (float)ph;
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < CA_NDB; ++db) {
                const int d = 32 * db + l31, g = 8 * kb + 4 * s2 + hi;   // granule g: keys 4 g .. 4 g + 3
                const half4_t lo = *reinterpret_cast<const half4_t*>(vsm + ca_v_off(d, g));
                const half4_t up = *reinterpret_cast<const half4_t*>(vsm + ca_v_off(d, g + 2));
                const half8_t vf = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, p[s2], o[db], 0, 0, 0);
            }
    }
    psum += __shfl_xor(psum, 32, 64);
    const float inv = 1.f / psum;  // psum >= 1: the maximum's own P is 1

    // ---- registers 4 g .. 4 g + 3 of block db are features 32 db + 8 g + 4 hi .. + 3 of query l31
    if (qrow >= L) return;
    half_t* op = a.out + (row0 + qrow) * a.out_ld + col0;
#pragma unroll
    for (int db = 0; db < CA_NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half4_t o4;
#pragma unroll
            for (int e = 0; e < 4; ++e) o4[e] = (half_t)(o[db][4 * g + e] * inv);
            *reinterpret_cast<half4_t*>(op + 32 * db + 8 * g + 4 * hi) = o4;
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// clip_fc1
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CF_A_BYTES = 8 * 1024;  // the tile's 128 rows of 64 bytes
constexpr int CF_LDS = 2 * CF_A_BYTES + 2 * CT_B_BYTES;
static_assert(CF_LDS == 32768, "the header comment states it");

struct CfArgs {
    const half_t* x;
    const half_t* w;
    const float* bias;
    half_t* out;
    int64_t ldo;
    int M, K, N, tiles;
};

__device__ __forceinline__ float cf_quick_gelu(float g) { return g / (1.f + expf(-1.702f * g)); }

__global__ __launch_bounds__(256) void clip_fc1_kernel(const CfArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[CF_LDS];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const CtTile t = ct_deal(1, a.tiles);
    const int co0 = t.col_tile * CT_BN;
    const int m0 = t.t_in * CT_BM;
    const uint32_t lds0 = lds_addr(smem);
    const char* zp = reinterpret_cast<const char*>(ct_zero_page);

    // ---- DMA sources: a lane owns LDS piece (slot & 3) of tile row slot >> 2 and fetches source piece (slot & 3) ^ swizzle(row)
    const char* a_src[2];
    const char* b_src[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int R, pc;
        ct_gemm_slot(wave, p, lane, R, pc);
        a_src[p] = (int64_t)m0 + R < a.M ? reinterpret_cast<const char*>(a.x + ((int64_t)m0 + R) * a.K + pc * 8) : nullptr;
        b_src[p] = ct_weight_src(a.w, co0, R, pc, a.N, a.K);
    }
    auto issue_a = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            lds_dma16(a_src[p] ? static_cast<const void*>(a_src[p] + (int64_t)chunk * (CT_BK * 2)) : static_cast<const void*>(zp),
                      lds0 + (uint32_t)((chunk & 1) * CF_A_BYTES + (wave * 2 + p) * 1024));
    };
    const uint32_t lds_b = lds0 + 2 * CF_A_BYTES;

    const int nbv = ct_live_blocks(a.N, co0, wn);  // 0 or 2: N is a multiple of 64
    floatx16 acc[2][2] = {};  // [channel block j][row block i]

    const int steps = a.K / CT_BK;
    const int wsw = (l31 >> 2) & 3;
    issue_a(0);
    ct_issue_weights(b_src, 0, 0, lds_b, wave);
    for (int s = 0; s < steps; ++s) {
        dma_wait_barrier<0>();
        if (s + 1 < steps) {
            ct_issue_weights(b_src, s + 1, (s + 1) * CT_BK, lds_b, wave);
            issue_a(s + 1);
        }
        const char* pa = smem + (s & 1) * CF_A_BYTES;
        const char* pb = smem + 2 * CF_A_BYTES + (s & 1) * CT_B_BYTES + (wn * 64 + l31) * 64;
        int aoff[2], asw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = ct_row(wm, i, l31);
            aoff[i] = r * 64;
            asw[i] = (r >> 2) & 3;
        }
#pragma unroll
        for (int ks = 0; ks < CT_BK / 16; ++ks) {
            const int piece = ks * 2 + hi;
            half8_t px[2], wt[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) px[i] = *reinterpret_cast<const half8_t*>(pa + aoff[i] + ((piece ^ asw[i]) * 16));
#pragma unroll
            for (int j = 0; j < 2; ++j) wt[j] = *reinterpret_cast<const half8_t*>(pb + j * 32 * 64 + ((piece ^ wsw) * 16));
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (j < nbv) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[j], px[i], acc[j][i], 0, 0, 0);
                }
        }
    }

    // ---- epilogue: registers 4 g .. 4 g + 3 of a block are four consecutive channels
    if (nbv == 0) return;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = ct_channel(co0, wn, j, hi, 4 * g);
            const floatx4 b4 = *reinterpret_cast<const floatx4*>(a.bias + ch);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int64_t row = (int64_t)m0 + ct_row(wm, i, l31);
                if (row >= a.M) continue;
                half4_t o4;
#pragma unroll
                for (int e = 0; e < 4; ++e) o4[e] = (half_t)cf_quick_gelu(acc[j][i][4 * g + e] + b4[e]);
                *reinterpret_cast<half4_t*>(a.out + row * a.ldo + ch) = o4;
            }
        }
}

}  // namespace fresco

using namespace fresco;

extern "C" int clip_embed(const void* tok, const void* pos, const int64_t* ids, void* out, int B, int L, int C, int vocab,
                          void* stream) {
    if (!tok || !pos || !ids || !out || B <= 0 || L <= 0 || C <= 0 || vocab <= 0) return FRESCO_EINVAL;
    if (C % 8 || (int64_t)B * L >= (int64_t)1 << 31) return FRESCO_EUNSUPPORTED;
    if (!aligned_to(tok, 16) || !aligned_to(pos, 16) || !aligned_to(out, 16) || !aligned_to(ids, 8)) return FRESCO_EINVAL;
    CeArgs a;
    a.tok = static_cast<const half_t*>(tok);
    a.pos = static_cast<const half_t*>(pos);
    a.ids = ids;
    a.out = static_cast<half_t*>(out);
    a.L = L;
    a.npieces = C / 8;
    a.vocab = vocab;
    a.items = (int64_t)B * L * a.npieces;
    const int64_t blocks = (a.items + 255) / 256;
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, as_stream(stream), a);
    return check_launch();
}

extern "C" int clip_attention(const void* q, const void* k, const void* v, int64_t qkv_ld, void* out, int64_t out_ld, int B,
                              int H, int L, int D, float scale, int dtype, void* stream) {
    if (!q || !k || !v || !out || B <= 0 || H <= 0 || L <= 0 || D <= 0 || !(scale > 0.f)) return FRESCO_EINVAL;
    if (dtype != FRESCO_F16 && dtype != FRESCO_BF16) return FRESCO_EINVAL;
    const int64_t C = (int64_t)H * D;
    if (qkv_ld < C || qkv_ld % 8 || out_ld < C || out_ld % 8) return FRESCO_EINVAL;
    if (!aligned_to(q, 16) || !aligned_to(k, 16) || !aligned_to(v, 16) || !aligned_to(out, 16)) return FRESCO_EINVAL;
    if (D != CA_D || L > CA_LMAX || dtype != FRESCO_F16 || B > 65535 || H > 65535) return FRESCO_EUNSUPPORTED;
    CaArgs a;
    a.q = static_cast<const half_t*>(q);
    a.k = static_cast<const half_t*>(k);
    a.v = static_cast<const half_t*>(v);
    a.out = static_cast<half_t*>(out);
    a.ld = qkv_ld;
    a.out_ld = out_ld;
    a.L = L;
    a.sl2 = scale * 1.4426950408889634f;
    hipLaunchKernelGGL(clip_attn64_kernel, dim3((unsigned)H, (unsigned)B), dim3(CA_THREADS), 0, as_stream(stream), a);
    return check_launch();
}

extern "C" int clip_fc1(const void* x, const void* w, const float* bias, void* out, int64_t M, int K, int N, int64_t ldo,
                        void* stream) {
    if (!x || !w || !bias || !out || M <= 0 || K <= 0 || N <= 0) return FRESCO_EINVAL;
    if (K % CT_BK || N % 64 || M >= (int64_t)1 << 31 || N >= 1 << 30) return FRESCO_EUNSUPPORTED;
    if (ldo < N || ldo % 4) return FRESCO_EINVAL;
    if (!aligned_to(x, 16) || !aligned_to(w, 16) || !aligned_to(bias, 16) || !aligned_to(out, 8)) return FRESCO_EINVAL;
    CfArgs a;
    a.x = static_cast<const half_t*>(x);
    a.w = static_cast<const half_t*>(w);
    a.bias = bias;
    a.out = static_cast<half_t*>(out);
    a.ldo = ldo;
    a.M = (int)M;
    a.K = K;
    a.N = N;
    a.tiles = (int)((M + CT_BM - 1) / CT_BM);
    const unsigned grid = ct_grid(1, a.tiles, N);
    if (!grid) return FRESCO_EUNSUPPORTED;
    hipLaunchKernelGGL(clip_fc1_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a);
    return check_launch();
}
