// The (hi, lo) fp16 operand planes of the split-fp16 dense layers (flownet.hip, hed.hip): how a producer writes one value.
#pragma once
#include "common.h"

namespace fresco {

// x * scale = h + l.  The matrix pipe FLUSHES fp16 subnormals (attn32.hip), so a lo piece below 6.1e-5 would be lost and the
// operand would be no better than fp16: every plane is written pre-scaled by a power of two the caller passes (`scale`; the
// GEMM is told the same value) -- by default activations by 2^6 (lo pieces
// stay normal down to |x| = 2e-3, values up to 1000 fit), weights by 2^10 (|w| from 1.2e-4 to 60) -- and the GEMM scales its
// fp32 accumulators back exactly.  Beyond the range the scaled value saturates (finite, wrong) instead of becoming inf / NaN
// -- and the producer says so: fn_split returns true for a value it had to clamp (or a NaN), every producer kernel ORs
// that into the caller's `range_flag` word (fresco_fn_prep / _layernorm / _gemm, fresco_hed_input / _side_pool), and the
// host side of the network re-runs the forward with library ops when the word is set (fresco_amd/gmflow.py, hed.py).
__device__ __forceinline__ bool fn_split(float x, float scale, half_t& h, half_t& l) {
    const float xs = x * scale;
    x = fminf(fmaxf(xs, -65000.f), 65000.f);
    h = (half_t)x;
    l = (half_t)(x - (float)h);
    return !(fabsf(xs) <= 65000.f);
}
// Four consecutive channels (a float[4] or a floatx4) -> the two half4_t stores at o_hi / o_lo + offset (8-byte aligned);
// true when one of them saturated.  OPTIONAL: the planes may be absent (o_hi == nullptr): the split is formed all the same and
// nothing is stored -- such a caller hands fn_flag_range its flag word only where it has planes (midas_layernorm_kernel).
template <bool OPTIONAL = false, typename V>
__device__ __forceinline__ bool fn_split_store4(const V& v, float scale, half_t* o_hi, half_t* o_lo, int64_t offset) {
    half4_t h4, l4;
    bool sat = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        half_t hh, ll;
        sat |= fn_split(v[e], scale, hh, ll);
        h4[e] = hh;
        l4[e] = ll;
    }
    if (!OPTIONAL || o_hi) {
        *reinterpret_cast<half4_t*>(o_hi + offset) = h4;
        *reinterpret_cast<half4_t*>(o_lo + offset) = l4;
    }
    return sat;
}
__device__ __forceinline__ void fn_flag_range(int32_t* range_flag, bool sat) {
    if (range_flag && sat) atomicOr(range_flag, 1);  // (rare path)
}

}  // namespace fresco
