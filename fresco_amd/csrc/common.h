// Shared helpers for the gfx950 kernels of libfresco_hip.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fresco_hip.h"

typedef _Float16 half_t;
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16_t;
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace fresco {

void set_last_error(hipError_t e);

// Every launch wrapper ends with this: maps a failed launch to FRESCO_ELAUNCH.
static inline int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(e);
        return FRESCO_ELAUNCH;
    }
    return FRESCO_OK;
}

// Lets kernel `fn` take `bytes` of dynamic LDS on the current device: FRESCO_OK, or FRESCO_ELAUNCH with the HIP error
// recorded.  The attribute is per device: the largest value set is remembered per (kernel, device), and the call is made
// only when a launch needs more.  Thread-safe.
int allow_dyn_lds(const void* fn, int bytes);
template <typename... A>
static inline int allow_dyn_lds(void (*fn)(A...), int bytes) {
    return allow_dyn_lds(reinterpret_cast<const void*>(fn), bytes);
}

// CUs of the current device (cached per device; 256 if the query fails)
int device_cus();

// Opt-in kernel timing (fresco_prof_*): brackets selected launches with HIP events on the launch stream.
struct ProfScope {
    bool on;
    hipStream_t st;
    ProfScope(int tag, int a, int b, int c, int d, hipStream_t s);
    ~ProfScope();
};

// true while fresco_prof_enable() is in effect (kernels that would otherwise overlap on two streams then run on one)
bool prof_active();

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

static inline bool aligned_to(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// Grid of a streaming kernel of 256-thread blocks that walks `threads` items with a grid-stride loop: capped at 2048 blocks
// (256 CUs x 8 blocks)
constexpr int STREAM_MAX_BLOCKS = 2048;
static inline int stream_blocks(int64_t threads) {
    const int64_t b = (threads + 255) / 256;
    return (int)(b < STREAM_MAX_BLOCKS ? b : STREAM_MAX_BLOCKS);
}

template <typename T>
static inline T* carve(char*& p, size_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += align_up(count * sizeof(T), 256);
    return r;
}

// Element type of the 16-bit MFMA kernels (attn.hip, proj.hip, temporal.hip): fp16 or bf16.  The two share operand and
// accumulator lane maps on gfx950, so staging, swizzles and the packed images are common; what differs is the fragment
// types, the MFMA instructions, the conversions (round to nearest even in both) and the bit pattern of 1.0.
template <typename T>
struct Elem;
template <>
struct Elem<half_t> {
    typedef half_t scalar;
    typedef half4_t x4;
    typedef half8_t x8;
    static constexpr int CODE = FRESCO_F16;
    static constexpr unsigned ONE_BITS = 0x3C00u;
    static __device__ __forceinline__ floatx16 mfma32x32x16(x8 a, x8 b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ floatx4 mfma16x16x32(x8 a, x8 b, floatx4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ floatx4 mfma16x16x16(x4 a, x4 b, floatx4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ scalar from_float(float f) { return (scalar)f; }
};
template <>
struct Elem<bf16_t> {
    typedef bf16_t scalar;
    typedef bf16x4_t x4;
    typedef bf16x8_t x8;
    static constexpr int CODE = FRESCO_BF16;
    static constexpr unsigned ONE_BITS = 0x3F80u;
    static __device__ __forceinline__ floatx16 mfma32x32x16(x8 a, x8 b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ floatx4 mfma16x16x32(x8 a, x8 b, floatx4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ floatx4 mfma16x16x16(x4 a, x4 b, floatx4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ scalar from_float(float f) { return (scalar)f; }  // v_cvt_pk_bf16_f32
};

// Calls f with a value of the element type that `dtype` names, f(half_t{}) or f(bf16_t{}); any other code: FRESCO_EINVAL.
template <typename F>
static inline int with_elem(int dtype, F&& f) {
    if (dtype == FRESCO_F16) return f(half_t{});
    if (dtype == FRESCO_BF16) return f(bf16_t{});
    return FRESCO_EINVAL;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide sum for blockDim.x == 256 (4 waves); `red` is >= 4 floats of LDS. All threads get the result.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

}  // namespace fresco
