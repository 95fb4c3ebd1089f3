// LDS-DMA (global_load_lds_dwordx4): the one global -> LDS copy primitive of the gfx950 kernels, and its waits.
//
// Protocol:
//   * The copy is inline asm on purpose.  hipcc does not see these LDS writes; if it did, it would drain vmcnt to zero in
//     front of every fragment read.  It therefore does not wait for them either: `__syncthreads()` alone is NOT enough.
//   * A piece is visible to the workgroup after the ISSUING wave's own counted wait (vmcnt(N): at most the N newest of its
//     vector-memory operations still in flight; its global stores count too) followed by a barrier: dma_wait_barrier<N>().
//     A wave that reads only what it copied itself needs the wait alone: dma_wait<N>().
//   * One instruction copies 64 lanes x 16 bytes; lane l's bytes land at M0 + 16 l.  M0 is compiler-reserved and not
//     preserved between statements, so it is written in the statement that uses it.  (It cannot be listed as a clobber:
//     hipcc rejects it as a reserved register; it does not keep values in m0 across statements on gfx9+.)
//   * The s_nop 0 between the M0 write and the copy is the wait state gfx950 requires there.  hipcc inserts it when it
//     emits the pair itself (__builtin_amdgcn_global_load_lds); nothing inside an asm string is padded for us.
// Each kernel documents its own ring (slots, look-ahead, which wave copies which piece) where it uses these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fresco {

// the wave-uniform 32-bit LDS address of a __shared__ pointer
__device__ __forceinline__ uint32_t lds_addr(const void* shared_ptr) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) char*)shared_ptr);
}

// one piece, scalar base + per-lane byte offset: lane l's 16 bytes come from sbase + lane_off and land at lds_dst + 16 l
__device__ __forceinline__ void lds_dma16(uint32_t lane_off, const void* sbase, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(sbase), "s"(lds_dst)
                 : "memory");
}
// one piece, per-lane source address
__device__ __forceinline__ void lds_dma16(const void* lane_addr, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(lane_addr), "s"(lds_dst) : "memory");
}

template <int N>
__device__ __forceinline__ void dma_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// LGKM = false leaves the wave's own LDS reads out of the wait (flownet.hip)
template <int N, bool LGKM = true>
__device__ __forceinline__ void dma_wait_barrier() {
    if (LGKM)
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
    else
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// Rings whose waves copy NPW_HI (`many`) or NPW_LO pieces per slot: wait until at most `keep` (0, 1 or 2) of this wave's
// newest slots are still in flight, then the barrier.
template <int NPW_LO, int NPW_HI>
__device__ __forceinline__ void dma_wait_barrier_keep(int keep, int many) {
    if (keep == 0) {
        dma_wait_barrier<0>();
    } else if (many) {
        if (keep == 1) dma_wait_barrier<NPW_HI>(); else dma_wait_barrier<2 * NPW_HI>();
    } else {
        if (keep == 1) dma_wait_barrier<NPW_LO>(); else dma_wait_barrier<2 * NPW_LO>();
    }
}

}  // namespace fresco
