// LDS-DMA helper shared by the 1x1 convolution kernels (conv1x1.hip, conv1x1_wide.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rla {

// 16 bytes per lane, global -> LDS, lane-linear from the wave-uniform LDS byte
// address `lds`; M0 saved and restored in the same statement (LDS-DMA recipe)
__device__ __forceinline__ void c1_dma16(const void* gsrc, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds)
               : "memory");
}

}  // namespace rla
