// mx_stage.hpp -- the row stage of tile256_frame.hpp as the f8f6f4 MFMA GEMMs use it (gemm_mx.hip, gemm_fp8.hip): a K-tile of 128
// elements issued as single 1 KiB LDS-DMA pieces, and the operand of v_mfma_[scale_]f32_32x32x64_f8f6f4 read back from it.  The
// operand maps are pinned in tools/mx_lab.hip (profiles/mx/mx_lab.log).
#pragma once
#include "tile256_frame.hpp"

typedef __attribute__((ext_vector_type(8))) int i32x8;

// RB = bytes of one row of one K-tile: 128 (fp8) or 64 (fp4)
template <int RB>
struct MxStage : RowStage<RB> {
  using RowStage<RB>::NI;
  using RowStage<RB>::chunk_off;
  __device__ static __forceinline__ void issue(const uint8_t* src, uint32_t lds_tile, int wave, const uint32_t (&off)[NI]) {
#pragma unroll
    for (int i = 0; i < NI; ++i) lds_dma_1k(src, __builtin_amdgcn_readfirstlane(lds_tile + (wave * NI + i) * 1024), off[i]);
  }
  // what lane half h supplies of `row` for the 64-wide step kk of the tile, as the instruction wants it; `sw` = swz(row)
  __device__ static __forceinline__ i32x8 frag(const char* tile, int row, int kk, int h, int sw) {
    i32x8 f;
    if constexpr (RB == 128) {
      const int slot = chunk_off(4 * kk + h, sw);  // 16-byte chunks h and 2 + h of the step's four
      const uint4 lo = *reinterpret_cast<const uint4*>(tile + row * 128 + slot);
      const uint4 hi = *reinterpret_cast<const uint4*>(tile + row * 128 + (slot ^ 32));
      f[0] = (int)lo.x; f[1] = (int)lo.y; f[2] = (int)lo.z; f[3] = (int)lo.w;
      f[4] = (int)hi.x; f[5] = (int)hi.y; f[6] = (int)hi.z; f[7] = (int)hi.w;
    } else {
      const uint4 lo = *reinterpret_cast<const uint4*>(tile + row * 64 + chunk_off(2 * kk + h, sw));  // block 2 kk + h
      f[0] = (int)lo.x; f[1] = (int)lo.y; f[2] = (int)lo.z; f[3] = (int)lo.w;
      f[4] = 0; f[5] = 0; f[6] = 0; f[7] = 0;  // fp4 occupies the first four registers; the instruction reads no more
    }
    return f;
  }
};
