// mx_strip.hpp -- the operand fragments of v_mfma_scale_f32_16x16x128_f8f6f4 as the strip kernels of the MX cell load them: the decode
// GEMV (gemm_mx_gemv.hip), the routed experts GEMM (gemm_mx_moe.hip) and the FP8 per-token decode GEMV (gemm_fp8.hip).  Operand map (tools/mx_lab.hip): lane l
// holds row l & 15, lane group g = l >> 4; fp8: registers 0 .. 3 are the 16 bytes at 16 g of the K-tile and 4 .. 7 the 16 bytes at
// 64 + 16 g; fp4: registers 0 .. 3 are the 16 bytes of block g; either format: the scale byte of block g.
#pragma once
#include "common.hpp"

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int XK = INC_MX_KTILE;

__host__ __device__ constexpr int mx_tile_bytes(int fmt) { return fmt == INC_MX_FP8_E4M3 ? XK : XK / 2; }  // of one row and K-tile

// what a lane supplies of its row for the K-tile at `p` (= row + tile + 16 g), as the instruction wants it
template <int F, bool NT>
__device__ __forceinline__ i32x8 mx_frag(const uint8_t* p) {
  const i32x4* q = reinterpret_cast<const i32x4*>(p);
  const i32x4 lo = NT ? __builtin_nontemporal_load(q) : q[0];
  i32x4 hi = {0, 0, 0, 0};
  if constexpr (F == INC_MX_FP8_E4M3) hi = NT ? __builtin_nontemporal_load(q + 4) : q[4];
  i32x8 f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
  f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}
