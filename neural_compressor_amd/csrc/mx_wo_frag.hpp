// mx_wo_frag.hpp -- the register dequantisation of the weight-only MX cell: packed MX codes and one E8M0 scale byte to the bf16 A
// fragment of v_mfma_f32_16x16x32_bf16 / _32x32x16_bf16 by the scaled conversions of gfx950 (tools/mx_cvt_lab.hip pins what they do;
// DESIGN section 8b).  Readers: gemm_mx_wo.hip (the decode GEMV and the tile GEMM) and gemm_mx_wo_moe.hip (the routed experts GEMM).
#pragma once
#include "strip_frame.hpp"

typedef __attribute__((ext_vector_type(2))) __bf16 wo_bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 wo_bf16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t wo_u32x4;

__device__ __forceinline__ uint32_t wo_bits(wo_bf16x2 v) {
  uint32_t r;
  __builtin_memcpy(&r, &v, 4);
  return r;
}
__device__ __forceinline__ wo_bf16x8 wo_frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const wo_u32x4 u = {a, b, c, d};
  wo_bf16x8 f;
  __builtin_memcpy(&f, &u, 16);
  return f;
}
// 8 consecutive k of one row as the bf16 MFMAs want them: fp4 from one dword (element 2 i in the low nibble of byte i, selector b
// converts byte b), fp8 from two (selector false / true converts bytes 0, 1 / 2, 3)
__device__ __forceinline__ wo_bf16x8 wo_cvt_fp4(uint32_t w, float scale) {
  return wo_frag(wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0)), wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1)),
                 wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2)), wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3)));
}
__device__ __forceinline__ wo_bf16x8 wo_cvt_fp8(uint32_t w0, uint32_t w1, float scale) {
  return wo_frag(wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, false)), wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, true)),
                 wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, false)), wo_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, true)));
}
// MFMA step s (8 k) of the 32 k a lane holds in `w` (fp4: dwords 0 .. 3, fp8: 0 .. 7)
template <int WF>
__device__ __forceinline__ wo_bf16x8 wo_step(const i32x8& w, int s, float scale) {
  if constexpr (WF == INC_MX_FP4_E2M1) return wo_cvt_fp4((uint32_t)w[s], scale);
  else return wo_cvt_fp8((uint32_t)w[2 * s], (uint32_t)w[2 * s + 1], scale);
}
__device__ __forceinline__ float wo_scale(int byte) { return __uint_as_float((uint32_t)byte << 23); }
