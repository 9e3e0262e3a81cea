// mx_format.hpp -- the element rounding of the e4m3 / e2m1 quantisers: one device function for the MX row quantiser (mx.hip) and the
// per-token FP8 quantiser (sq.hip, inc_fp8_quant_rows), so both put a value on the same code, bit for bit.
// The rounding is done in fp32 arithmetic, not with v_cvt_scalef32_pk_*: with e = max(expfield(|v|), expfield(min normal)) the
// grid step at |v| is 2^(e - 127 - MB) (MB mantissa bits), t = rint(|v| / step) is an integer in [0, 2^(MB+1)] and
// ((e - expfield(min normal)) << MB) + t is the code -- the carry of t = 2^(MB+1) lands in the exponent field by itself and the
// subnormal codes are the case e == expfield(min normal).
#pragma once
#include "common.hpp"

template <int FMT> struct MxFmt;
template <> struct MxFmt<INC_MX_FP8_E4M3> { static constexpr int EMAX = 8, MB = 3, EMINF = 127 - 6; static constexpr float SAT = 448.f; };
template <> struct MxFmt<INC_MX_FP4_E2M1> { static constexpr int EMAX = 2, MB = 1, EMINF = 127; static constexpr float SAT = 6.f; };

// the code of the already scaled value v: RNE onto the element grid, saturating at +-SAT (a NaN saturates too: no NaN code is
// produced), with `sign` (0 / 1) in the sign bit
template <int FMT>
__device__ __forceinline__ uint32_t mx_encode(float v, uint32_t sign) {
  using F = MxFmt<FMT>;
  const float a = fminf(fabsf(v), F::SAT);
  int e = (int)(__float_as_uint(a) >> 23);
  e = e < F::EMINF ? F::EMINF : e;
  const float inv_step = __uint_as_float((uint32_t)(254 + F::MB - e) << 23);
  const uint32_t t = (uint32_t)(int)rintf(a * inv_step);
  const uint32_t mag = ((uint32_t)(e - F::EMINF) << F::MB) + t;
  return mag | (sign << (FMT == INC_MX_FP8_E4M3 ? 7 : 3));
}
