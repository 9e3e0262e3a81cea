// mx.hip -- K15: OCP microscaling (MX) row quantiser, MXFP8 (e4m3) and MXFP4 (e2m1).  HBM-bound streaming kernel.
//
// The specification is the comment of inc_mx_quant in include/inc_mi355x.h; the reference emulates the formats
// with fake quantisation in float (torch/algorithms/mx_quant/utils.py), here the codes are the operands of
// v_mfma_scale_f32_32x32x64_f8f6f4 (gemm_mx.hip).  A block is 32 consecutive values along K:
//   byte  = clamp(expfield(max|x|) - emax, 0, 254)            (E8M0 scale 2^(byte - 127); emax 8 for e4m3, 2 for e2m1)
//   v     = x * 2^(127 - byte)                                (exact: a power of two; where it underflows fp32 the code is 0 anyway)
//   code  = RNE(v) onto the element grid, saturating, with the sign bit of x
// One lane owns one block, so max|x| needs no exchange between lanes and every code has one right answer, bit for bit: the row is
// read once (16-byte loads where K and the pointer allow it), the 32 codes leave as two (fp8) or one (fp4) 16-byte store.
// The element rounding is mx_encode of mx_format.hpp (shared with the per-token FP8 quantiser).
#include "mx_format.hpp"

namespace {

template <int FMT>
__device__ __forceinline__ uint32_t mx_code(float x, float mult) {
  return mx_encode<FMT>(x * mult, __float_as_uint(x) >> 31);
}

// the 32 values of block k0 .. k0 + 31 of the row that starts at element `row`; 0 from K on
template <int DT>
__device__ __forceinline__ void mx_load32(const void* __restrict__ x, int64_t row, int64_t k0, int64_t K, bool vec, float (&v)[32]) {
  if constexpr (DT == INC_F32) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int64_t kb = k0 + 4 * g;
      if (vec && kb < K) {  // K % 4 == 0: the group is whole
        const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + row + kb);
        v[4 * g] = a.x; v[4 * g + 1] = a.y; v[4 * g + 2] = a.z; v[4 * g + 3] = a.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * g + j] = (kb + j < K) ? static_cast<const float*>(x)[row + kb + j] : 0.f;
      }
    }
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t kb = k0 + 8 * g;
      if (vec && kb < K) {  // K % 8 == 0: the group is whole
        const uint4 u = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(x) + row + kb);
        const uint32_t r[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (DT == INC_BF16) {
            v[8 * g + 2 * j] = __uint_as_float(r[j] << 16);
            v[8 * g + 2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u);
          } else {
            v[8 * g + 2 * j] = f16_bits_to_f32((uint16_t)(r[j] & 0xffffu));
            v[8 * g + 2 * j + 1] = f16_bits_to_f32((uint16_t)(r[j] >> 16));
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[8 * g + j] = (kb + j < K) ? load_as_f32<DT>(x, row + kb + j) : 0.f;
      }
    }
  }
}

template <int DT, int FMT>
__global__ __launch_bounds__(256) void mx_quant_kernel(const void* __restrict__ x, int64_t M, int64_t K, int64_t Kp,
                                                       uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
  const int64_t nb = Kp / 32;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * nb) return;
  const int64_t m = i / nb, b = i - m * nb;
  constexpr int G = DT == INC_F32 ? 4 : 8;
  const bool vec = (K % G) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  float v[32];
  mx_load32<DT>(x, m * K, b * 32, K, vec, v);
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(v[j]));
  int byte = (int)(__float_as_uint(amax) >> 23) - MxFmt<FMT>::EMAX;  // at most 254 - 2
  byte = byte < 0 ? 0 : byte;
  const float mult = __uint_as_float((uint32_t)(254 - byte) << 23);  // 2^(127 - byte), a normal number for every byte <= 252
  scales[i] = (uint8_t)byte;
  if constexpr (FMT == INC_MX_FP8_E4M3) {
    uint32_t w[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      w[d] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[d] |= mx_code<FMT>(v[4 * d + j], mult) << (8 * j);
    }
    uint4* dst = reinterpret_cast<uint4*>(codes + m * Kp + b * 32);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  } else {
    uint32_t w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      w[d] = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) w[d] |= mx_code<FMT>(v[8 * d + j], mult) << (4 * j);  // element 2i: low nibble of byte i
    }
    *reinterpret_cast<uint4*>(codes + m * (Kp / 2) + b * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

extern "C" int inc_mx_quant(const void* x, int xdtype, int64_t M, int64_t K, int64_t Kp, int fmt, uint8_t* codes, uint8_t* scales,
                            inc_stream_t stream) {
  INC_CHECK_ARG(x && codes && scales && M > 0 && K > 0 && Kp >= K);
  if (fmt != INC_MX_FP8_E4M3 && fmt != INC_MX_FP4_E2M1) return INC_ERR_UNSUPPORTED;
  if (xdtype != INC_F32 && xdtype != INC_F16 && xdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  if ((Kp % INC_MX_KTILE) != 0) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(codes) & 15) == 0);
  INC_CHECK_ARG(M * (Kp / 32) < ((int64_t)1 << 31) * 256);
  const unsigned grid = (unsigned)ceil_div64(M * (Kp / 32), 256);
  INC_DISPATCH_DTYPE(xdtype, DT, {
    if (fmt == INC_MX_FP8_E4M3) mx_quant_kernel<DT, INC_MX_FP8_E4M3><<<grid, 256, 0, inc_s(stream)>>>(x, M, K, Kp, codes, scales);
    else mx_quant_kernel<DT, INC_MX_FP4_E2M1><<<grid, 256, 0, inc_s(stream)>>>(x, M, K, Kp, codes, scales);
  })
  INC_LAUNCH_RETURN();
}
