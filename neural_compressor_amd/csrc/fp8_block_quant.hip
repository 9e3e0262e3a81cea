// fp8_block_quant.hip -- K18q: the quantisers of the block-scaled FP8 cell: one fp32 scale per 1 x 128 group of x
// (inc_fp8_quant_groups, at run time) and one per 128 x 128 block of W (inc_fp8_quant_blocks, at convert time).
//
// The scale rule and the element rounding are those of inc_fp8_quant_rows (sq.hip): s = max(max |t| / 448, 2^-60), codes =
// e4m3(t / s) through mx_encode (mx_format.hpp), the sign bit of a code the sign bit of t -- over other sets (include/inc_mi355x.h has
// the specification).  The kernels are a file of their own, not a part of sq.hip, because this file is built with
// the packed fp32 instructions off (Makefile) and sq.hip keeps the build it has.
// 16 lanes own one row of 128 elements, 8 elements each (one 16-byte load of a 16-bit input, two of fp32; one 8-byte store of codes),
// so a group's maximum is four shuffle steps inside the wave, with no LDS, and a block's is the workgroup's: every value is read from
// HBM once and stays in registers between the maximum and the rounding.  An input that is not 16-byte aligned, or whose K is no
// multiple of 8, takes the element path.  max is order-free: codes and scales have one right answer, bit for bit.
// Algorithmic bytes: the input once, rows * Kp of codes, 4 bytes per scale.
#include <math.h>

#include "mx_format.hpp"

namespace {

// the 8 values at kb .. kb + 7 of a row that starts at element `row`, 0 from K on -> their abs-max.  vec: K % 8 == 0 and x is 16-byte
// aligned, so that every 8 lie in one aligned 16 (32) bytes
template <int DT>
__device__ __forceinline__ float block_load8(const void* __restrict__ x, int64_t row, int64_t kb, int64_t K, bool vec, float (&v)[8]) {
  if (vec && kb < K) {
    if constexpr (DT == INC_F32) {
      const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + row + kb);
      const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + row + kb + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
      const uint4 u = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(x) + row + kb);
      const uint32_t r[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (DT == INC_BF16) {
          v[2 * j] = __uint_as_float(r[j] << 16);
          v[2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u);
        } else {
          v[2 * j] = f16_bits_to_f32((uint16_t)(r[j] & 0xffffu));
          v[2 * j + 1] = f16_bits_to_f32((uint16_t)(r[j] >> 16));
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (kb + j < K) ? load_as_f32<DT>(x, row + kb + j) : 0.f;
  }
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  return amax;
}

__device__ __forceinline__ float block_scale(float amax) { return fmaxf(amax / 448.0f, 0x1p-60f); }

__device__ __forceinline__ uint2 fp8_pack8(const float (&t)[8], float s) {
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j >> 2] |= mx_encode<INC_MX_FP8_E4M3>(t[j] / s, __float_as_uint(t[j]) >> 31) << (8 * (j & 3));
  return make_uint2(w[0], w[1]);
}

// groups: 16 groups per workgroup, group gi = m * KB + g in the order of `scales`
template <int DT>
__global__ __launch_bounds__(256) void fp8_quant_groups_kernel(const void* __restrict__ x, int64_t M, int64_t K, int64_t Kp,
                                                               uint8_t* __restrict__ codes, float* __restrict__ scales) {
  const int64_t KB = Kp / 128;
  const int64_t gi = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = gi < M * KB;  // a dead group is 16 whole lanes: they take part in the shuffles and touch no memory
  const int64_t m = live ? gi / KB : 0, g = live ? gi % KB : 0;
  const int64_t kb = g * 128 + 8 * (threadIdx.x & 15);
  const bool vec = (K % 8) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float amax = 0.f;
  if (live) amax = block_load8<DT>(x, m * K, kb, K, vec, t);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if (!live) return;
  const float s = block_scale(amax);
  *reinterpret_cast<uint2*>(codes + m * Kp + kb) = fp8_pack8(t, s);
  if ((threadIdx.x & 15) == 0) scales[gi] = s;
}

// blocks: workgroup b = nb * KB + kblk owns rows 128 nb .. x columns 128 kblk ..: 16 rows per pass, the 8 passes held in registers
template <int DT>
__global__ __launch_bounds__(256) void fp8_quant_blocks_kernel(const void* __restrict__ w, int64_t N, int64_t K, int64_t Kp,
                                                               uint8_t* __restrict__ codes, float* __restrict__ scales) {
  __shared__ float red[4];
  const int64_t KB = Kp / 128;
  const int64_t nb = blockIdx.x / KB, kblk = blockIdx.x % KB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t kb = kblk * 128 + 8 * (tid & 15);
  const int64_t n_first = nb * 128 + (tid >> 4);
  const bool vec = (K % 8) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  float t[8][8];
  float amax = 0.f;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int64_t n = n_first + 16 * p;
    if (n < N) amax = fmaxf(amax, block_load8<DT>(w, n * K, kb, K, vec, t[p]));
  }
  amax = wave_max(amax);
  if (lane == 0) red[wave] = amax;
  __syncthreads();
  const float s = block_scale(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int64_t n = n_first + 16 * p;
    if (n < N) *reinterpret_cast<uint2*>(codes + n * Kp + kb) = fp8_pack8(t[p], s);
  }
  if (tid == 0) scales[blockIdx.x] = s;
}

// the checks both quantisers share, in inc_fp8_quant_rows's order
int fp8_block_quant_check(const void* x, int xdtype, int64_t rows, int64_t K, int64_t Kp, const void* codes, const void* scales) {
  INC_CHECK_ARG(x && codes && scales && rows > 0 && K > 0 && Kp >= K);
  if (xdtype != INC_F32 && xdtype != INC_F16 && xdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  if ((Kp % INC_MX_KTILE) != 0) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(rows <= 0x7fffffff && Kp <= 0x7fffffff);
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(codes) & 15) == 0 && (reinterpret_cast<uintptr_t>(scales) & 3) == 0);
  return INC_OK;
}

}  // namespace

extern "C" int inc_fp8_quant_groups(const void* x, int xdtype, int64_t M, int64_t K, int64_t Kp, uint8_t* codes, float* scales,
                                    inc_stream_t stream) {
  const int rc = fp8_block_quant_check(x, xdtype, M, K, Kp, codes, scales);
  if (rc != INC_OK) return rc;
  const int64_t grid = ceil_div64(M * (Kp / 128), 16);
  INC_CHECK_ARG(grid < ((int64_t)1 << 31));
  INC_DISPATCH_DTYPE(xdtype, DT, { fp8_quant_groups_kernel<DT><<<(unsigned)grid, 256, 0, inc_s(stream)>>>(x, M, K, Kp, codes, scales); })
  INC_LAUNCH_RETURN();
}

extern "C" int inc_fp8_quant_blocks(const void* w, int wdtype, int64_t N, int64_t K, int64_t Kp, uint8_t* codes, float* scales,
                                    inc_stream_t stream) {
  const int rc = fp8_block_quant_check(w, wdtype, N, K, Kp, codes, scales);
  if (rc != INC_OK) return rc;
  const int64_t grid = ceil_div64(N, 128) * (Kp / 128);
  INC_CHECK_ARG(grid < ((int64_t)1 << 31));
  INC_DISPATCH_DTYPE(wdtype, DT, { fp8_quant_blocks_kernel<DT><<<(unsigned)grid, 256, 0, inc_s(stream)>>>(w, N, K, Kp, codes, scales); })
  INC_LAUNCH_RETURN();
}
