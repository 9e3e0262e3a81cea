// tile256_frame.hpp -- the wave frame every 256 x 256 MFMA GEMM of the library is built on (gemm_tile256.hip, gemm_i8.hip, gemm_mx.hip, gemm_fp8.hip,
// tools/kbench_gemm_1.inc; gemm_d2r.hip and tools/gemm_d2r8.hip take the row stage only).  A kernel file keeps what is its own -- the
// K-loop schedule, the MFMA, the dequantisation or scales -- and takes the rest from here.
//
//   wave grid   512 threads = 8 waves as 2 (M) x 4 (N): wave w has wm = w >> 2, wn = w & 3 and owns rows 128 wm .. + 127 x columns
//               64 wn .. + 63 of the tile = 4 (mf) x 2 (nf) MFMA 32 x 32 tiles, acc[nf][mf].
//   operands    W is the A operand and x the B operand of the MFMA, so the accumulator's rows are output COLUMNS: a lane owns 4
//               consecutive output columns per accumulator quad and stores them as 8 bytes.
//   LDS image   an operand whose rows are K-contiguous (x always; W too where it is not dequantised) is a tile of 256 rows x RB bytes
//               (RB = 128 or 64 bytes of one K-tile), row-major, brought in by LDS-DMA in 1 KiB pieces of 1024 / RB whole rows; piece
//               i of wave w is piece w * NI + i of the tile.  The DMA destination is lane-linear, so the swizzle is applied to the
//               per-lane SOURCE address and again on the ds_read_b128 side: the 16-byte chunk c of row R sits in slot c ^ swz(R),
//               swz(R) = bits 1..3 of R for 128-byte rows and bits 2..3 for 64-byte rows.  16 consecutive rows then read 16 different
//               16-byte slots of a 256-byte bank window (no bank conflicts) and the global reads stay full lines.  Rows past the
//               operand's last real row re-read that row; what is computed from them is never stored.
//   C/D map     epilogue: D row i = n-offset (r&3) + 8*(r>>2) + 4*(lane>>5), col j = m-offset lane&31 -- register r of acc[nf][mf] is
//               y[m0 + 128 wm + 32 mf + (lane & 31)][n0 + 64 wn + 32 nf + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)], so the quad rq = r >> 2
//               is 4 adjacent columns starting at nb = n0 + 64 wn + 32 nf + 8 rq + 4 (lane >> 5).
#pragma once
#include "common.hpp"

// One swizzled operand tile: 256 rows of RB bytes, NI 1 KiB pieces per wave (RB / 32 with eight waves: 4 at RB = 128, 2 at RB = 64; 8
// for the four waves of gemm_d2r.hip).  How the pieces are issued (lds_dma_4x1k, lds_dma_1k, an asm macro) is the kernel's choice.
template <int RB, int NI_ = RB / 32>
struct RowStage {
  static constexpr int NI = NI_, RPI = 1024 / RB, CPR = RB / 16;
  static constexpr int TILE = 256 * RB;
  __device__ static __forceinline__ int swz(int row) { return RB == 128 ? (row >> 1) & 7 : (row >> 2) & 3; }
  // per-lane source offsets of the wave's pieces: bytes from the tile's first row (r0 of `rows`) at K-tile 0, `ld` = bytes per row
  __device__ static __forceinline__ void offsets(int wave, int lane, int64_t r0, int64_t rows, int64_t ld, uint32_t (&off)[NI]) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int R = (wave * NI + i) * RPI + lane / CPR;
      const int c = (lane % CPR) ^ swz(R);
      int64_t r = r0 + R;
      if (r > rows - 1) r = rows - 1;
      off[i] = (uint32_t)((r - r0) * ld + 16 * c);
    }
  }
  // byte offset inside its row of the 16-byte chunk c, for a ds_read_b128; `sw` = swz(row) (= swz(lane & 31) for the rows of a lane's
  // fragments: their bases are multiples of 32)
  __device__ static __forceinline__ int chunk_off(int c, int sw) { return (c ^ sw) << 4; }
};

// The C/D map as a loop: col(nb) once per column quad (nf, rq) -- where a caller loads what depends on the column only: bias, alpha,
// corr -- then quad(nf, mf, rq, m, nb, what col returned) for the four row blocks.  m may lie past M and nb + 3 past N: the hooks guard.
template <class ColF, class QuadF>
__device__ __forceinline__ void tile256_walk(int64_t m0, int64_t n0, int wm, int wn, int lane, ColF&& col, QuadF&& quad) {
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int64_t nb = n0 + wn * 64 + nf * 32 + 8 * rq + 4 * (lane >> 5);
      const auto c = col(nb);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) quad(nf, mf, rq, m0 + wm * 128 + mf * 32 + (lane & 31), nb, c);
    }
  }
}

// the bias of a column quad as fp32 (0 without a bias and past N)
struct BiasQuad { float b[4]; };
template <bool IS_BF16>
__device__ __forceinline__ BiasQuad load_bias_quad(const uint16_t* bias, int64_t nb, int64_t N) {
  BiasQuad q = {{0.f, 0.f, 0.f, 0.f}};
  if (bias) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (nb + e < N) q.b[e] = IS_BF16 ? bf16_bits_to_f32(bias[nb + e]) : f16_bits_to_f32(bias[nb + e]);
  }
  return q;
}

// y[m][nb .. nb + 3] = v, one rounding each: one 8-byte store where the quad is whole and aligned, guarded element stores otherwise
template <bool IS_BF16>
__device__ __forceinline__ void store_quad16(uint16_t* y, int64_t m, int64_t nb, int64_t N, int y_vec_ok, const float (&v)[4]) {
  uint16_t* dst = y + m * N + nb;
  if (y_vec_ok && nb + 4 <= N) {
    *reinterpret_cast<uint2*>(dst) = make_uint2(cvt_pair<IS_BF16>(v[0], v[1]), cvt_pair<IS_BF16>(v[2], v[3]));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (nb + e < N) dst[e] = IS_BF16 ? f32_to_bf16_bits(v[e]) : f32_to_f16_bits(v[e]);
  }
}
