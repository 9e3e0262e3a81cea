// mx_stage.hpp -- the row stage of tile256_frame.hpp as the f8f6f4 MFMA GEMMs use it (gemm_mx.hip, gemm_fp8.hip): a K-tile of 128
// elements issued as single 1 KiB LDS-DMA pieces, and the operand of v_mfma_[scale_]f32_32x32x64_f8f6f4 read back from it.  The
// operand maps are pinned in tools/mx_lab.hip (profiles/mx/mx_lab.log).
#pragma once
#include "tile256_frame.hpp"

typedef __attribute__((ext_vector_type(8))) int i32x8;

// RB = bytes of one row of one K-tile: 128 (fp8) or 64 (fp4); 96 (fp6) is the specialisation below
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

// RB = 96: a K-tile row of an fp6 operand, four blocks of 24 bytes = six 16-byte chunks.  RowStage cannot express it -- a 1 KiB piece
// is 10 2/3 rows and neither of its swizzle rules applies -- so the stage is written out with the same members.
//   image     row-major, row R at byte 96 R = 16-byte slots 6 R .. 6 R + 5; the tile is 24 KiB = 24 pieces, NI = 3 per wave.  Slot s of
//             the tile (lane-linear: piece s >> 6, lane s & 63) is filled from row R = s / 6, chunk (s % 6) ^ swz(R), swz(R) = bit 3
//             of R: a swizzle on the SOURCE chunk index, which stays inside the row (0^1, 2^3, 4^5), so global reads stay whole
//             96-byte row segments.
//   reads     block b = 2 kk + h of a row is bytes 24 b .. 24 b + 23: one WHOLE chunk cf = 3 kk + 2 h (0, 2, 3, 5) and one HALF of
//             chunk ch = 3 kk + 1 (1, 4; low half for h = 0, high for h = 1): ds_read_b128 + ds_read_b64, both naturally aligned --
//             the form the 8-byte alignment of a block allows without a third instruction.  For h = 0 the string is (whole, half),
//             for h = 1 (half, whole): six selects on the lane half put it in registers 0 .. 5; 6 and 7 are zero (not read).
//   banks     a 256-byte bank window is 16 slots.  Unswizzled, slot 6 R + c mod 16 takes 8 values over 16 consecutive rows (6 R mod 16
//             = 0 6 12 2 8 14 4 10, then again): rows R and R + 8 collide, a 2-way conflict on every b128.  With chunk c ^ bit 3 of R
//             the second eight rows land on the other parity: 16 consecutive rows read 16 different slots, the b128 is
//             conflict-free.  The b64 of 32 rows with the SAME half can reach only 16 of the window's 32 8-byte units at this slot
//             granularity: it stays 2-way -- 8 + 8 clocks per fragment against 12 for an ideal 24 bytes, and against 24 for three
//             b64 on this image.  (Weighed and not built: a block-major [block][row][24 B] image, whose 3 R unit stride is
//             conflict-free for three b64 but needs the 12-byte LDS-DMA form; rows padded to 128 bytes, which move fp8's bytes.)
template <>
struct MxStage<96> {
  static constexpr int NI = 3, CPR = 6, TILE = 256 * 96;
  __device__ static __forceinline__ int swz(int row) { return (row >> 3) & 1; }
  __device__ static __forceinline__ void offsets(int wave, int lane, int64_t r0, int64_t rows, int64_t ld, uint32_t (&off)[NI]) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int s = (wave * NI + i) * 64 + lane;  // < 24 * 64 = 256 * 6
      const int R = s / CPR;
      const int c = (s - R * CPR) ^ swz(R);
      int64_t r = r0 + R;
      if (r > rows - 1) r = rows - 1;
      off[i] = (uint32_t)((r - r0) * ld + 16 * c);
    }
  }
  __device__ static __forceinline__ void issue(const uint8_t* src, uint32_t lds_tile, int wave, const uint32_t (&off)[NI]) {
#pragma unroll
    for (int i = 0; i < NI; ++i) lds_dma_1k(src, __builtin_amdgcn_readfirstlane(lds_tile + (wave * NI + i) * 1024), off[i]);
  }
  __device__ static __forceinline__ i32x8 frag(const char* tile, int row, int kk, int h, int sw) {
    const char* r = tile + row * 96;
    const uint4 w = *reinterpret_cast<const uint4*>(r + (((3 * kk + 2 * h) ^ sw) << 4));
    const uint2 p = *reinterpret_cast<const uint2*>(r + (((3 * kk + 1) ^ sw) << 4) + 8 * h);
    i32x8 f;
    f[0] = (int)(h ? p.x : w.x); f[1] = (int)(h ? p.y : w.y);
    f[2] = (int)(h ? w.x : w.z); f[3] = (int)(h ? w.y : w.w);
    f[4] = (int)(h ? w.z : p.x); f[5] = (int)(h ? w.w : p.y);
    f[6] = 0; f[7] = 0;
    return f;
  }
};
