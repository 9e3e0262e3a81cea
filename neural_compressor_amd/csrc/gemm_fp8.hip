// gemm_fp8.hip -- K17: the per-token / per-channel FP8 (OCP e4m3) GEMM on the f8f6f4 matrix instructions of gfx950.
//
//   y[m, n] = rd16((row_scale[m] * alpha[n]) * sum_k x[m,k] * w[n,k]  +  bias[n])
//
// xq / wq are the e4m3 codes and row_scale / alpha the fp32 scales of inc_fp8_quant_rows (include/inc_mi355x.h has the specification,
// DESIGN section 8c).  The codes are the MX cell's fp8 codes without block scales, so inc_fp8_gemm is gemm_mx.hip's kernel of the
// (fp8, fp8) pair with the scale path taken out -- no scale pointers, no scale loads, no scale registers -- and the two factors applied
// in the epilogue, as inc_w8a8_gemm_rowscale applies them: the wave frame of tile256_frame.hpp, 256 x 256 x 128 tiles, both operands
// K-contiguous rows of 128 bytes through MxStage<128> (mx_stage.hpp), two stages, the DMA of tile t+1 issued at the top of step t, one
// workgroup per tile, no split-K tail.  16 x v_mfma_f32_32x32x64_f8f6f4 per wave and K-tile.  The decode route for 1 <= M <= 16
// (inc_fp8_gemv and its group launches) is gemm_fp8_group.hip.
// The instruction is issued through the scale builtin with literal zero scale operands, which the compiler emits as the UNSCALED opcode
// (no scale register); tools/mx_lab.hip shows on the device that it equals the scaled opcode with both scale bytes 127 bit for bit
// (profiles/mx/mx_lab.log), so the accumulator is what inc_mx_gemm computes for scale bytes 127.
// Operand map: gemm_mx.hip.  Rows past M / N re-read the last row; what they produce is never stored.
// Algorithmic work per launch: 2*M*N*Kp flop; bytes (M + N) * Kp + 4 * (M + N) + 2*M*N.
#include "mx_stage.hpp"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int FM = 256, FN = 256, XK = INC_MX_KTILE;  // the tile
constexpr int E4M3 = INC_MX_FP8_E4M3;

template <bool IS_BF16>
__global__ __launch_bounds__(512) void fp8_gemm_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ row_scale,
                                                       const uint8_t* __restrict__ wq, const float* __restrict__ alpha,
                                                       const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t M,
                                                       int64_t N, int64_t Kp, int y_vec_ok) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ST = MxStage<XK>;
  constexpr int STAGE = 2 * ST::TILE;
  const int tiles_n = (int)((N + FN - 1) / FN);
  const int tiles_m = (int)((M + FM - 1) / FM);
  const int tiles = tiles_m * tiles_n;
  const int wg = xcd_remap(blockIdx.x, tiles);
  int tm, tn;
  banded_tile_decode(wg, tiles_m, tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * FM, n0 = (int64_t)tn * FN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;

  uint32_t xoff[ST::NI], woff[ST::NI];
  ST::offsets(wave, lane, m0, M, Kp, xoff);
  ST::offsets(wave, lane, n0, N, Kp, woff);
  const uint8_t* const xtile = xq + m0 * Kp;
  const uint8_t* const wtile = wq + n0 * Kp;
  const int nk = (int)(Kp / XK);
  auto issue = [&](int kt, int stage) {
    kt = kt > nk - 1 ? nk - 1 : kt;
    ST::issue(xtile + (int64_t)kt * XK, lds0 + stage * STAGE, wave, xoff);
    ST::issue(wtile + (int64_t)kt * XK, lds0 + stage * STAGE + ST::TILE, wave, woff);
  };

  const int hi = lane >> 5;
  const int x_row = wm * 128 + (lane & 31);
  const int w_row = wn * 64 + (lane & 31);
  const int sw = ST::swz(lane & 31);  // row bases are multiples of 32: the swizzle bits are the lane's

  f32x16 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < nk; ++t) {
    const char* S = smem + (t & 1) * STAGE;
    issue(t + 1, (t + 1) & 1);  // the other stage was last read in step t-1, which every wave left through the barrier
    i32x8 xa[2][4], wa[2][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) xa[kk][mf] = ST::frag(S, x_row + 32 * mf, kk, hi, sw);
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) wa[kk][nf] = ST::frag(S + ST::TILE, w_row + 32 * nf, kk, hi, sw);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
          acc[nf][mf] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa[kk][nf], xa[kk][mf], acc[nf][mf], E4M3, E4M3, 0, 0, 0, 0);
    // the MFMAs and the waits for their LDS reads stay in front of the barrier that frees this stage
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 has landed (this wave's share; the barrier covers the rest)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }

  // the row factors of the lane's 4 rows once, the column factors and the bias once per column quad
  float rs[4];
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
    const int64_t m = m0 + wm * 128 + mf * 32 + (lane & 31);
    rs[mf] = m < M ? row_scale[m] : 0.f;
  }
  struct Cols { float al[4], bv[4]; };
  tile256_walk(
      m0, n0, wm, wn, lane,
      [&](int64_t nb) {
        Cols c;
        const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c.al[e] = nb + e < N ? alpha[nb + e] : 0.f;
          c.bv[e] = bq.b[e];
        }
        return c;
      },
      [&](int nf, int mf, int rq, int64_t m, int64_t nb, const Cols& c) {
        if (m >= M) return;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (rs[mf] * c.al[e]) * acc[nf][mf][4 * rq + e] + c.bv[e];
        store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
      });
}

// the argument checks, in inc_mx_gemm's order
int fp8_check(const void* xq, const void* row_scale, const void* wq, const void* alpha, const void* y, int ydtype, int64_t M, int64_t N,
              int64_t Kp) {
  INC_CHECK_ARG(xq && row_scale && wq && alpha && y && M > 0 && N > 0 && Kp > 0);
  if (ydtype != INC_BF16 && ydtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(row_scale) | reinterpret_cast<uintptr_t>(alpha)) & 3) == 0);
  return INC_OK;
}

}  // namespace

extern "C" int inc_fp8_gemm(const uint8_t* xq, const float* row_scale, const uint8_t* wq, const float* alpha, const void* bias, void* y,
                            int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  const int rc = fp8_check(xq, row_scale, wq, alpha, y, ydtype, M, N, Kp);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG((int64_t)FM * Kp < ((int64_t)1 << 32));  // 32-bit DMA offsets inside a tile
  INC_CHECK_ARG(ceil_div64(M, FM) * ceil_div64(N, FN) < ((int64_t)1 << 31));
  const size_t smem = (size_t)2 * 2 * MxStage<XK>::TILE;  // 128 KiB
  static std::atomic<uint64_t> attr_set{0};
  if (inc_attr_needed(attr_set)) {
    (void)hipFuncSetAttribute((const void*)fp8_gemm_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    (void)hipFuncSetAttribute((const void*)fp8_gemm_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    inc_attr_done(attr_set);
  }
  const unsigned grid = (unsigned)(ceil_div64(M, FM) * ceil_div64(N, FN));
  const int y_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  if (ydtype == INC_BF16)
    fp8_gemm_kernel<true><<<grid, 512, smem, inc_s(stream)>>>(xq, row_scale, wq, alpha, (const uint16_t*)bias, (uint16_t*)y, M, N, Kp, y_vec_ok);
  else
    fp8_gemm_kernel<false><<<grid, 512, smem, inc_s(stream)>>>(xq, row_scale, wq, alpha, (const uint16_t*)bias, (uint16_t*)y, M, N, Kp, y_vec_ok);
  INC_LAUNCH_RETURN();
}
