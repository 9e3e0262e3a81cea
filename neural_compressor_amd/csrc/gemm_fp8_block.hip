// gemm_fp8_block.hip -- K18: the block-scaled FP8 (OCP e4m3) products: 128 x 128 weight blocks, 1 x 128 activation groups, the scheme of
// DeepSeek-V3 / Qwen3-FP8 checkpoints (`weight_scale_inv`), on the f8f6f4 matrix instructions of gfx950.
//
//   y[m, n] = rd16( sum_kt (xs[m, kt] * ws[n / 128, kt]) * acc_kt[m, n]  +  bias[n] ),   acc_kt = the matrix pipe's sum over K-tile kt alone
//
// xq / xs are what inc_fp8_quant_groups writes, wq / ws what inc_fp8_quant_blocks writes or what such a checkpoint stores (include/inc_mi355x.h has
// the specification).  The K-tile of both kernels is 128 elements = one scale block, so the factor changes with every
// K-tile and a tile's sum is promoted into a second fp32 accumulator INSIDE the K loop; that is what sets these kernels apart from
// gemm_fp8.hip / gemm_fp8_group.hip, whose factors wait for the epilogue.  The instruction is the unscaled opcode (literal zero scale
// operands), started from a zero C operand (an inline constant: no register is cleared).
//
// inc_fp8_block_gemm: fp8_gemm_kernel's frame (tile256_frame.hpp, MxStage<128>, 256 x 256 x 128 tiles, two stages, one workgroup per tile).
//   W is the A operand, so the 16 registers of a 32 x 32 fragment of a lane all belong to ONE row m = lane & 31 of x: the x factor is one
//   scalar per lane and mf, and the wave's 64 columns lie inside one 128-column block: the weight factor is one wave-uniform value per
//   K-tile.  Per K-tile and lane: 4 factor products, 16 MFMAs, 128 multiply-adds.  No second set of 128 partial accumulators: per
//   fragment (mf outer, nf inner, so that a pair of x fragments is live at a time) the two kk MFMAs run into a 16-register temporary and
//   the temporary of the fragment BEFORE is promoted behind them, so the promotion's VALU work sits under the next fragment's MFMAs; two
//   temporaries rotate.  The factors of tile t + 1 are loaded with that tile's DMA issue.
// inc_fp8_block_gemv: the strip body of gemm_fp8_group.hip (strip_frame.hpp: lane map, fragments, wave-order sum) for 1 <= M <= 16 with the
//   K loop written out: one v_mfma_f32_16x16x128_f8f6f4 per K-tile and wave into a zero temporary, then 4 multiply-adds with
//   xs[m = lane & 15, kt] * ws[n0 / 128, kt] (a strip of 16 columns never crosses a 128-column block).  The scale loads of a round are
//   issued with its fragment loads.  Wave w takes the tiles w, w + 8, ... ascending, 4 per round with the cascade tail of inc_fp8_gemv;
//   the 8 partials are added in wave order: no workspace, repeated calls are bit-identical.
// Rows of x past M re-read row M - 1 (GEMM) or supply zero codes (GEMV), weight rows past N re-read row N - 1; what they produce is
// never stored.  Algorithmic work per launch: 2*M*N*Kp flop; bytes (M + N) * Kp + 4 * (M + ceil(N/128)) * Kp/128 + 2*M*N.
#include "mx_stage.hpp"
#include "strip_frame.hpp"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int FM = 256, FN = 256;  // the tile (K: XK = 128 = one scale block)
constexpr int WB = 128;            // rows of a weight scale block
constexpr int GW = 8;              // waves of a GEMV workgroup = ways of its K split: fixed, as in gemm_fp8_group.hip
constexpr int GU = 4;              // K-tiles of a wave in flight per GEMV round
constexpr int E4M3 = INC_MX_FP8_E4M3;

template <bool IS_BF16>
__global__ __launch_bounds__(512) void fp8_block_gemm_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ xs,
                                                             const uint8_t* __restrict__ wq, const float* __restrict__ ws,
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

  // the factors: the lane's 4 rows of xs (clamped like the rows of xq) and the wave's row of ws
  const float* xsp[4];
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
    int64_t m = m0 + wm * 128 + mf * 32 + (lane & 31);
    m = m > M - 1 ? M - 1 : m;
    xsp[mf] = xs + m * nk;
  }
  int64_t wblk = (n0 + wn * 64) / WB;
  wblk = wblk > (N - 1) / WB ? (N - 1) / WB : wblk;
  const float* const wsp = ws + wblk * nk;  // wave-uniform

  float xf[4], wf;
  auto issue = [&](int kt, int stage) {
    kt = kt > nk - 1 ? nk - 1 : kt;
    ST::issue(xtile + (int64_t)kt * XK, lds0 + stage * STAGE, wave, xoff);
    ST::issue(wtile + (int64_t)kt * XK, lds0 + stage * STAGE + ST::TILE, wave, woff);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) xf[mf] = xsp[mf][kt];
    wf = wsp[kt];
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
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < nk; ++t) {
    const char* S = smem + (t & 1) * STAGE;
    float f[4];  // this tile's factors, before the issue overwrites them with the next tile's
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) f[mf] = xf[mf] * wf;
    issue(t + 1, (t + 1) & 1);  // the other stage was last read in step t-1, which every wave left through the barrier
    i32x8 wa[2][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) wa[kk][nf] = ST::frag(S + ST::TILE, w_row + 32 * nf, kk, hi, sw);
    // fragment i = 2 mf + nf: its two MFMAs, then the promotion of fragment i - 1
    f32x16 tmp[2];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (i < 8) {
        const int mf = i >> 1, nf = i & 1;
        const i32x8 xa0 = ST::frag(S, x_row + 32 * mf, 0, hi, sw), xa1 = ST::frag(S, x_row + 32 * mf, 1, hi, sw);
        tmp[i & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa[0][nf], xa0, zero, E4M3, E4M3, 0, 0, 0, 0);
        tmp[i & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa[1][nf], xa1, tmp[i & 1], E4M3, E4M3, 0, 0, 0, 0);
      }
      if (i > 0) {
        const int j = i - 1, mf = j >> 1, nf = j & 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nf][mf][r] = f[mf] * tmp[j & 1][r] + acc[nf][mf][r];
      }
    }
    // the MFMAs and the waits for their LDS reads stay in front of the barrier that frees this stage
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 and its factors have landed (this wave's share; the barrier covers the rest)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }

  tile256_walk(
      m0, n0, wm, wn, lane, [&](int64_t nb) { return load_bias_quad<IS_BF16>(bias, nb, N); },
      [&](int nf, int mf, int rq, int64_t m, int64_t nb, const BiasQuad& bq) {
        if (m >= M) return;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[nf][mf][4 * rq + e] + bq.b[e];
        store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
      });
}

template <bool IS_BF16>
__global__ __launch_bounds__(GW * 64) void fp8_block_gemv_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ xs,
                                                                 const uint8_t* __restrict__ wq, const float* __restrict__ ws,
                                                                 const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M,
                                                                 int64_t N, int64_t Kp, int y_vec_ok) {
  __shared__ f32x4 part[1][GW][64];
  const int64_t n0 = (int64_t)blockIdx.x * STRIP;
  const StripLane L = strip_lane(n0, N, M);
  const int nk = (int)(Kp / XK);
  const uint8_t* const wp = strip_row<E4M3, false>(wq, nullptr, L.wrow, nk, L.g).q;
  const uint8_t* const xp = strip_row<E4M3, false>(xq, nullptr, L.xrow, nk, L.g).q;
  const float* const xsp = xs + (int64_t)L.xrow * nk;  // the lane's accumulator column is row m = lane & 15 of x
  const float* const wsp = ws + (n0 / WB) * nk;        // uniform over the workgroup: n0 < N, a strip lies inside one block

  f32x4 acc[1][1] = {{{0.f, 0.f, 0.f, 0.f}}}, sum[1];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // C of the wave's K-tiles kt, kt + GW, ...: every load first (fragments and factors), then per tile the MFMA and its promotion, in K order
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[C], xf[C];
    float sx[C], sw[C];
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * GW;
      wf[u] = mx_frag<E4M3, true>(wp + t * XK);
      xf[u] = mx_frag<E4M3, false>(xp + t * XK);
      sx[u] = xsp[t];
      sw[u] = wsp[t];
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
#pragma unroll
      for (int d = 0; d < 8; ++d) xf[u][d] &= L.xkeep;
      const f32x4 tmp = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[u], xf[u], zero, E4M3, E4M3, 0, 0, 0, 0);
      const float f = sx[u] * sw[u];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[0][0][e] = f * tmp[e] + acc[0][0][e];
    }
  };
  int kt = L.wave;
  for (; kt + (GU - 1) * GW < nk; kt += GU * GW) round(kt, std::integral_constant<int, GU>{});
  const int left = kt < nk ? (nk - kt + GW - 1) / GW : 0;  // 0 .. GU - 1 tiles of this wave remain
  if (left == 3) round(kt, std::integral_constant<int, 3>{});
  else if (left == 2) round(kt, std::integral_constant<int, 2>{});
  else if (left == 1) round(kt, std::integral_constant<int, 1>{});

  strip_sum_wave0(part, acc, L.wave, L.lane, sum);
  if (L.wave != 0) return;
  const int m = L.r;
  if (m >= M) return;
  const int64_t nb = n0 + 4 * L.g;
  if (nb >= N) return;
  const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = sum[0][e] + bq.b[e];
  store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
}

// the argument checks of both entry points, in inc_fp8_gemm's order; max_m = 0: any M
int fp8_block_check(const void* xq, const void* xs, const void* wq, const void* ws, const void* y, int ydtype, int64_t M, int64_t N,
                    int64_t Kp, int64_t max_m) {
  INC_CHECK_ARG(xq && xs && wq && ws && y && M > 0 && N > 0 && Kp > 0);
  if (max_m && M > max_m) return INC_ERR_UNSUPPORTED;
  if (ydtype != INC_BF16 && ydtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(ws)) & 3) == 0);
  return INC_OK;
}

}  // namespace

extern "C" int inc_fp8_block_gemm(const uint8_t* xq, const float* xs, const uint8_t* wq, const float* ws, const void* bias, void* y,
                                  int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  const int rc = fp8_block_check(xq, xs, wq, ws, y, ydtype, M, N, Kp, 0);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG((int64_t)FM * Kp < ((int64_t)1 << 32));  // 32-bit DMA offsets inside a tile
  INC_CHECK_ARG(ceil_div64(M, FM) * ceil_div64(N, FN) < ((int64_t)1 << 31));
  const size_t smem = (size_t)2 * 2 * MxStage<XK>::TILE;  // 128 KiB
  static std::atomic<uint64_t> attr_set{0};
  if (inc_attr_needed(attr_set)) {
    (void)hipFuncSetAttribute((const void*)fp8_block_gemm_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    (void)hipFuncSetAttribute((const void*)fp8_block_gemm_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    inc_attr_done(attr_set);
  }
  const unsigned grid = (unsigned)(ceil_div64(M, FM) * ceil_div64(N, FN));
  const int y_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  if (ydtype == INC_BF16)
    fp8_block_gemm_kernel<true><<<grid, 512, smem, inc_s(stream)>>>(xq, xs, wq, ws, (const uint16_t*)bias, (uint16_t*)y, M, N, Kp, y_vec_ok);
  else
    fp8_block_gemm_kernel<false><<<grid, 512, smem, inc_s(stream)>>>(xq, xs, wq, ws, (const uint16_t*)bias, (uint16_t*)y, M, N, Kp, y_vec_ok);
  INC_LAUNCH_RETURN();
}

extern "C" int inc_fp8_block_gemv(const uint8_t* xq, const float* xs, const uint8_t* wq, const float* ws, const void* bias, void* y,
                                  int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  const int rc = fp8_block_check(xq, xs, wq, ws, y, ydtype, M, N, Kp, INC_MX_GEMV_MAX_M);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG(ceil_div64(N, STRIP) < ((int64_t)1 << 31));
  const unsigned grid = (unsigned)ceil_div64(N, STRIP);
  const int y_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  if (ydtype == INC_BF16)
    fp8_block_gemv_kernel<true><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, xs, wq, ws, (const uint16_t*)bias, (uint16_t*)y, (int)M, N, Kp, y_vec_ok);
  else
    fp8_block_gemv_kernel<false><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, xs, wq, ws, (const uint16_t*)bias, (uint16_t*)y, (int)M, N, Kp, y_vec_ok);
  INC_LAUNCH_RETURN();
}
