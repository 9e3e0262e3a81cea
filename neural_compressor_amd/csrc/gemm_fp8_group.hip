// gemm_fp8_group.hip -- K17 / K17g: the decode launches of the per-token / per-channel FP8 cell, one or more weight matrices against the
// SAME 1 <= M <= 16 rows of x, on v_mfma_f32_16x16x128_f8f6f4.
//
//   inc_fp8_gemv         y[m, n]   = rd16((row_scale[m] * alpha[n]) * sum_k x[m,k] * w[n,k]  +  bias[n])
//   inc_fp8_gemv_multi   y_i[m, n] = the same of member i,                                                            i = 0 .. n-1, 2 <= n <= 8
//   inc_fp8_gemv_gated   h[m, n]   = rd16( silu(g) * u ),  silu(g) * u = g / (1.f + expf(-g)) * u  (silu_mul_f32 of common.hpp), with
//                        g = (row_scale[m] * alpha_gate[n]) * sum_k x[m,k] * w_gate[n,k]  +  bias_gate[n]
//                        u = (row_scale[m] * alpha_up[n])   * sum_k x[m,k] * w_up[n,k]    +  bias_up[n]
//
// xq / wq are the e4m3 codes and row_scale / alpha the fp32 scales of inc_fp8_quant_rows (include/inc_mi355x.h has the specification,
// DESIGN section 8c).  The codes are the MX cell's fp8 codes without block scales, so every sum is gemm_mx_gemv.hip's for the
// (fp8, fp8) pair with the scale path taken out (strip_frame.hpp, SCALED = false): one workgroup per 16 output columns, K split over
// 8 waves, wave 0 adds the 8 partials in wave order.  The epilogue is fp8_quad of the frame.  No workspace, no counters: repeated
// calls are bit-identical.  The number of K-tiles a wave has in flight per round differs between the kernels; it changes no sum
// order.  The wave count is fixed: the identities below rest on it.
//   gemv    one weight matrix.  It keeps a kernel of its own in written-out form (the note at the kernel says why).
//   multi   a workgroup finds its member in a table passed by value (StripMembers) and runs the same fp8_gemv_strip, so y_i is
//           inc_fp8_gemv's output on member i bit for bit.
//   gated   both weights are [N, Kp]; a workgroup owns strip s of gate AND strip s of up: a wave loads its x fragment once per K-tile
//           and issues two MFMAs into two accumulators, the two partial sets meet in LDS (16 KiB), and wave 0 forms g and u -- each
//           inc_fp8_gemv's value before its rounding -- and the SiLU product in fp32 and rounds ONCE.  Without a bias g, u and h are
//           those of inc_fp8_moe_gemm's mode 0 for one expert with weight cat(gate, up) and alpha cat(alpha_gate, alpha_up), bit for
//           bit (the same sums, the same epilogue).  Against the unfused modules (round g, round u, silu rounds, mul rounds) h
//           differs by those three roundings.
//           Range: below g ~ -88.7 expf(-g) overflows to +inf and silu(g) is -0 where the exact value is about -1e-37 or smaller in
//           magnitude -- under the smallest bf16 / fp16 step, so h is right after rounding; g = -inf gives NaN (-inf / inf), as in
//           the experts kernels.
// Lanes of an x row >= M supply zero codes, lanes of a weight row >= N re-read row N - 1; what they produce is never stored.
// Algorithmic bytes per launch: sum_i N_i * Kp + M * Kp + 4 * (M + sum_i N_i) + 2 * M * sum_i N_i (gated: the weights of both, one h).
#include "strip_frame.hpp"

namespace {

constexpr int GW = 8;  // waves of a workgroup = ways of the in-workgroup K split: fixed
constexpr int E4M3 = INC_MX_FP8_E4M3;
// K-tiles of a wave whose loads are in flight together.  One weight strip: 4 (64 fragment registers), with the cascade tail.  Gate +
// up: 24 fragment registers per tile; 2 is the experts kernel's depth for two strips and one row block (moe_unroll,
// gemm_strip_moe.hip) and keeps as many weight bytes in flight per wave as the single strip at 4.  3 and 4 measured within 3 % of it
// (profiles/fp8/fp8_gated_unroll_ab.log; 58 VGPRs at 2, 62 at 3, 86 at 4).  Resources of both kernels: DESIGN section 8c.
constexpr int UNROLL_MULTI = 4;
#ifndef INC_FP8_GATED_UNROLL
#define INC_FP8_GATED_UNROLL 2
#endif
constexpr int UNROLL_GATED = INC_FP8_GATED_UNROLL;

using Fp8GemvMembers = StripMembers<float>;  // ws: the member's alpha

// one strip of one weight matrix: the body of every member of inc_fp8_gemv_multi
template <bool IS_BF16>
__device__ __forceinline__ void fp8_gemv_strip(const uint8_t* xq, const float* row_scale, const uint8_t* wq, const float* alpha,
                                               const uint16_t* bias, uint16_t* y, int M, int64_t N, int64_t Kp, int y_vec_ok, int64_t n0) {
  __shared__ f32x4 part[1][GW][64];
  const StripLane L = strip_lane(n0, N, M);
  const int nk = (int)(Kp / XK);
  const StripRow w[1] = {strip_row<E4M3, false>(wq, nullptr, L.wrow, nk, L.g)};
  const StripRow x[1] = {strip_row<E4M3, false>(xq, nullptr, L.xrow, nk, L.g)};

  f32x4 acc[1][1] = {{{0.f, 0.f, 0.f, 0.f}}}, sum[1];
  strip_partials<E4M3, E4M3, false, 1, 1, UNROLL_MULTI, GW, true, true>(w, x, L.xkeep, L.wave, nk, acc);
  strip_sum_wave0(part, acc, L.wave, L.lane, sum);
  if (L.wave != 0) return;

  const int m = L.r;
  if (m >= M) return;
  const int64_t nb = n0 + 4 * L.g;
  if (nb >= N) return;
  float v[4];
  fp8_quad<IS_BF16>(row_scale[m], alpha, bias, nb, N, sum[0], v);
  store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
}

// inc_fp8_gemv's kernel is kept in written-out form: fp8_gemv_strip in the parent's own text (its K loop is strip_partials<E4M3, E4M3,
// false, 1, 1, 4, GW, true, true>, its sum strip_sum_wave0, its epilogue fp8_quad).  As a thin call of fp8_gemv_strip it measured
// 1.3 - 3.9 % slower at N = 13824, K = 5120 on three visits, through the multi kernel 0.4 us per launch slower
// (profiles/strip_frame/README.md).  Any change of the tile-to-wave map, the K order or the sum order is made in strip_frame.hpp too.
template <bool IS_BF16>
__global__ __launch_bounds__(GW * 64) void fp8_gemv_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ row_scale,
                                                           const uint8_t* __restrict__ wq, const float* __restrict__ alpha,
                                                           const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M,
                                                           int64_t N, int64_t Kp, int y_vec_ok) {
  __shared__ f32x4 part[GW][64];
  const int64_t n0 = (int64_t)blockIdx.x * STRIP;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  int64_t wrow = n0 + r;
  if (wrow > N - 1) wrow = N - 1;
  const int xrow = r < M ? r : M - 1;
  const int xkeep = r < M ? -1 : 0;
  const uint8_t* const wp = wq + wrow * Kp + 16 * g;
  const uint8_t* const xp = xq + (int64_t)xrow * Kp + 16 * g;
  const int nk = (int)(Kp / XK);

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // C rounds of the wave's K-tiles kt, kt + GW, ...: every load first, then the MFMAs in K order
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[C], xf[C];
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * GW;
      wf[u] = mx_frag<E4M3, true>(wp + t * XK);
      xf[u] = mx_frag<E4M3, false>(xp + t * XK);
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
#pragma unroll
      for (int d = 0; d < 8; ++d) xf[u][d] &= xkeep;
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[u], xf[u], acc, E4M3, E4M3, 0, 0, 0, 0);
    }
  };
  int kt = wave;
  for (; kt + (UNROLL_MULTI - 1) * GW < nk; kt += UNROLL_MULTI * GW) round(kt, std::integral_constant<int, UNROLL_MULTI>{});
  const int left = kt < nk ? (nk - kt + GW - 1) / GW : 0;  // 0 .. UNROLL_MULTI - 1 tiles of this wave remain
  if (left == 3) round(kt, std::integral_constant<int, 3>{});
  else if (left == 2) round(kt, std::integral_constant<int, 2>{});
  else if (left == 1) round(kt, std::integral_constant<int, 1>{});

  part[wave][lane] = acc;
  __syncthreads();
  if (wave != 0) return;
  f32x4 sum = part[0][lane];
#pragma unroll
  for (int w = 1; w < GW; ++w) sum += part[w][lane];

  // C/D map of the 16 x 16 MFMA: register e of lane l is D[4 (l >> 4) + e][l & 15] = y[m = l & 15][n0 + 4 g + e]
  const int m = r;
  if (m >= M) return;
  const int64_t nb = n0 + 4 * g;
  if (nb >= N) return;
  const float rs = row_scale[m];
  const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float al = nb + e < N ? alpha[nb + e] : 0.f;
    v[e] = (rs * al) * sum[e] + bq.b[e];
  }
  store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
}

template <bool IS_BF16>
__global__ __launch_bounds__(GW * 64) void fp8_gemv_multi_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ row_scale,
                                                                 const Fp8GemvMembers mem, int M, int64_t Kp) {
  const int strip = blockIdx.x;
  const int mi = strip_member(mem, strip);
  fp8_gemv_strip<IS_BF16>(xq, row_scale, mem.wq[mi], mem.ws[mi], mem.bias[mi], mem.y[mi], M, mem.N[mi], Kp, mem.y_vec_ok[mi],
                          (int64_t)(strip - mem.first[mi]) * STRIP);
}

template <bool IS_BF16>
__global__ __launch_bounds__(GW * 64) void fp8_gemv_gated_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ row_scale,
                                                                 const uint8_t* __restrict__ wq_gate, const float* __restrict__ alpha_gate,
                                                                 const uint16_t* __restrict__ bias_gate, const uint8_t* __restrict__ wq_up,
                                                                 const float* __restrict__ alpha_up, const uint16_t* __restrict__ bias_up,
                                                                 uint16_t* __restrict__ h, int M, int64_t N, int64_t Kp, int h_vec_ok) {
  __shared__ f32x4 part[2][GW][64];  // gate's and up's partials: 16 KiB
  const int64_t n0 = (int64_t)blockIdx.x * STRIP;
  const StripLane L = strip_lane(n0, N, M);
  const int nk = (int)(Kp / XK);
  const StripRow w[2] = {strip_row<E4M3, false>(wq_gate, nullptr, L.wrow, nk, L.g), strip_row<E4M3, false>(wq_up, nullptr, L.wrow, nk, L.g)};
  const StripRow x[1] = {strip_row<E4M3, false>(xq, nullptr, L.xrow, nk, L.g)};

  f32x4 acc[2][1] = {{{0.f, 0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f, 0.f}}}, sum[2];
  strip_partials<E4M3, E4M3, false, 2, 1, UNROLL_GATED, GW, true, UNROLL_GATED == 4>(w, x, L.xkeep, L.wave, nk, acc);
  strip_sum_wave0(part, acc, L.wave, L.lane, sum);
  if (L.wave != 0) return;

  const int m = L.r;
  if (m >= M) return;
  const int64_t nb = n0 + 4 * L.g;
  if (nb >= N) return;
  const float rs = row_scale[m];
  float gv[4], uv[4], v[4];
  fp8_quad<IS_BF16>(rs, alpha_gate, bias_gate, nb, N, sum[0], gv);
  fp8_quad<IS_BF16>(rs, alpha_up, bias_up, nb, N, sum[1], uv);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = silu_mul_f32(gv[e], uv[e]);
  store_quad16<IS_BF16>(h, m, nb, N, h_vec_ok, v);
}

// the checks of what the members share, in inc_mx_gemm's order; the per-member ones follow in the entry points
int fp8_group_check_x(const void* xq, const void* row_scale, int ydtype, int64_t M, int64_t Kp) {
  INC_CHECK_ARG(xq && row_scale && M > 0 && Kp > 0);
  if (M > INC_MX_GEMV_MAX_M) return INC_ERR_UNSUPPORTED;
  if (ydtype != INC_BF16 && ydtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(xq) & 15) == 0 && (reinterpret_cast<uintptr_t>(row_scale) & 3) == 0);
  return INC_OK;
}

bool fp8_group_member_aligned(const void* wq, const void* alpha) {
  return (reinterpret_cast<uintptr_t>(wq) & 15) == 0 && (reinterpret_cast<uintptr_t>(alpha) & 3) == 0;
}

}  // namespace

extern "C" int inc_fp8_gemv(const uint8_t* xq, const float* row_scale, const uint8_t* wq, const float* alpha, const void* bias, void* y,
                            int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  INC_CHECK_ARG(xq && row_scale && wq && alpha && y && M > 0 && N > 0 && Kp > 0);
  const int rc = fp8_group_check_x(xq, row_scale, ydtype, M, Kp);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG(fp8_group_member_aligned(wq, alpha));
  INC_CHECK_ARG(ceil_div64(N, STRIP) < ((int64_t)1 << 31));
  const unsigned grid = (unsigned)ceil_div64(N, STRIP);
  const int y_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  if (ydtype == INC_BF16)
    fp8_gemv_kernel<true><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, row_scale, wq, alpha, (const uint16_t*)bias, (uint16_t*)y, (int)M, N, Kp, y_vec_ok);
  else
    fp8_gemv_kernel<false><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, row_scale, wq, alpha, (const uint16_t*)bias, (uint16_t*)y, (int)M, N, Kp, y_vec_ok);
  INC_LAUNCH_RETURN();
}

extern "C" int inc_fp8_gemv_multi(int n, const uint8_t* xq, const float* row_scale, const uint8_t* const* wq, const float* const* alpha,
                                  const void* const* bias, void* const* y, int ydtype, int64_t M, const int64_t* N, int64_t Kp,
                                  inc_stream_t stream) {
  INC_CHECK_ARG(wq && alpha && y && N);
  if (n < 2 || n > STRIP_MAX_MEMBERS) return INC_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) INC_CHECK_ARG(wq[i] && alpha[i] && y[i] && N[i] > 0);
  const int rc = fp8_group_check_x(xq, row_scale, ydtype, M, Kp);
  if (rc != INC_OK) return rc;
  Fp8GemvMembers mem = {};
  const int rf = strip_members_fill(mem, n, wq, alpha, bias, y, N);
  if (rf != INC_OK) return rf;
  const unsigned grid = (unsigned)mem.first[n];
  if (ydtype == INC_BF16)
    fp8_gemv_multi_kernel<true><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, row_scale, mem, (int)M, Kp);
  else
    fp8_gemv_multi_kernel<false><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, row_scale, mem, (int)M, Kp);
  INC_LAUNCH_RETURN();
}

extern "C" int inc_fp8_gemv_gated(const uint8_t* xq, const float* row_scale, const uint8_t* wq_gate, const float* alpha_gate,
                                  const void* bias_gate, const uint8_t* wq_up, const float* alpha_up, const void* bias_up, void* h,
                                  int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  INC_CHECK_ARG(xq && row_scale && wq_gate && alpha_gate && wq_up && alpha_up && h && M > 0 && N > 0 && Kp > 0);
  const int rc = fp8_group_check_x(xq, row_scale, ydtype, M, Kp);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG(fp8_group_member_aligned(wq_gate, alpha_gate) && fp8_group_member_aligned(wq_up, alpha_up));
  INC_CHECK_ARG(ceil_div64(N, STRIP) < ((int64_t)1 << 31));
  const unsigned grid = (unsigned)ceil_div64(N, STRIP);
  const int h_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(h) & 7) == 0);
  if (ydtype == INC_BF16)
    fp8_gemv_gated_kernel<true><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, row_scale, wq_gate, alpha_gate, (const uint16_t*)bias_gate, wq_up,
                                                                     alpha_up, (const uint16_t*)bias_up, (uint16_t*)h, (int)M, N, Kp,
                                                                     h_vec_ok);
  else
    fp8_gemv_gated_kernel<false><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, row_scale, wq_gate, alpha_gate, (const uint16_t*)bias_gate, wq_up,
                                                                      alpha_up, (const uint16_t*)bias_up, (uint16_t*)h, (int)M, N, Kp,
                                                                      h_vec_ok);
  INC_LAUNCH_RETURN();
}
