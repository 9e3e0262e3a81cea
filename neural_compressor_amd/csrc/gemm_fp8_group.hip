// gemm_fp8_group.hip -- K17g: the decode GROUP launches of the per-token / per-channel FP8 cell, inc_fp8_gemv's strip body over more
// than one weight matrix that multiplies the SAME 1 <= M <= 16 rows of x, on v_mfma_f32_16x16x128_f8f6f4.
//
//   inc_fp8_gemv_multi   y_i[m, n] = rd16((row_scale[m] * alpha_i[n]) * sum_k x[m,k] * w_i[n,k]  +  bias_i[n])        i = 0 .. n-1, 2 <= n <= 8
//   inc_fp8_gemv_gated   h[m, n]   = rd16( silu(g) * u ),  silu(g) * u = g / (1.f + expf(-g)) * u  (silu_mul_f32 of common.hpp), with
//                        g = (row_scale[m] * alpha_gate[n]) * sum_k x[m,k] * w_gate[n,k]  +  bias_gate[n]
//                        u = (row_scale[m] * alpha_up[n])   * sum_k x[m,k] * w_up[n,k]    +  bias_up[n]
//
// xq / wq are the e4m3 codes and row_scale / alpha the fp32 scales of inc_fp8_quant_rows (include/inc_mi355x.h has the specification,
// DESIGN section 8c).  Every sum is inc_fp8_gemv's (gemm_fp8.hip), by the same strip body: one workgroup per 16 output columns, the
// weights non-temporal from HBM straight into the instruction's registers (mx_frag of mx_strip.hpp), K split over the 8 waves -- wave
// w takes the K-tiles w, w + 8, ... and accumulates them in increasing K -- and wave 0 adds the 8 partials from LDS in wave order.
// The factor product is one fp32 multiply; the multiply by the sum and the bias add (0.f without a bias) are inc_fp8_gemv's expression
// and may contract to one fma as they do there.  No workspace, no counters: repeated calls are bit-identical.  The number of K-tiles
// a wave has in flight per round differs between the kernels; it changes no sum order.  The wave count and the tile-to-wave map are
// inc_fp8_gemv's and fixed: the identities below rest on them.
//   multi   a workgroup finds its member in a table passed by value (MxGemvMembers' scheme, gemm_mx_gemv.hip) and runs the strip body,
//           so y_i is inc_fp8_gemv's output on member i bit for bit.
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
#include <type_traits>

#include "mx_strip.hpp"
#include "tile256_frame.hpp"  // load_bias_quad, store_quad16: inc_fp8_gemv's epilogue pieces

namespace {

constexpr int GW = 8;      // waves of a workgroup = ways of the in-workgroup K split: inc_fp8_gemv's, fixed
constexpr int STRIP = 16;  // weight rows of a workgroup: the instruction's M
constexpr int E4M3 = INC_MX_FP8_E4M3;
constexpr int MAX_MEMBERS = 8;
// K-tiles of a wave whose loads are in flight together.  One weight strip: inc_fp8_gemv's 4 (64 fragment registers).  Gate + up: 24
// fragment registers per tile; 2 is the experts kernel's depth for two strips and one row block (moe_unroll, gemm_fp8_moe.hip) and
// keeps as many weight bytes in flight per wave as the single strip at 4.  3 and 4 compile to the same 88 VGPRs and measure within
// 3 % of it (profiles/fp8/fp8_gated_unroll_ab.log).  Resources of both kernels: DESIGN section 8c.
constexpr int UNROLL_MULTI = 4;
#ifndef INC_FP8_GATED_UNROLL
#define INC_FP8_GATED_UNROLL 2
#endif
constexpr int UNROLL_GATED = INC_FP8_GATED_UNROLL;

// sum_k x[m,k] * w_s[n,k] of NS weight strips against the same rows of x: inc_fp8_gemv's K loop.  wp[s] / xp: the lane's row at
// K-tile 0 (+ 16 g); acc[s] is this wave's partial over its K-tiles
template <int NS, int U>
__device__ __forceinline__ void strip_partials(const uint8_t* const (&wp)[NS], const uint8_t* xp, int xkeep, int wave, int nk,
                                               f32x4 (&acc)[NS]) {
  // C of the wave's K-tiles kt, kt + GW, ...: every load first, then the MFMAs in K order
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[NS][C], xf[C];
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * GW;
#pragma unroll
      for (int s = 0; s < NS; ++s) wf[s][u] = mx_frag<E4M3, true>(wp[s] + t * XK);
      xf[u] = mx_frag<E4M3, false>(xp + t * XK);
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
#pragma unroll
      for (int d = 0; d < 8; ++d) xf[u][d] &= xkeep;
#pragma unroll
      for (int s = 0; s < NS; ++s)
        acc[s] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[s][u], xf[u], acc[s], E4M3, E4M3, 0, 0, 0, 0);
    }
  };
  int kt = wave;
  for (; kt + (U - 1) * GW < nk; kt += U * GW) round(kt, std::integral_constant<int, U>{});
  if constexpr (U == 4) {
    const int left = kt < nk ? (nk - kt + GW - 1) / GW : 0;  // 0 .. 3 tiles of this wave remain
    if (left == 3) round(kt, std::integral_constant<int, 3>{});
    else if (left == 2) round(kt, std::integral_constant<int, 2>{});
    else if (left == 1) round(kt, std::integral_constant<int, 1>{});
  } else {
    for (; kt < nk; kt += GW) round(kt, std::integral_constant<int, 1>{});
  }
}

// the weight matrices of one launch; member i owns the strips first[i] .. first[i + 1] - 1 of the grid
struct Fp8GemvMembers {
  const uint8_t* wq[MAX_MEMBERS];
  const float* alpha[MAX_MEMBERS];
  const uint16_t* bias[MAX_MEMBERS];
  uint16_t* y[MAX_MEMBERS];
  int64_t N[MAX_MEMBERS];
  int first[MAX_MEMBERS + 1];
  int y_vec_ok[MAX_MEMBERS];
  int n;
};

template <bool IS_BF16>
__global__ __launch_bounds__(GW * 64) void fp8_gemv_multi_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ row_scale,
                                                                 const Fp8GemvMembers mem, int M, int64_t Kp) {
  __shared__ f32x4 part[GW][64];
  const int strip = blockIdx.x;
  int mi = 0;
  for (int i = 1; i < mem.n; ++i)
    if (strip >= mem.first[i]) mi = i;
  const int64_t N = mem.N[mi];
  const int64_t n0 = (int64_t)(strip - mem.first[mi]) * STRIP;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  int64_t wrow = n0 + r;
  if (wrow > N - 1) wrow = N - 1;
  const int xrow = r < M ? r : M - 1;
  const int xkeep = r < M ? -1 : 0;
  const uint8_t* const wp[1] = {mem.wq[mi] + wrow * Kp + 16 * g};
  const uint8_t* const xp = xq + (int64_t)xrow * Kp + 16 * g;

  f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
  strip_partials<1, UNROLL_MULTI>(wp, xp, xkeep, wave, (int)(Kp / XK), acc);

  part[wave][lane] = acc[0];
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
  const float* const alpha = mem.alpha[mi];
  const BiasQuad bq = load_bias_quad<IS_BF16>(mem.bias[mi], nb, N);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float al = nb + e < N ? alpha[nb + e] : 0.f;
    v[e] = (rs * al) * sum[e] + bq.b[e];
  }
  store_quad16<IS_BF16>(mem.y[mi], m, nb, N, mem.y_vec_ok[mi], v);
}

template <bool IS_BF16>
__global__ __launch_bounds__(GW * 64) void fp8_gemv_gated_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ row_scale,
                                                                 const uint8_t* __restrict__ wq_gate, const float* __restrict__ alpha_gate,
                                                                 const uint16_t* __restrict__ bias_gate, const uint8_t* __restrict__ wq_up,
                                                                 const float* __restrict__ alpha_up, const uint16_t* __restrict__ bias_up,
                                                                 uint16_t* __restrict__ h, int M, int64_t N, int64_t Kp, int h_vec_ok) {
  __shared__ f32x4 part[2][GW][64];  // gate's and up's partials: 16 KiB
  const int64_t n0 = (int64_t)blockIdx.x * STRIP;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  int64_t wrow = n0 + r;
  if (wrow > N - 1) wrow = N - 1;
  const int xrow = r < M ? r : M - 1;
  const int xkeep = r < M ? -1 : 0;
  const uint8_t* const wp[2] = {wq_gate + wrow * Kp + 16 * g, wq_up + wrow * Kp + 16 * g};
  const uint8_t* const xp = xq + (int64_t)xrow * Kp + 16 * g;

  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  strip_partials<2, UNROLL_GATED>(wp, xp, xkeep, wave, (int)(Kp / XK), acc);

  part[0][wave][lane] = acc[0];
  part[1][wave][lane] = acc[1];
  __syncthreads();
  if (wave != 0) return;
  f32x4 sg = part[0][0][lane], su = part[1][0][lane];
#pragma unroll
  for (int w = 1; w < GW; ++w) {
    sg += part[0][w][lane];
    su += part[1][w][lane];
  }

  // C/D map of the 16 x 16 MFMA: register e of lane l is D[4 (l >> 4) + e][l & 15] = h[m = l & 15][n0 + 4 g + e]
  const int m = r;
  if (m >= M) return;
  const int64_t nb = n0 + 4 * g;
  if (nb >= N) return;
  const float rs = row_scale[m];
  const BiasQuad bg = load_bias_quad<IS_BF16>(bias_gate, nb, N);
  const BiasQuad bu = load_bias_quad<IS_BF16>(bias_up, nb, N);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float ag = nb + e < N ? alpha_gate[nb + e] : 0.f;
    const float au = nb + e < N ? alpha_up[nb + e] : 0.f;
    const float gv = (rs * ag) * sg[e] + bg.b[e];
    const float uv = (rs * au) * su[e] + bu.b[e];
    v[e] = silu_mul_f32(gv, uv);
  }
  store_quad16<IS_BF16>(h, m, nb, N, h_vec_ok, v);
}

// inc_fp8_gemv's checks of what the members share, in its order; the per-member ones follow in the entry points
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

extern "C" int inc_fp8_gemv_multi(int n, const uint8_t* xq, const float* row_scale, const uint8_t* const* wq, const float* const* alpha,
                                  const void* const* bias, void* const* y, int ydtype, int64_t M, const int64_t* N, int64_t Kp,
                                  inc_stream_t stream) {
  INC_CHECK_ARG(wq && alpha && y && N);
  if (n < 2 || n > MAX_MEMBERS) return INC_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) INC_CHECK_ARG(wq[i] && alpha[i] && y[i] && N[i] > 0);
  const int rc = fp8_group_check_x(xq, row_scale, ydtype, M, Kp);
  if (rc != INC_OK) return rc;
  Fp8GemvMembers mem = {};
  int64_t strips = 0;
  for (int i = 0; i < n; ++i) {
    INC_CHECK_ARG(fp8_group_member_aligned(wq[i], alpha[i]));
    mem.wq[i] = wq[i];
    mem.alpha[i] = alpha[i];
    mem.bias[i] = bias ? static_cast<const uint16_t*>(bias[i]) : nullptr;
    mem.y[i] = static_cast<uint16_t*>(y[i]);
    mem.N[i] = N[i];
    mem.first[i] = (int)strips;
    mem.y_vec_ok[i] = (N[i] % 4 == 0) && ((reinterpret_cast<uintptr_t>(y[i]) & 7) == 0);
    strips += ceil_div64(N[i], STRIP);
    INC_CHECK_ARG(strips < ((int64_t)1 << 31));
  }
  mem.first[n] = (int)strips;
  mem.n = n;
  const unsigned grid = (unsigned)strips;
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
