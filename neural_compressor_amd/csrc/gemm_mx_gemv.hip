// gemm_mx_gemv.hip -- K16b: the decode route of the MX cell, inc_mx_gemm's product for 1 <= M <= 16 rows of x, on
// v_mfma_scale_f32_16x16x128_f8f6f4.
//
//   y[m, n] = sum_blocks 2^(xs[m,b] + ws[n,b] - 254) * sum_{k in block b} x[m,k] * w[n,k]  +  bias[n]
//
// Operands, storage and arithmetic are inc_mx_gemm's (include/inc_mi355x.h has the specification).  This is the strip scheme of
// strip_frame.hpp with block scales (SCALED = true), one weight strip and one block of x rows: a workgroup owns one strip of 16 weight
// rows over all of K; a lane loads what the instruction wants of its row straight from global memory into VGPRs -- two (fp8) or one
// (fp4) 16-byte loads and one scale byte per operand and K-tile, non-temporal for the weights (streamed once), plain for x (every
// strip re-reads it from L2) -- with no LDS round trip and no shuffle.  K is split over the W waves of the workgroup, UNROLL tiles per
// round and the cascade tail; wave 0 adds the W partials in wave order, adds the bias in fp32 and rounds once.  No global hand-off, no
// counters, no workspace: repeated calls are bit-identical.
// Lanes of an x row >= M supply zero codes, lanes of a weight row >= N re-read row N - 1; what they produce is never stored.
// inc_mx_gemv_multi is the same kernel over the strips of up to 8 weight matrices one after another: a workgroup finds its member in
// a table passed by value (StripMembers) and then runs the same strip, so member i's output is inc_mx_gemv's bit for bit; inc_mx_gemv
// is the launch with a table of one member.
// Algorithmic bytes per launch: N * Kp * (1 or 1/2) + N * Kp / 32 + M * Kp * (1 or 1/2) + M * Kp / 32 + 2 * M * N.
#include "strip_frame.hpp"

#ifndef INC_MX_GEMV_WAVES
#define INC_MX_GEMV_WAVES 8  // W: 4, 8 or 16 (scripts/mx_gemv_time.py; the rejected values are in profiles/NOTES.md)
#endif

namespace {

constexpr int GW = INC_MX_GEMV_WAVES;  // waves of a workgroup = ways of the in-workgroup K split
constexpr int UNROLL = 4;              // K-tiles of a wave whose loads are in flight together
static_assert(GW == 4 || GW == 8 || GW == 16, "W is 4, 8 or 16");

using MxGemvMembers = StripMembers<uint8_t>;  // ws: the member's scale bytes

// The kernel is kept in written-out form around the frame's member table and mx_frag: its K loop is strip_partials<WF, XF, true, 1, 1,
// UNROLL, GW, true, true>, its sum strip_sum_wave0, in the parent's own text.  Through the frame's functions the compiler scheduled
// the same instructions differently (80 / 76 / 62 instead of 72 / 66 / 60 VGPRs) and the a8w8 / a8w4 launches measured 0.5 - 2.5 %
// slower (profiles/strip_frame/README.md).  Any change to the tile-to-wave map, the K order or the sum order here must be made in
// strip_frame.hpp too: the experts kernel's one-expert identity rests on their being equal.
template <bool IS_BF16, int XF, int WF>
__global__ __launch_bounds__(GW * 64) void mx_gemv_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                                          const MxGemvMembers mem, int M, int64_t Kp) {
  __shared__ f32x4 part[GW][64];
  const int strip = blockIdx.x;
  const int mi = strip_member(mem, strip);
  const int64_t N = mem.N[mi];
  const int64_t n0 = (int64_t)(strip - mem.first[mi]) * STRIP;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  constexpr int TX = mx_tile_bytes(XF), TW = mx_tile_bytes(WF);
  const int64_t sld = Kp / 32;  // scale bytes per row
  int64_t wrow = n0 + r;
  if (wrow > N - 1) wrow = N - 1;
  const int xrow = r < M ? r : M - 1;
  const int xkeep = r < M ? -1 : 0;
  const uint8_t* const wp = mem.wq[mi] + wrow * (Kp / XK * TW) + 16 * g;
  const uint8_t* const xp = xq + (int64_t)xrow * (Kp / XK * TX) + 16 * g;
  const uint8_t* const wsp = mem.ws[mi] + wrow * sld + g;
  const uint8_t* const xsp = xs + (int64_t)xrow * sld + g;
  const int nk = (int)(Kp / XK);

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // C rounds of the wave's K-tiles kt, kt + GW, ...: every load first, then the MFMAs in K order
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[C], xf[C];
    int sw[C], sx[C];
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * GW;
      wf[u] = mx_frag<WF, true>(wp + t * TW);
      sw[u] = wsp[t * 4];
      xf[u] = mx_frag<XF, false>(xp + t * TX);
      sx[u] = xsp[t * 4];
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
#pragma unroll
      for (int d = 0; d < 8; ++d) xf[u][d] &= xkeep;
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[u], xf[u], acc, WF, XF, 0, sw[u], 0, sx[u]);
    }
  };
  int kt = wave;
  for (; kt + (UNROLL - 1) * GW < nk; kt += UNROLL * GW) round(kt, std::integral_constant<int, UNROLL>{});
  const int left = kt < nk ? (nk - kt + GW - 1) / GW : 0;  // 0 .. UNROLL - 1 tiles of this wave remain
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
  const uint16_t* const bias = mem.bias[mi];
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float b = 0.f;
    if (bias && nb + e < N) b = IS_BF16 ? bf16_bits_to_f32(bias[nb + e]) : f16_bits_to_f32(bias[nb + e]);
    v[e] = sum[e] + b;
  }
  uint16_t* dst = mem.y[mi] + (int64_t)m * N + nb;
  if (mem.y_vec_ok[mi] && nb + 4 <= N) {
    *reinterpret_cast<uint2*>(dst) = make_uint2(cvt_pair<IS_BF16>(v[0], v[1]), cvt_pair<IS_BF16>(v[2], v[3]));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (nb + e < N) dst[e] = IS_BF16 ? f32_to_bf16_bits(v[e]) : f32_to_f16_bits(v[e]);
  }
}

template <int XF, int WF>
int gemv_launch(const uint8_t* xq, const uint8_t* xs, const MxGemvMembers& mem, int ydtype, int64_t M, int64_t Kp, inc_stream_t stream) {
  const unsigned grid = (unsigned)mem.first[mem.n];
  if (ydtype == INC_BF16)
    mx_gemv_kernel<true, XF, WF><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, xs, mem, (int)M, Kp);
  else
    mx_gemv_kernel<false, XF, WF><<<grid, GW * 64, 0, inc_s(stream)>>>(xq, xs, mem, (int)M, Kp);
  INC_LAUNCH_RETURN();
}

// the checks both entry points share, in inc_mx_gemm's order; fills the table
int gemv_run(int n, const uint8_t* xq, const uint8_t* xs, int xfmt, const uint8_t* const* wq, const uint8_t* const* ws, int wfmt,
             const void* const* bias, void* const* y, int ydtype, int64_t M, const int64_t* N, int64_t Kp, inc_stream_t stream) {
  INC_CHECK_ARG(xq && xs && M > 0 && Kp > 0);
  for (int i = 0; i < n; ++i) INC_CHECK_ARG(wq[i] && ws[i] && y[i] && N[i] > 0);
  if (M > INC_MX_GEMV_MAX_M) return INC_ERR_UNSUPPORTED;
  if (ydtype != INC_BF16 && ydtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  const bool p88 = xfmt == INC_MX_FP8_E4M3 && wfmt == INC_MX_FP8_E4M3;
  const bool p84 = xfmt == INC_MX_FP8_E4M3 && wfmt == INC_MX_FP4_E2M1;
  const bool p44 = xfmt == INC_MX_FP4_E2M1 && wfmt == INC_MX_FP4_E2M1;
  if (!p88 && !p84 && !p44) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(xq) & 15) == 0 && (reinterpret_cast<uintptr_t>(xs) & 3) == 0);
  MxGemvMembers mem = {};
  const int rc = strip_members_fill(mem, n, wq, ws, bias, y, N);
  if (rc != INC_OK) return rc;
  if (p88) return gemv_launch<INC_MX_FP8_E4M3, INC_MX_FP8_E4M3>(xq, xs, mem, ydtype, M, Kp, stream);
  if (p84) return gemv_launch<INC_MX_FP8_E4M3, INC_MX_FP4_E2M1>(xq, xs, mem, ydtype, M, Kp, stream);
  return gemv_launch<INC_MX_FP4_E2M1, INC_MX_FP4_E2M1>(xq, xs, mem, ydtype, M, Kp, stream);
}

}  // namespace

extern "C" int inc_mx_gemv(const uint8_t* xq, const uint8_t* xs, int xfmt, const uint8_t* wq, const uint8_t* ws, int wfmt,
                           const void* bias, void* y, int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  return gemv_run(1, xq, xs, xfmt, &wq, &ws, wfmt, &bias, &y, ydtype, M, &N, Kp, stream);
}

extern "C" int inc_mx_gemv_multi(int n, const uint8_t* xq, const uint8_t* xs, int xfmt, const uint8_t* const* wq,
                                 const uint8_t* const* ws, int wfmt, const void* const* bias, void* const* y, int ydtype, int64_t M,
                                 const int64_t* N, int64_t Kp, inc_stream_t stream) {
  INC_CHECK_ARG(wq && ws && y && N);
  if (n < 2 || n > STRIP_MAX_MEMBERS) return INC_ERR_UNSUPPORTED;
  return gemv_run(n, xq, xs, xfmt, wq, ws, wfmt, bias, y, ydtype, M, N, Kp, stream);
}
