// gemm_mx_moe.hip -- K16e: the routed MX GEMM of the fused MoE experts, inc_mx_gemm's product per expert over the rows inc_moe_route
// sorted, on v_mfma_scale_f32_16x16x128_f8f6f4.
//
// Replaces the two F.linear of transformers' MixtralExperts.forward (also the Qwen2-MoE / Qwen3-MoE / OLMoE experts) for MX weights.
// One forward of MXExperts is six launches and no host synchronisation:
//
//   inc_moe_route -> inc_mx_quant(x) -> inc_mx_moe_gemm(0) -> inc_mx_quant(h) -> inc_mx_moe_gemm(1) -> inc_moe_combine
//
//   mode 0 (gate_up): h[p, j] = rd( silu(g) * u ),  g = x[tok(p)] . Wg[e, j],  u = x[tok(p)] . Wu[e, j],  j < I    (bf16 / fp16)
//   mode 1 (down):    y[p, n] = w[slot(p)] * (h[p] . Wd[e, n])                                                  (fp32)
//   mode 2 (plain):   y[p, n] = x[tok(p)] . W[e, n]                                                              (fp32)
//
// p is a position of the sorted slot order, e the expert whose range holds p, tok(p) = order[p] / top_k, slot(p) = order[p].  Operands,
// storage and arithmetic are inc_mx_gemm's; slice e of wq / ws is what inc_mx_quant writes for expert e's [N, K] matrix.
//
// Workgroup = (strip of 16 output columns, 64-row tile of the route's table); the grid is sized from S and E alone and slots past
// route[0] exit at once.  The strip's 16 weight rows are the A operand (the decode GEMV's strip body, mx_strip.hpp), a block of 16
// sorted positions is a B operand, and only the ceil(rows / 16) blocks a tile has are loaded and multiplied (chosen per workgroup:
// a decode tile is one MFMA per K-tile).  A lane takes its row's fragment and scale byte straight from global memory: non-temporal
// for the weights, plain for the activations (every strip re-reads them from L2), gathered through order[] in modes 0 / 2.  Lanes past
// the end of the expert's range re-read the tile's first row and lanes of a weight row past the strip's end re-read its last row: a
// lane's row feeds one row or column of D only, and those are never stored.  In mode 0 a wave carries the gate strip and the up strip of the same j: by the C/D map
// a lane holds the same four (p, j) of both, so the SiLU product is lane-local.
// K is split INSIDE the workgroup as in the GEMV: wave w of W takes the K-tiles w, w + W, ...; the partials meet in LDS (one strip at a
// time: 32 KiB), wave b adds the W partials of row block b in wave order and stores it.  No global hand-off, no workspace, no
// counters: repeated calls are bit-identical, and with W = INC_MX_GEMV_WAVES one expert's rows are inc_mx_gemv's sums.
// Algorithmic bytes per launch: the weights and scales of the experts that were hit once per 64-row tile, the activation rows once.
#include <type_traits>

#include "moe_common.hpp"
#include "mx_strip.hpp"

#ifndef INC_MX_MOE_WAVES
#define INC_MX_MOE_WAVES 8  // W: 4, 8 or 16
#endif

namespace {

constexpr int MW = INC_MX_MOE_WAVES;  // waves of a workgroup = ways of the in-workgroup K split
constexpr int STRIP = 16;             // weight rows of a workgroup: the instruction's M
constexpr int RB = MOE_BM / 16;       // row blocks of a tile
static_assert(MW == 4 || MW == 8 || MW == 16, "W is 4, 8 or 16 (at least one wave per row block)");

struct MxMoeArgs {
  const uint8_t* aq;
  const uint8_t* as;
  const int* route;
  const uint8_t* wq;
  const uint8_t* ws;
  const void* rw;
  void* out;
  int64_t N, Kp;
  int wdt, out_bf16, inplace, vec_ok, S, top_k, E, strips;
};

// K-tiles of a wave whose loads are in flight together: up to 64 fragment registers per round, so that every instantiation stays
// inside 128 VGPRs (two workgroups per CU) without scratch
__host__ __device__ constexpr int moe_unroll(int ns, int nb) { return ns + nb <= 2 ? 4 : ns + nb <= 4 ? 2 : 1; }

// one (strip, tile) with NB row blocks; part: the workgroup's LDS
template <int AF, int WF, bool GATED, int NB>
__device__ __forceinline__ void mx_moe_body(const MxMoeArgs& a, f32x4 (*part)[RB][64], int e, int p0, int rows, int strip) {
  constexpr int NS = GATED ? 2 : 1;  // weight strips: gate and up rows of the same j
  constexpr int TA = mx_tile_bytes(AF), TW = mx_tile_bytes(WF);
  constexpr int U = moe_unroll(NS, NB);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t Nout = GATED ? a.N / 2 : a.N;
  const int64_t n0 = (int64_t)strip * STRIP;
  const int64_t sld = a.Kp / 32;  // scale bytes per row
  const int nk = (int)(a.Kp / XK);
  const int* const order = a.route + moe_route_layout(a.S, a.E).order;

  int64_t wrow = n0 + r;
  if (wrow > Nout - 1) wrow = Nout - 1;
  const uint8_t* wp[NS];
  const uint8_t* wsp[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int64_t row = (int64_t)e * a.N + s * Nout + wrow;
    wp[s] = a.wq + row * ((int64_t)nk * TW) + 16 * g;
    wsp[s] = a.ws + row * sld + g;
  }
  const uint8_t* ap[NB];
  const uint8_t* asp[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int rr = 16 * b + r;
    const int p = rr < rows ? p0 + rr : p0;  // past the range: the tile's first row again; that column of D is never stored
    const int64_t src = a.inplace ? p : order[p] / a.top_k;
    ap[b] = a.aq + src * ((int64_t)nk * TA) + 16 * g;
    asp[b] = a.as + src * sld + g;
  }

  f32x4 acc[NS][NB];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[s][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // C of the wave's K-tiles kt, kt + MW, ...: every load first, then the MFMAs in K order
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[NS][C], xf[NB][C];
    int sw[NS][C], sx[NB][C];
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * MW;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        wf[s][u] = mx_frag<WF, true>(wp[s] + t * TW);
        sw[s][u] = wsp[s][t * 4];
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        xf[b][u] = mx_frag<AF, false>(ap[b] + t * TA);
        sx[b][u] = asp[b][t * 4];
      }
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int s = 0; s < NS; ++s)
          acc[s][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[s][u], xf[b][u], acc[s][b], WF, AF, 0, sw[s][u], 0, sx[b][u]);
    }
  };
  int kt = wave;
  for (; kt + (U - 1) * MW < nk; kt += U * MW) round(kt, std::integral_constant<int, U>{});
  for (; kt < nk; kt += MW) round(kt, std::integral_constant<int, 1>{});

  // wave b sums row block b over the waves, in wave order; one strip at a time through the same LDS
  f32x4 res[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s) __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) part[wave][b][lane] = acc[s][b];
    __syncthreads();
    if (wave < NB) {
      f32x4 sum = part[0][wave][lane];
#pragma unroll
      for (int w = 1; w < MW; ++w) sum += part[w][wave][lane];
      res[s] = sum;
    }
  }
  if (wave >= NB) return;

  // C/D map of the 16 x 16 MFMA: register i of lane l is D[4 (l >> 4) + i][l & 15] = position 16 wave + r, column n0 + 4 g + i
  const int rr = 16 * wave + r;
  if (rr >= rows) return;
  const int64_t p = p0 + rr;
  const int64_t nb = n0 + 4 * g;
  if (nb >= Nout) return;
  const bool vec = a.vec_ok && nb + 4 <= Nout;
  if constexpr (GATED) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = silu_mul_f32(res[0][i], res[1][i]);
    uint16_t* dst = static_cast<uint16_t*>(a.out) + p * Nout + nb;
    if (vec) {
      *reinterpret_cast<uint2*>(dst) = a.out_bf16 ? make_uint2(cvt_pair<true>(v[0], v[1]), cvt_pair<true>(v[2], v[3]))
                                                  : make_uint2(cvt_pair<false>(v[0], v[1]), cvt_pair<false>(v[2], v[3]));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (nb + i < Nout) dst[i] = a.out_bf16 ? f32_to_bf16_bits(v[i]) : f32_to_f16_bits(v[i]);
    }
  } else {
    f32x4 v = res[0];
    if (a.inplace) {
      const float wt = moe_load_weight(a.rw, order[p], a.wdt);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = res[0][i] * wt;
    }
    float* dst = static_cast<float*>(a.out) + p * Nout + nb;
    if (vec) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (nb + i < Nout) dst[i] = v[i];
    }
  }
}

template <int AF, int WF, bool GATED>
__global__ __launch_bounds__(MW * 64, 4) void mx_moe_gemm_kernel(const MxMoeArgs a) {
  __shared__ f32x4 part[MW][RB][64];
  const int tile = (int)(blockIdx.x / (unsigned)a.strips), strip = (int)(blockIdx.x - (unsigned)tile * (unsigned)a.strips);
  if (tile >= a.route[0]) return;  // more tile slots than tiles
  const RouteLayout L = moe_route_layout(a.S, a.E);
  const int e = a.route[L.tiles + 2 * tile], p0 = a.route[L.tiles + 2 * tile + 1];
  const int pe = a.route[L.offsets + e + 1];
  const int rows = pe - p0 < MOE_BM ? pe - p0 : MOE_BM;
  const int blocks = __builtin_amdgcn_readfirstlane((rows + 15) >> 4);  // row blocks of this tile: the same for the whole workgroup
  if (blocks == 1) mx_moe_body<AF, WF, GATED, 1>(a, part, e, p0, rows, strip);
  else if (blocks == 2) mx_moe_body<AF, WF, GATED, 2>(a, part, e, p0, rows, strip);
  else if (blocks == 3) mx_moe_body<AF, WF, GATED, 3>(a, part, e, p0, rows, strip);
  else mx_moe_body<AF, WF, GATED, 4>(a, part, e, p0, rows, strip);
}

template <int AF, int WF>
int moe_launch(bool gated, unsigned grid, const MxMoeArgs& a, inc_stream_t stream) {
  if (gated)
    mx_moe_gemm_kernel<AF, WF, true><<<grid, MW * 64, 0, inc_s(stream)>>>(a);
  else
    mx_moe_gemm_kernel<AF, WF, false><<<grid, MW * 64, 0, inc_s(stream)>>>(a);
  INC_LAUNCH_RETURN();
}

}  // namespace

extern "C" int inc_mx_moe_gemm(int mode, const uint8_t* aq, const uint8_t* as, int afmt, const int32_t* route, const uint8_t* wq,
                               const uint8_t* ws, int wfmt, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T,
                               int top_k, int64_t E, int64_t N, int64_t Kp, inc_stream_t stream) {
  INC_CHECK_ARG(mode >= 0 && mode <= 2);
  INC_CHECK_ARG(aq && as && route && wq && ws && out && T > 0 && top_k > 0 && E > 0 && N > 0 && Kp > 0);
  INC_CHECK_ARG(mode != 1 || routing_weights);
  const bool p88 = afmt == INC_MX_FP8_E4M3 && wfmt == INC_MX_FP8_E4M3;
  const bool p84 = afmt == INC_MX_FP8_E4M3 && wfmt == INC_MX_FP4_E2M1;
  const bool p44 = afmt == INC_MX_FP4_E2M1 && wfmt == INC_MX_FP4_E2M1;
  if (!p88 && !p84 && !p44) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  if (E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  if (mode == 0 && (N % 2) != 0) return INC_ERR_UNSUPPORTED;
  if (mode == 0 ? (odtype != INC_BF16 && odtype != INC_F16) : odtype != INC_F32) return INC_ERR_UNSUPPORTED;
  if (mode == 1 && wdtype != INC_F32 && wdtype != INC_F16 && wdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(aq) & 15) == 0 && (reinterpret_cast<uintptr_t>(wq) & 15) == 0);
  const int64_t S = T * top_k, Nout = mode == 0 ? N / 2 : N;
  const int64_t strips = ceil_div64(Nout, STRIP), units = strips * moe_tiles_max(S, E);
  if (units >= ((int64_t)1 << 31)) return INC_ERR_UNSUPPORTED;
  MxMoeArgs a = {};
  a.aq = aq; a.as = as; a.route = route; a.wq = wq; a.ws = ws; a.rw = routing_weights; a.out = out;
  a.N = N; a.Kp = Kp;
  a.wdt = wdtype; a.out_bf16 = odtype == INC_BF16; a.inplace = mode == 1;
  a.vec_ok = (Nout % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & (mode == 0 ? 7 : 15)) == 0;
  a.S = (int)S; a.top_k = top_k; a.E = (int)E; a.strips = (int)strips;
  const unsigned grid = (unsigned)units;
  if (p88) return moe_launch<INC_MX_FP8_E4M3, INC_MX_FP8_E4M3>(mode == 0, grid, a, stream);
  if (p84) return moe_launch<INC_MX_FP8_E4M3, INC_MX_FP4_E2M1>(mode == 0, grid, a, stream);
  return moe_launch<INC_MX_FP4_E2M1, INC_MX_FP4_E2M1>(mode == 0, grid, a, stream);
}
