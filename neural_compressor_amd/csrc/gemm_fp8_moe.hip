// gemm_fp8_moe.hip -- K17e: the routed FP8 GEMM of the fused MoE experts, inc_fp8_gemm's product per expert over the rows inc_moe_route
// sorted, on v_mfma_f32_16x16x128_f8f6f4.
//
// Replaces the two F.linear of transformers' MixtralExperts.forward (also the Qwen2-MoE / Qwen3-MoE / OLMoE experts) for per-token /
// per-channel e4m3 weights.  One forward of FP8Experts is six launches and no host synchronisation:
//
//   inc_moe_route -> inc_fp8_quant_rows(x) -> inc_fp8_moe_gemm(0) -> inc_fp8_quant_rows(h) -> inc_fp8_moe_gemm(1) -> inc_moe_combine
//
//   f(r, n) = a_scale[r] * alpha[e, n]                                                                       (one fp32 multiply)
//   mode 0 (gate_up): h[p, j] = rd( silu(g) * u ),  g = f(tok(p), j) * acc[p, j],  u = f(tok(p), I + j) * acc[p, I + j]  (bf16 / fp16)
//   mode 1 (down):    y[p, n] = w[slot(p)] * (f(p, n) * acc[p, n])                                                       (fp32)
//   mode 2 (plain):   y[p, n] = f(tok(p), n) * acc[p, n]                                                                 (fp32)
//
// p is a position of the sorted slot order, e the expert whose range holds p, tok(p) = order[p] / top_k, slot(p) = order[p]; acc is the
// instruction's fp32 accumulator over the row's K-tiles.  Slice e of wq / alpha is what inc_fp8_quant_rows writes for expert e's [N, K]
// matrix.
//
// This is gemm_mx_moe.hip's kernel for the (fp8, fp8) pair with the block-scale path taken out, as gemm_fp8.hip relates to
// gemm_mx*.hip: no scale-byte pointers, loads or registers, the builtin with literal zero scale operands (the compiler emits the
// UNSCALED opcode; it equals the scaled one with both scale bytes 127 bit for bit, tools/mx_lab.hip), and the two
// fp32 factors in the epilogue.  Everything else is that kernel's contract: workgroup = (strip of 16 output columns, 64-row tile of
// the route's table), the grid sized from S and E alone, slots past route[0] exit at once; the strip's 16 weight rows are the A
// operand (mx_strip.hpp), a block of 16 sorted positions a B operand, and only the ceil(rows / 16) blocks a tile has are loaded and
// multiplied.  Weights non-temporal, activations plain, gathered through order[] in modes 0 / 2.  Lanes past the end of the expert's
// range re-read the tile's first row and lanes of a weight row past the strip's end re-read its last row; what they produce is never
// stored, and a_scale is read in the epilogue by the lanes that store only.  In mode 0 a wave carries the gate strip and the up strip
// of the same j, so the SiLU product is lane-local.
// K is split INSIDE the workgroup: wave w of 8 takes the K-tiles w, w + 8, ... ascending; the partials meet in LDS (one strip at a
// time: 32 KiB), wave b adds the 8 partials of row block b in wave order and stores it.  No global hand-off, no workspace, no counters:
// repeated calls are bit-identical, and one expert's rows carry inc_fp8_gemv's sums (W = 8 is that kernel's split, hence fixed).
// Algorithmic bytes per launch: the weights and alpha of the experts that were hit once per 64-row tile, the activation rows once.
#include <type_traits>

#include "moe_common.hpp"
#include "mx_strip.hpp"

namespace {

constexpr int MW = 8;            // waves of a workgroup = ways of the in-workgroup K split: inc_fp8_gemv's, fixed
constexpr int STRIP = 16;        // weight rows of a workgroup: the instruction's M
constexpr int RB = MOE_BM / 16;  // row blocks of a tile
constexpr int E4M3 = INC_MX_FP8_E4M3;
static_assert(MW >= RB, "at least one wave per row block");

struct Fp8MoeArgs {
  const uint8_t* aq;
  const float* as;
  const int* route;
  const uint8_t* wq;
  const float* alpha;
  const void* rw;
  void* out;
  int64_t N, Kp;
  int wdt, out_bf16, inplace, vec_ok, S, top_k, E, strips;
};

// K-tiles of a wave whose loads are in flight together: inc_mx_moe_gemm's depths (up to 64 fragment registers per round).  Without
// the scale registers deeper rounds fit (6 / 4 / 3 / 2: 124 and 88 VGPRs, no scratch) but do not pay: measured on the MI355X they are
// 0.96 - 1.27 x the time of these depths, slower on 12 of 16 points ("FP8 experts")
__host__ __device__ constexpr int moe_unroll(int ns, int nb) { return ns + nb <= 2 ? 4 : ns + nb <= 4 ? 2 : 1; }

// one (strip, tile) with NB row blocks; part: the workgroup's LDS
template <bool GATED, int NB>
__device__ __forceinline__ void fp8_moe_body(const Fp8MoeArgs& a, f32x4 (*part)[RB][64], int e, int p0, int rows, int strip) {
  constexpr int NS = GATED ? 2 : 1;  // weight strips: gate and up rows of the same j
  constexpr int U = moe_unroll(NS, NB);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t Nout = GATED ? a.N / 2 : a.N;
  const int64_t n0 = (int64_t)strip * STRIP;
  const int nk = (int)(a.Kp / XK);
  const int* const order = a.route + moe_route_layout(a.S, a.E).order;

  int64_t wrow = n0 + r;
  if (wrow > Nout - 1) wrow = Nout - 1;
  const uint8_t* wp[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) wp[s] = a.wq + ((int64_t)e * a.N + s * Nout + wrow) * a.Kp + 16 * g;
  const uint8_t* ap[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int rr = 16 * b + r;
    const int p = rr < rows ? p0 + rr : p0;  // past the range: the tile's first row again; that column of D is never stored
    const int64_t src = a.inplace ? p : order[p] / a.top_k;
    ap[b] = a.aq + src * a.Kp + 16 * g;
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
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * MW;
#pragma unroll
      for (int s = 0; s < NS; ++s) wf[s][u] = mx_frag<E4M3, true>(wp[s] + t * XK);
#pragma unroll
      for (int b = 0; b < NB; ++b) xf[b][u] = mx_frag<E4M3, false>(ap[b] + t * XK);
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int s = 0; s < NS; ++s)
          acc[s][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[s][u], xf[b][u], acc[s][b], E4M3, E4M3, 0, 0, 0, 0);
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
  // the two factors: the row's (a valid position's source row, the only rows whose a_scale is read) and the columns'
  const int slot = order[p];
  const float rs = a.as[a.inplace ? p : (int64_t)(slot / a.top_k)];
  float v[4];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float* al = a.alpha + (int64_t)e * a.N + s * Nout + nb;
#pragma unroll
    for (int i = 0; i < 4; ++i) res[s][i] = (rs * (nb + i < Nout ? al[i] : 0.f)) * res[s][i];
  }
  if constexpr (GATED) {
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
    const float wt = a.inplace ? moe_load_weight(a.rw, slot, a.wdt) : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = a.inplace ? wt * res[0][i] : res[0][i];
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

template <bool GATED>
__global__ __launch_bounds__(MW * 64, 4) void fp8_moe_gemm_kernel(const Fp8MoeArgs a) {
  __shared__ f32x4 part[MW][RB][64];
  const int tile = (int)(blockIdx.x / (unsigned)a.strips), strip = (int)(blockIdx.x - (unsigned)tile * (unsigned)a.strips);
  if (tile >= a.route[0]) return;  // more tile slots than tiles
  const RouteLayout L = moe_route_layout(a.S, a.E);
  const int e = a.route[L.tiles + 2 * tile], p0 = a.route[L.tiles + 2 * tile + 1];
  const int pe = a.route[L.offsets + e + 1];
  const int rows = pe - p0 < MOE_BM ? pe - p0 : MOE_BM;
  const int blocks = __builtin_amdgcn_readfirstlane((rows + 15) >> 4);  // row blocks of this tile: the same for the whole workgroup
  if (blocks == 1) fp8_moe_body<GATED, 1>(a, part, e, p0, rows, strip);
  else if (blocks == 2) fp8_moe_body<GATED, 2>(a, part, e, p0, rows, strip);
  else if (blocks == 3) fp8_moe_body<GATED, 3>(a, part, e, p0, rows, strip);
  else fp8_moe_body<GATED, 4>(a, part, e, p0, rows, strip);
}

}  // namespace

extern "C" int inc_fp8_moe_gemm(int mode, const uint8_t* aq, const float* a_scale, const int32_t* route, const uint8_t* wq,
                                const float* alpha, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T,
                                int top_k, int64_t E, int64_t N, int64_t Kp, inc_stream_t stream) {
  INC_CHECK_ARG(mode >= 0 && mode <= 2);
  INC_CHECK_ARG(aq && a_scale && route && wq && alpha && out && T > 0 && top_k > 0 && E > 0 && N > 0 && Kp > 0);
  INC_CHECK_ARG(mode != 1 || routing_weights);
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  if (E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  if (mode == 0 && (N % 2) != 0) return INC_ERR_UNSUPPORTED;
  if (mode == 0 ? (odtype != INC_BF16 && odtype != INC_F16) : odtype != INC_F32) return INC_ERR_UNSUPPORTED;
  if (mode == 1 && wdtype != INC_F32 && wdtype != INC_F16 && wdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(aq) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(a_scale) | reinterpret_cast<uintptr_t>(alpha)) & 3) == 0);
  const int64_t S = T * top_k, Nout = mode == 0 ? N / 2 : N;
  const int64_t strips = ceil_div64(Nout, STRIP), units = strips * moe_tiles_max(S, E);
  if (units >= ((int64_t)1 << 31)) return INC_ERR_UNSUPPORTED;
  Fp8MoeArgs a = {};
  a.aq = aq; a.as = a_scale; a.route = route; a.wq = wq; a.alpha = alpha; a.rw = routing_weights; a.out = out;
  a.N = N; a.Kp = Kp;
  a.wdt = wdtype; a.out_bf16 = odtype == INC_BF16; a.inplace = mode == 1;
  a.vec_ok = (Nout % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & (mode == 0 ? 7 : 15)) == 0;
  a.S = (int)S; a.top_k = top_k; a.E = (int)E; a.strips = (int)strips;
  const unsigned grid = (unsigned)units;
  if (mode == 0)
    fp8_moe_gemm_kernel<true><<<grid, MW * 64, 0, inc_s(stream)>>>(a);
  else
    fp8_moe_gemm_kernel<false><<<grid, MW * 64, 0, inc_s(stream)>>>(a);
  INC_LAUNCH_RETURN();
}
