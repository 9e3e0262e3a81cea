// gemm_strip_moe.hip -- K16e / K17e: the routed GEMM of the fused MoE experts for the MX cell (inc_mx_moe_gemm, inc_mx_gemm's product)
// and the per-token / per-channel FP8 cell (inc_fp8_moe_gemm, inc_fp8_gemm's product), per expert over the rows inc_moe_route sorted,
// on v_mfma_(scale_)f32_16x16x128_f8f6f4.  One kernel template; a cell type says what differs.
//
// Replaces the two F.linear of transformers' MixtralExperts.forward (also the Qwen2-MoE / Qwen3-MoE / OLMoE experts).  One forward of
// MXExperts / FP8Experts is six launches and no host synchronisation, quant = inc_mx_quant / inc_fp8_quant_rows:
//
//   inc_moe_route -> quant(x) -> inc_*_moe_gemm(0) -> quant(h) -> inc_*_moe_gemm(1) -> inc_moe_combine
//
//   mode 0 (gate_up): h[p, j] = rd( silu(g) * u ),  g = f(tok(p), j) * acc[p, j],  u = f(tok(p), I + j) * acc[p, I + j]   (bf16 / fp16)
//   mode 1 (down):    y[p, n] = w[slot(p)] * (f(p, n) * acc[p, n])                                                        (fp32)
//   mode 2 (plain):   y[p, n] = f(tok(p), n) * acc[p, n]                                                                  (fp32)
//
// p is a position of the sorted slot order, e the expert whose range holds p, tok(p) = order[p] / top_k, slot(p) = order[p]; acc is the
// instruction's fp32 accumulator over the row's K-tiles.  Slice e of wq / ws is what the cell's quantiser writes for expert e's
// [N, K] matrix.
//
// Workgroup = (strip of 16 output columns, 64-row tile of the route's table); the grid is sized from S and E alone and slots past
// route[0] exit at once.  The strip's 16 weight rows are the A operand (strip_frame.hpp), a block of 16 sorted positions is a B
// operand, and only the ceil(rows / 16) blocks a tile has are loaded and multiplied (chosen per workgroup: a decode tile is one MFMA
// per K-tile).  Weights non-temporal, activations plain (every strip re-reads them from L2), gathered through order[] in modes 0 / 2.
// Lanes past the end of the expert's range re-read the tile's first row and lanes of a weight row past the strip's end re-read its
// last row: a lane's row feeds one row or column of D only, and those are never stored.  In mode 0 a wave carries the gate strip and
// the up strip of the same j: by the C/D map a lane holds the same four (p, j) of both, so the SiLU product is lane-local.
// K is split INSIDE the workgroup as in the GEMVs: wave w of W takes the K-tiles w, w + W, ... ascending; the partials meet in LDS (one
// strip at a time: 32 KiB), wave b adds the W partials of row block b in wave order and stores it.  No global hand-off, no workspace,
// no counters: repeated calls are bit-identical, and one expert's rows carry the cell's decode GEMV sums.
// The cells:
//   MxCell    acc carries the block scales (as / ws are E8M0 scale bytes, [rows, Kp / 32]; the scaled opcode) and f = 1: no factor
//             multiply.  Three format pairs.  W = INC_MX_MOE_WAVES (with W = INC_MX_GEMV_WAVES the sums are inc_mx_gemv's).
//   Fp8Cell   no scale bytes: no scale pointers, loads or registers, the unscaled opcode (the MX accumulator at scale bytes 127 bit for
//             bit); as = a_scale[rows] and ws = alpha[E, N] are fp32 and f(r, n) = a_scale[r] * alpha[e, n] is one
//             fp32 multiply in the epilogue; a_scale is read by the lanes that store only.  (fp8, fp8) alone; W = 8 is inc_fp8_gemv's
//             split, hence fixed.
// The epilogues (an Args type says which): PlainEpi is the above; GluEpi (inc_mx_moe_gemm_glu, the experts of GPT-OSS) adds a per-expert
// fp32 bias b(e, n) to acc in every mode -- read after the LDS sum by the lanes that store, for the columns they store -- and replaces
// the SiLU product of mode 0 by the clamped SwiGLU glu_clamped_f32(g, u, alpha, limit) of common.hpp; the K loop is the same code.
// Algorithmic bytes per launch: the weights and scales of the experts that were hit once per 64-row tile, the activation rows once.
#include "moe_common.hpp"
#include "strip_frame.hpp"
#include <type_traits>

#ifndef INC_MX_MOE_WAVES
#define INC_MX_MOE_WAVES 8  // W: 4, 8 or 16
#endif

namespace {

constexpr int RB = MOE_BM / 16;  // row blocks of a tile

// Scale: the type behind as / ws; MW: waves of a workgroup = ways of the in-workgroup K split; SCALE_ALIGN: what as / ws must be aligned to
struct MxCell {
  using Scale = uint8_t;
  static constexpr bool SCALED = true;
  static constexpr int MW = INC_MX_MOE_WAVES;
  static constexpr uintptr_t SCALE_ALIGN = 1;
};
struct Fp8Cell {
  using Scale = float;
  static constexpr bool SCALED = false;
  static constexpr int MW = 8;
  static constexpr uintptr_t SCALE_ALIGN = 4;
};
static_assert(MxCell::MW == 4 || MxCell::MW == 8 || MxCell::MW == 16, "W is 4, 8 or 16 (at least one wave per row block)");

template <class Scale>
struct StripMoeArgs {
  const uint8_t* aq;
  const Scale* as;
  const int* route;
  const uint8_t* wq;
  const Scale* ws;
  const void* rw;
  void* out;
  int64_t N, Kp;
  int wdt, out_bf16, inplace, vec_ok, S, top_k, E, strips;
};
// The epilogue policy: PlainEpi is the kernel argument of inc_mx_moe_gemm / inc_fp8_moe_gemm as it is (SiLU product, no bias); GluEpi
// adds what inc_mx_moe_gemm_glu has on top -- a per-expert fp32 bias [E, N] (NULL: none) in every mode and the clamped SwiGLU of the
// GPT-OSS experts in mode 0
template <class Scale>
struct PlainEpi : StripMoeArgs<Scale> {
  static constexpr bool GLU = false;
};
template <class Scale>
struct GluEpi : StripMoeArgs<Scale> {
  static constexpr bool GLU = true;
  const float* bias;
  float alpha, limit;
};

// K-tiles of a wave whose loads are in flight together: up to 64 fragment registers per round, so that every instantiation stays
// inside 128 VGPRs (two workgroups per CU) without scratch.  Without the scale registers deeper rounds fit the FP8 cell (6 / 4 / 3 / 2:
// 124 and 88 VGPRs, no scratch) but do not pay: measured on the MI355X they are 0.96 - 1.27 x the time of these depths, slower on 12
// of 16 points ("FP8 experts")
__host__ __device__ constexpr int moe_unroll(int ns, int nb) { return ns + nb <= 2 ? 4 : ns + nb <= 4 ? 2 : 1; }

// one (strip, tile) with NB row blocks; part: the workgroup's LDS
template <class Cell, class Args, int AF, int WF, bool GATED, int NB>
__device__ __forceinline__ void moe_body(const Args& a, f32x4 (&part)[Cell::MW][RB][64], int e, int p0, int rows,
                                         int strip) {
  constexpr int NS = GATED ? 2 : 1;  // weight strips: gate and up rows of the same j
  constexpr bool SC = Cell::SCALED;
  const int64_t Nout = GATED ? a.N / 2 : a.N;
  const int64_t n0 = (int64_t)strip * STRIP;
  const StripLane L = strip_lane(n0, Nout);
  const int r = L.r, g = L.g, wave = L.wave;
  const int nk = (int)(a.Kp / XK);
  const int* const order = a.route + moe_route_layout(a.S, a.E).order;
  // the scale bytes of the rows, where the cell has them
  const uint8_t* const as8 = SC ? reinterpret_cast<const uint8_t*>(a.as) : nullptr;
  const uint8_t* const ws8 = SC ? reinterpret_cast<const uint8_t*>(a.ws) : nullptr;

  StripRow w[NS], x[NB];
#pragma unroll
  for (int s = 0; s < NS; ++s) w[s] = strip_row<WF, SC>(a.wq, ws8, (int64_t)e * a.N + s * Nout + L.wrow, nk, g);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int rr = 16 * b + r;
    const int p = rr < rows ? p0 + rr : p0;  // past the range: the tile's first row again; that column of D is never stored
    const int64_t src = a.inplace ? p : order[p] / a.top_k;
    x[b] = strip_row<AF, SC>(a.aq, as8, src, nk, g);
  }

  f32x4 acc[NS][NB];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[s][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  strip_partials<WF, AF, SC, NS, NB, moe_unroll(NS, NB), Cell::MW, false, false>(w, x, -1, wave, nk, acc);

  f32x4 res[NS];
  strip_sum_blocks<NS, NB, Cell::MW, RB>(part, acc, wave, L.lane, res);
  if (wave >= NB) return;

  // C/D map: register i of lane l is position 16 wave + r, column n0 + 4 g + i
  const int rr = 16 * wave + r;
  if (rr >= rows) return;
  const int64_t p = p0 + rr;
  const int64_t nb = n0 + 4 * g;
  if (nb >= Nout) return;
  const bool vec = a.vec_ok && nb + 4 <= Nout;
  const int slot = !SC || a.inplace ? order[p] : 0;  // read only where it is used
  if constexpr (!SC) {
    // the two factors: the row's (a valid position's source row, the only rows whose a_scale is read) and the columns'
    const float rs = a.as[a.inplace ? p : (int64_t)(slot / a.top_k)];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float* al = a.ws + (int64_t)e * a.N + s * Nout + nb;
#pragma unroll
      for (int i = 0; i < 4; ++i) res[s][i] = (rs * (nb + i < Nout ? al[i] : 0.f)) * res[s][i];
    }
  }
  if constexpr (Args::GLU) {
    // b(e, n): one fp32 add on the LDS sum, read by the lanes that store only (as the FP8 cell's factors above)
    if (a.bias) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const float* bs = a.bias + (int64_t)e * a.N + s * Nout + nb;
#pragma unroll
        for (int i = 0; i < 4; ++i) res[s][i] = res[s][i] + (nb + i < Nout ? bs[i] : 0.f);
      }
    }
  }
  if constexpr (GATED) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (Args::GLU) v[i] = glu_clamped_f32(res[0][i], res[1][i], a.alpha, a.limit);
      else v[i] = silu_mul_f32(res[0][i], res[1][i]);
    }
    uint16_t* dst = static_cast<uint16_t*>(a.out) + p * Nout + nb;  // the 16-bit type is a launch argument here: no store_quad16
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
      const float wt = moe_load_weight(a.rw, slot, a.wdt);
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

template <class Cell, class Args, int AF, int WF, bool GATED>
__global__ __launch_bounds__(Cell::MW * 64, 4) void strip_moe_gemm_kernel(const Args a) {
  __shared__ f32x4 part[Cell::MW][RB][64];
  const int tile = (int)(blockIdx.x / (unsigned)a.strips), strip = (int)(blockIdx.x - (unsigned)tile * (unsigned)a.strips);
  if (tile >= a.route[0]) return;  // more tile slots than tiles
  const RouteLayout L = moe_route_layout(a.S, a.E);
  const int e = a.route[L.tiles + 2 * tile], p0 = a.route[L.tiles + 2 * tile + 1];
  const int pe = a.route[L.offsets + e + 1];
  const int rows = pe - p0 < MOE_BM ? pe - p0 : MOE_BM;
  const int blocks = __builtin_amdgcn_readfirstlane((rows + 15) >> 4);  // row blocks of this tile: the same for the whole workgroup
  if (blocks == 1) moe_body<Cell, Args, AF, WF, GATED, 1>(a, part, e, p0, rows, strip);
  else if (blocks == 2) moe_body<Cell, Args, AF, WF, GATED, 2>(a, part, e, p0, rows, strip);
  else if (blocks == 3) moe_body<Cell, Args, AF, WF, GATED, 3>(a, part, e, p0, rows, strip);
  else moe_body<Cell, Args, AF, WF, GATED, 4>(a, part, e, p0, rows, strip);
}

template <class Cell, class Args, int AF, int WF>
void moe_launch(bool gated, unsigned grid, const Args& a, inc_stream_t stream) {
  if (gated)
    strip_moe_gemm_kernel<Cell, Args, AF, WF, true><<<grid, Cell::MW * 64, 0, inc_s(stream)>>>(a);
  else
    strip_moe_gemm_kernel<Cell, Args, AF, WF, false><<<grid, Cell::MW * 64, 0, inc_s(stream)>>>(a);
}

// the argument checks the entry points share, in their order, then the launch.  The FP8 cell has the (fp8, fp8) pair alone; bias,
// alpha and limit are the GLU epilogue's and are neither checked nor carried without it
template <class Cell, bool GLU = false>
int moe_run(int mode, const uint8_t* aq, const typename Cell::Scale* as, int afmt, const int32_t* route, const uint8_t* wq,
            const typename Cell::Scale* ws, int wfmt, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T, int top_k,
            int64_t E, int64_t N, int64_t Kp, inc_stream_t stream, const float* bias = nullptr, float alpha = 1.f, float limit = 1.f) {
  using Args = std::conditional_t<GLU, GluEpi<typename Cell::Scale>, PlainEpi<typename Cell::Scale>>;
  constexpr int F8 = INC_MX_FP8_E4M3, F4 = INC_MX_FP4_E2M1;
  INC_CHECK_ARG(mode >= 0 && mode <= 2);
  INC_CHECK_ARG(aq && as && route && wq && ws && out && T > 0 && top_k > 0 && E > 0 && N > 0 && Kp > 0);
  INC_CHECK_ARG(mode != 1 || routing_weights);
  if constexpr (GLU) INC_CHECK_ARG(limit > 0.f && alpha == alpha);
  const bool p88 = afmt == F8 && wfmt == F8;
  const bool p84 = Cell::SCALED && afmt == F8 && wfmt == F4;
  const bool p44 = Cell::SCALED && afmt == F4 && wfmt == F4;
  if (!p88 && !p84 && !p44) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  if (E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  if (mode == 0 && (N % 2) != 0) return INC_ERR_UNSUPPORTED;
  if (mode == 0 ? (odtype != INC_BF16 && odtype != INC_F16) : odtype != INC_F32) return INC_ERR_UNSUPPORTED;
  if (mode == 1 && wdtype != INC_F32 && wdtype != INC_F16 && wdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(aq) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(as) | reinterpret_cast<uintptr_t>(ws)) & (Cell::SCALE_ALIGN - 1)) == 0);
  if constexpr (GLU) INC_CHECK_ARG((reinterpret_cast<uintptr_t>(bias) & 3) == 0);
  const int64_t S = T * top_k, Nout = mode == 0 ? N / 2 : N;
  const int64_t strips = ceil_div64(Nout, STRIP), units = strips * moe_tiles_max(S, E);
  if (units >= ((int64_t)1 << 31)) return INC_ERR_UNSUPPORTED;
  Args a = {};
  if constexpr (GLU) {
    a.bias = bias; a.alpha = alpha; a.limit = limit;
  }
  a.aq = aq; a.as = as; a.route = route; a.wq = wq; a.ws = ws; a.rw = routing_weights; a.out = out;
  a.N = N; a.Kp = Kp;
  a.wdt = wdtype; a.out_bf16 = odtype == INC_BF16; a.inplace = mode == 1;
  a.vec_ok = (Nout % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & (mode == 0 ? 7 : 15)) == 0;
  a.S = (int)S; a.top_k = top_k; a.E = (int)E; a.strips = (int)strips;
  const unsigned grid = (unsigned)units;
  if (p88) moe_launch<Cell, Args, F8, F8>(mode == 0, grid, a, stream);
  if constexpr (Cell::SCALED) {
    if (p84) moe_launch<Cell, Args, F8, F4>(mode == 0, grid, a, stream);
    if (p44) moe_launch<Cell, Args, F4, F4>(mode == 0, grid, a, stream);
  }
  INC_LAUNCH_RETURN();
}

}  // namespace

extern "C" int inc_mx_moe_gemm(int mode, const uint8_t* aq, const uint8_t* as, int afmt, const int32_t* route, const uint8_t* wq,
                               const uint8_t* ws, int wfmt, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T,
                               int top_k, int64_t E, int64_t N, int64_t Kp, inc_stream_t stream) {
  return moe_run<MxCell>(mode, aq, as, afmt, route, wq, ws, wfmt, routing_weights, wdtype, out, odtype, T, top_k, E, N, Kp, stream);
}

extern "C" int inc_mx_moe_gemm_glu(int mode, const uint8_t* aq, const uint8_t* as, int afmt, const int32_t* route, const uint8_t* wq,
                                   const uint8_t* ws, int wfmt, const float* bias, float alpha, float limit, const void* routing_weights,
                                   int wdtype, void* out, int odtype, int64_t T, int top_k, int64_t E, int64_t N, int64_t Kp,
                                   inc_stream_t stream) {
  return moe_run<MxCell, true>(mode, aq, as, afmt, route, wq, ws, wfmt, routing_weights, wdtype, out, odtype, T, top_k, E, N, Kp, stream,
                               bias, alpha, limit);
}

extern "C" int inc_fp8_moe_gemm(int mode, const uint8_t* aq, const float* a_scale, const int32_t* route, const uint8_t* wq,
                                const float* alpha, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T,
                                int top_k, int64_t E, int64_t N, int64_t Kp, inc_stream_t stream) {
  return moe_run<Fp8Cell>(mode, aq, a_scale, INC_MX_FP8_E4M3, route, wq, alpha, INC_MX_FP8_E4M3, routing_weights, wdtype, out, odtype, T, top_k, E,
                          N, Kp, stream);
}
