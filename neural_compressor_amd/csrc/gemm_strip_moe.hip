// gemm_strip_moe.hip -- K16e / K17e: the routed GEMM of the fused MoE experts (strip_moe_frame.hpp: kernel, epilogues, checks) for the
// MX cell (inc_mx_moe_gemm and inc_mx_moe_gemm_glu, inc_mx_gemm's product) and the per-token / per-channel FP8 cell (inc_fp8_moe_gemm,
// inc_fp8_gemm's product).  Both keep a row's sum over its K-tiles in the instruction's accumulator: their K loop is strip_partials.
// The cells:
//   MxCell    acc carries the block scales (as / ws are E8M0 scale bytes, [rows, Kp / 32]; the scaled opcode) and f = 1: no factor
//             multiply.  Three format pairs.  W = INC_MX_MOE_WAVES (with W = INC_MX_GEMV_WAVES the sums are inc_mx_gemv's).
//   Fp8Cell   no scale bytes: no scale pointers, loads or registers, the unscaled opcode (the MX accumulator at scale bytes 127 bit for
//             bit); as = a_scale[rows] and ws = alpha[E, N] are fp32 and f(r, n) = a_scale[r] * alpha[e, n] is one
//             fp32 multiply in the epilogue; a_scale is read by the lanes that store only.  (fp8, fp8) alone; W = 8 is inc_fp8_gemv's
//             split, hence fixed.
#include "strip_moe_frame.hpp"

#ifndef INC_MX_MOE_WAVES
#define INC_MX_MOE_WAVES 8  // W: 4, 8 or 16
#endif

namespace {

// SCALED: the rows have scale bytes (as / ws, read as bytes) and the opcode is the scaled one; W: the waves
template <bool SCALED, int W>
struct RowCell {
  static constexpr int MW = W;
  template <int AF, int WF, int NS, int NB, class Args>
  static __device__ __forceinline__ void partials(const Args& a, const int64_t (&wrow)[NS], const int64_t (&src)[NB], int, int64_t,
                                                  int64_t, int nk, const StripLane& L, f32x4 (&acc)[NS][NB]) {
    // the scale bytes of the rows, where the cell has them
    const uint8_t* const as8 = SCALED ? reinterpret_cast<const uint8_t*>(a.as) : nullptr;
    const uint8_t* const ws8 = SCALED ? reinterpret_cast<const uint8_t*>(a.ws) : nullptr;
    StripRow w[NS], x[NB];
#pragma unroll
    for (int s = 0; s < NS; ++s) w[s] = strip_row<WF, SCALED>(a.wq, ws8, wrow[s], nk, L.g);
#pragma unroll
    for (int b = 0; b < NB; ++b) x[b] = strip_row<AF, SCALED>(a.aq, as8, src[b], nk, L.g);
    strip_partials<WF, AF, SCALED, NS, NB, moe_unroll(NS, NB), W, false, false>(w, x, -1, L.wave, nk, acc);
  }
};
struct MxCell : RowCell<true, INC_MX_MOE_WAVES> {
  using Scale = uint8_t;
  static constexpr bool FP4 = true, FACTOR = false;
  static constexpr uintptr_t SCALE_ALIGN = 1;
};
struct Fp8Cell : RowCell<false, 8> {
  using Scale = float;
  static constexpr bool FP4 = false, FACTOR = true;
  static constexpr uintptr_t SCALE_ALIGN = 4;
};
static_assert(MxCell::MW == 4 || MxCell::MW == 8 || MxCell::MW == 16, "W is 4, 8 or 16 (at least one wave per row block)");

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
