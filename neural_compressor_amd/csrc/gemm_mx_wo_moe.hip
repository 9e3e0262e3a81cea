// gemm_mx_wo_moe.hip -- K16we: the routed GEMM of the fused MoE experts for the weight-only MX cell (inc_mx_wo_moe_gemm and
// inc_mx_wo_moe_gemm_glu): MXFP4 / MXFP8 expert weights (MXExperts' buffers) against bf16 activations on v_mfma_f32_16x16x32_bf16,
// the weights dequantised in registers by v_cvt_scalef32_pk_bf16_fp4 / _fp8 (mx_wo_frag.hpp).  One forward of MXWeightOnlyExperts /
// MXWeightOnlyGptOssExperts is four launches, no activation quantiser and no host synchronisation:
//
//   inc_moe_route -> inc_mx_wo_moe_gemm[_glu](0) -> inc_mx_wo_moe_gemm[_glu](1) -> inc_moe_combine
//
//   val[p, n] = sum_{k < K} x[src(p), k] * value(code[e, n, k]) * 2^(ws[e, n, k / 32] - 127)       (fp32)
//
// The kernel, the tile / strip map, the LDS sum and every epilogue (bias, SiLU product or clamped SwiGLU, routing weight, 16-bit and
// fp32 stores) are strip_moe_frame.hpp's, unchanged: WoCell is a fourth reader with a K loop of its own, and WoArgs carries what the
// frame's arguments lack (K beside Kp; aq points at bf16 rows of stride K, as is not read).  The frame's moe_run checks format pairs and
// scale pointers this cell does not have, so the argument checks and the launch are wo_moe_run below.
//
// The K loop (WoCell::partials).  Wave w of 8 takes the K-tiles w, w + 8, ... ascending, MFMA steps s = 0 .. 3 of a tile in order into
// one accumulator per (strip, row block): for one expert's rows that is mx_wo_gemv_kernel's sum bit for bit.  Lane (r, g) holds the
// 32 k of weight row r at k0 + 32 g -- 16 bytes (fp4) or 32 bytes (fp8), non-temporal, straight from HBM into registers -- and one
// scale byte; wo_scale is one shift.  The 8-k fragment of step s is converted ONCE per K-tile and multiplied as the A operand against
// all NB row blocks (mode 0: the gate and the up fragment of the same j side by side), so the conversion costs half a VALU
// instruction per weight whatever the tile's row count.  The B fragment of step s and row block b is x[src(16 b + r)][k0 + 32 g + 8 s
// .. + 7], one plain 16-byte load (x stays in L2: every strip re-reads it), gathered through order[] in modes 0 / 2.  K % 8 == 0, so
// a chunk lies whole on one side of K: chunks at k >= K are zero fragments that are never loaded.  Rows past the expert's range are
// the tile's first row again (the frame's src[]); those columns of D are never stored.
// Registers.  A bf16 row block is 16 dwords of x per K-tile and lane, four times an fp8 fragment, so the frame's moe_unroll does not
// carry over: wo_moe_unroll is this cell's table, and the two widest instantiations (mode 0 with 3 or 4 row blocks) load x per MFMA
// step into one set of fragment registers instead of per tile (wo_moe_xstep).  Every instantiation stays inside the frame's 128-VGPR
// launch bound without scratch ("Weight-only MX experts", has the table).  The K loop has no fp32 VALU arithmetic,
// so the file keeps the default build (packed fp32 instructions on: the sums and products of the frame's epilogue have the same values).
#include "mx_wo_frag.hpp"
#include "strip_moe_frame.hpp"

namespace {

// K-tiles of a wave whose loads are in flight together.  Per tile and lane: 9 NS dwords of weights and scale (fp8) and 16 NB of x
__host__ __device__ constexpr int wo_moe_unroll(int ns, int nb) { return ns + nb <= 2 ? 3 : ns + nb == 3 ? 2 : 1; }
// x per MFMA step (4 NB dwords) instead of per tile
__host__ __device__ constexpr bool wo_moe_xstep(int ns, int nb) { return ns == 2 && nb >= 3; }

template <class Epi>
struct WoArgs : Epi {
  int64_t K;  // the row stride of x = the real reduction length; Kp is the weights'
};

struct WoCell {
  using Scale = uint8_t;
  static constexpr int MW = 8;  // mx_wo_gemv_kernel's split: one expert's rows carry its sums
  static constexpr bool FACTOR = false;

  template <int AF, int WF, int NS, int NB, class Args>
  static __device__ __forceinline__ void partials(const Args& a, const int64_t (&wrow)[NS], const int64_t (&src)[NB], int, int64_t,
                                                  int64_t, int nk, const StripLane& L, f32x4 (&acc)[NS][NB]) {
    constexpr int TW = mx_tile_bytes(WF), LB = TW / 4;  // bytes of a row's K-tile / of a lane's 32 k
    constexpr int U = wo_moe_unroll(NS, NB);
    const uint8_t* wp[NS];
    const uint8_t* sp[NS];
    const uint16_t* xp[NB];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      wp[s] = a.wq + wrow[s] * ((int64_t)nk * TW) + LB * L.g;
      sp[s] = a.ws + wrow[s] * ((int64_t)nk * (XK / 32)) + L.g;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) xp[b] = reinterpret_cast<const uint16_t*>(a.aq) + src[b] * a.K + 32 * L.g;
    const int64_t kleft = a.K - 32 * L.g;  // chunk (t, j) of this lane is real where t * XK + 8 j < kleft

    auto load_w = [&](int64_t t, i32x8 (&wf)[NS], int (&sb)[NS]) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const i32x4* const q = reinterpret_cast<const i32x4*>(wp[s] + t * TW);  // streamed once per tile of the route: non-temporal
        const i32x4 lo = __builtin_nontemporal_load(q);
        wf[s][0] = lo[0]; wf[s][1] = lo[1]; wf[s][2] = lo[2]; wf[s][3] = lo[3];
        if constexpr (WF == INC_MX_FP8_E4M3) {
          const i32x4 hi = __builtin_nontemporal_load(q + 1);
          wf[s][4] = hi[0]; wf[s][5] = hi[1]; wf[s][6] = hi[2]; wf[s][7] = hi[3];
        }
        sb[s] = sp[s][t * (XK / 32)];
      }
    };
    auto load_x1 = [&](int64_t t, int j, int b) {
      return t * XK + 8 * j < kleft ? *reinterpret_cast<const i32x4*>(xp[b] + t * XK + 8 * j) : i32x4{0, 0, 0, 0};
    };
    auto load_x = [&](int64_t t, int j, i32x4 (&xf)[NB]) {
#pragma unroll
      for (int b = 0; b < NB; ++b) xf[b] = load_x1(t, j, b);
    };
    // MFMA step j of a tile: each strip's fragment converted once, then against every row block
    auto step = [&](const i32x8 (&wf)[NS], const float (&sc)[NS], int j, const i32x4 (&xf)[NB]) {
      wo_bf16x8 af[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) af[s] = wo_step<WF>(wf[s], j, sc[s]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        wo_bf16x8 bf;
        __builtin_memcpy(&bf, &xf[b], 16);
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s], bf, acc[s][b], 0, 0, 0);
      }
    };
    // C of the wave's K-tiles kt, kt + MW, ...: every load first, then the MFMAs in K order
    auto round = [&](int kt, auto count) {
      constexpr int C = decltype(count)::value;
      i32x8 wf[C][NS];
      int sb[C][NS];
      if constexpr (wo_moe_xstep(NS, NB)) {
        static_assert(C == 1, "x per step is written for one tile per round");
        // one x fragment per row block: block b's fragment of step j + 1 is requested into the registers of step j's as soon as
        // the MFMAs of (j, b) have issued (an MFMA reads its operands at issue), so a step's loads fly behind the rest of the step
        // before it without a second set of registers
        i32x4 xf[NB];
        load_w(kt, wf[0], sb[0]);
        load_x(kt, 0, xf);
        float sc[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) sc[s] = wo_scale(sb[0][s]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wo_bf16x8 af[NS];
#pragma unroll
          for (int s = 0; s < NS; ++s) af[s] = wo_step<WF>(wf[0][s], j, sc[s]);
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            wo_bf16x8 bf;
            __builtin_memcpy(&bf, &xf[b], 16);
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s], bf, acc[s][b], 0, 0, 0);
            if (j < 3) xf[b] = load_x1(kt, j + 1, b);
          }
        }
      } else {
        i32x4 xf[C][4][NB];
#pragma unroll
        for (int u = 0; u < C; ++u) {
          const int64_t t = kt + u * MW;
          load_w(t, wf[u], sb[u]);
#pragma unroll
          for (int j = 0; j < 4; ++j) load_x(t, j, xf[u][j]);
        }
#pragma unroll
        for (int u = 0; u < C; ++u) {
          float sc[NS];
#pragma unroll
          for (int s = 0; s < NS; ++s) sc[s] = wo_scale(sb[u][s]);
#pragma unroll
          for (int j = 0; j < 4; ++j) step(wf[u], sc, j, xf[u][j]);
        }
      }
    };
    int kt = L.wave;
    if constexpr (U > 1)
      for (; kt + (U - 1) * MW < nk; kt += U * MW) round(kt, std::integral_constant<int, U>{});
    for (; kt < nk; kt += MW) round(kt, std::integral_constant<int, 1>{});
  }
};

// the argument checks in the header's order -- the frame's, with inc_mx_wo_gemv's K rules in place of the format pairs and bf16 alone
// in mode 0 -- then the launch of the frame's kernel
template <bool GLU>
int wo_moe_run(int mode, const void* x, const int32_t* route, const uint8_t* wq, const uint8_t* ws, int wfmt, const float* bias,
               float alpha, float limit, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T, int top_k, int64_t E,
               int64_t N, int64_t K, int64_t Kp, inc_stream_t stream) {
  using Args = WoArgs<std::conditional_t<GLU, GluEpi<uint8_t>, PlainEpi<uint8_t>>>;
  constexpr int F8 = INC_MX_FP8_E4M3, F4 = INC_MX_FP4_E2M1;
  INC_CHECK_ARG(mode >= 0 && mode <= 2);
  INC_CHECK_ARG(x && route && wq && ws && out && T > 0 && top_k > 0 && E > 0 && N > 0 && K > 0 && Kp > 0);
  INC_CHECK_ARG(mode != 1 || routing_weights);
  if constexpr (GLU) INC_CHECK_ARG(limit > 0.f && alpha == alpha);
  if (wfmt != F8 && wfmt != F4) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0 || (K % 8) != 0 || K > Kp || Kp - K >= XK) return INC_ERR_UNSUPPORTED;
  if (E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  if (mode == 0 && (N % 2) != 0) return INC_ERR_UNSUPPORTED;
  if (mode == 0 ? odtype != INC_BF16 : odtype != INC_F32) return INC_ERR_UNSUPPORTED;  // E8M0's range does not fit an fp16 h
  if (mode == 1 && wdtype != INC_F32 && wdtype != INC_F16 && wdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  if constexpr (GLU) INC_CHECK_ARG((reinterpret_cast<uintptr_t>(bias) & 3) == 0);
  const int64_t S = T * top_k, Nout = mode == 0 ? N / 2 : N;
  const int64_t strips = ceil_div64(Nout, STRIP), units = strips * moe_tiles_max(S, E);
  if (units >= ((int64_t)1 << 31)) return INC_ERR_UNSUPPORTED;
  Args a = {};
  if constexpr (GLU) {
    a.bias = bias; a.alpha = alpha; a.limit = limit;
  }
  a.aq = static_cast<const uint8_t*>(x); a.as = nullptr; a.route = route; a.wq = wq; a.ws = ws; a.rw = routing_weights; a.out = out;
  a.N = N; a.Kp = Kp; a.K = K;
  a.wdt = wdtype; a.out_bf16 = 1; a.inplace = mode == 1;
  a.vec_ok = (Nout % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & (mode == 0 ? 7 : 15)) == 0;
  a.S = (int)S; a.top_k = top_k; a.E = (int)E; a.strips = (int)strips;
  if (wfmt == F4) moe_launch<WoCell, Args, 0, F4>(mode == 0, (unsigned)units, a, stream);
  else moe_launch<WoCell, Args, 0, F8>(mode == 0, (unsigned)units, a, stream);
  INC_LAUNCH_RETURN();
}

}  // namespace

extern "C" int inc_mx_wo_moe_gemm(int mode, const void* x, const int32_t* route, const uint8_t* wq, const uint8_t* ws, int wfmt,
                                  const void* routing_weights, int wdtype, void* out, int odtype, int64_t T, int top_k, int64_t E,
                                  int64_t N, int64_t K, int64_t Kp, inc_stream_t stream) {
  return wo_moe_run<false>(mode, x, route, wq, ws, wfmt, nullptr, 1.f, 1.f, routing_weights, wdtype, out, odtype, T, top_k, E, N, K, Kp,
                           stream);
}

extern "C" int inc_mx_wo_moe_gemm_glu(int mode, const void* x, const int32_t* route, const uint8_t* wq, const uint8_t* ws, int wfmt,
                                      const float* bias, float alpha, float limit, const void* routing_weights, int wdtype, void* out,
                                      int odtype, int64_t T, int top_k, int64_t E, int64_t N, int64_t K, int64_t Kp,
                                      inc_stream_t stream) {
  return wo_moe_run<true>(mode, x, route, wq, ws, wfmt, bias, alpha, limit, routing_weights, wdtype, out, odtype, T, top_k, E, N, K, Kp,
                          stream);
}
