// strip_frame.hpp -- the frame every "strip" kernel on v_mfma_(scale_)f32_16x16x128_f8f6f4 is written against: the MX decode GEMV
// (gemm_mx_gemv.hip: member table and fragments; its loop and sum are written out), the FP8 per-token decode GEMVs (gemm_fp8_group.hip) and the routed experts GEMM of both cells (gemm_strip_moe.hip).
// A kernel file keeps what is its own -- where its rows come from and what its epilogue multiplies -- and takes the rest from here.
//
//   workgroup   owns STRIP = 16 weight rows (one strip; gate AND up strip where NS = 2) over all of K against NB blocks of 16 rows of x.
//               The weight rows are the A operand and the rows of x the B operand, so a K-tile of 128 elements is one instruction per
//               (strip, block) and the accumulator's rows are output columns.
//   operands    lane l holds row r = l & 15, lane group g = l >> 4 (tools/mx_lab.hip).  fp8: registers 0 .. 3 are
//               the 16 bytes at 16 g of the K-tile and 4 .. 7 the 16 bytes at 64 + 16 g; fp4: registers 0 .. 3 are the 16 bytes of
//               block g (4 .. 7 are not read); either format: the scale byte of block g.  A lane loads that straight from global
//               memory into the instruction's registers (mx_frag): non-temporal for the weights, plain for x.  A weight row past N
//               re-reads row N - 1; what it produces is never stored.
//   K loop      strip_partials: K is split INSIDE the workgroup, wave w of W takes the K-tiles w, w + W, ... in ascending order, U of
//               them per round with every load of the round (per tile: weight fragment, weight scale byte, x fragment, x scale byte)
//               in front of its first MFMA; MFMA order per tile: row block outer, strip inner.  Behind the full rounds either the
//               cascade (one round of the 1 .. 3 tiles left, depth 4 only) or one tile at a time.  U and the tail form change no sum.
//   sum         the W partials meet in LDS and are added in wave order, part[0] + part[1] + ...: by wave 0 (GEMV form,
//               strip_sum_wave0) or by wave b for row block b, one strip at a time through the same LDS (experts form,
//               strip_sum_blocks).  No global hand-off, no counters, no workspace: repeated calls are bit-identical.
//   C/D map     register e of lane l is D[4 (l >> 4) + e][l & 15] = (row l & 15 of the block, column n0 + 4 g + e): a lane stores 4
//               adjacent columns of one row (store_quad16 of tile256_frame.hpp for 16-bit outputs).
// Every cross-kernel identity of the family (multi == gemv, gated == experts mode 0, fp8 == mx at scale bytes 127, one expert == gemv)
// rests on the tile-to-wave map, the ascending K inside a wave and the wave-order sum; they are defined here and, written out for its
// codegen, in mx_gemv_kernel (gemm_mx_gemv.hip), nowhere else.
// SCALED = false issues the builtin with literal zero scale operands, which the compiler emits as the UNSCALED opcode (no scale
// register); it equals the scaled opcode with both scale bytes 127 bit for bit (profiles/mx/mx_lab.log).
#pragma once
#include <type_traits>

#include "tile256_frame.hpp"  // BiasQuad, load_bias_quad, store_quad16

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int XK = INC_MX_KTILE;
constexpr int STRIP = 16;  // weight rows of a workgroup: the instruction's M
constexpr int STRIP_MAX_MEMBERS = 8;

__host__ __device__ constexpr int mx_tile_bytes(int fmt) { return fmt == INC_MX_FP8_E4M3 ? XK : XK / 2; }  // of one row and K-tile

// what a lane supplies of its row for the K-tile at `p` (= row + tile + 16 g), as the instruction wants it
template <int F, bool NT>
__device__ __forceinline__ i32x8 mx_frag(const uint8_t* p) {
  const i32x4* q = reinterpret_cast<const i32x4*>(p);
  const i32x4 lo = NT ? __builtin_nontemporal_load(q) : q[0];
  i32x4 hi = {0, 0, 0, 0};
  if constexpr (F == INC_MX_FP8_E4M3) hi = NT ? __builtin_nontemporal_load(q + 4) : q[4];
  i32x8 f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
  f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}

// ---- the lane preamble ---------------------------------------------------------------------------------------------------------------
// wrow: the lane's weight row of the strip at n0, clamped to N - 1.  GEMVs (x is [M, .], M <= 16): the lane's row of x, clamped, and
// the mask that turns the codes of a row >= M into zeros
struct StripLane {
  int lane, wave, r, g;
  int64_t wrow;
  int xrow, xkeep;
};
__device__ __forceinline__ StripLane strip_lane(int64_t n0, int64_t N, int M = STRIP) {
  StripLane L;
  L.lane = threadIdx.x & 63;
  L.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  L.r = L.lane & 15;
  L.g = L.lane >> 4;
  L.wrow = n0 + L.r;
  if (L.wrow > N - 1) L.wrow = N - 1;
  L.xrow = L.r < M ? L.r : M - 1;
  L.xkeep = L.r < M ? -1 : 0;
  return L;
}

// a lane's row of one operand at K-tile 0: its codes (+ 16 g) and, where the cell has block scales, its scale bytes (+ g)
struct StripRow {
  const uint8_t* q;
  const uint8_t* s;
};
template <int F, bool SCALED>
__device__ __forceinline__ StripRow strip_row(const uint8_t* q, const uint8_t* s, int64_t row, int nk, int g) {
  return {q + row * ((int64_t)nk * mx_tile_bytes(F)) + 16 * g, SCALED ? s + row * ((int64_t)nk * (XK / 32)) + g : nullptr};
}

// ---- the K loop ----------------------------------------------------------------------------------------------------------------------
// acc[s][b] += this wave's share of sum_k w_s[., k] * x_b[., k] (x block-scaled where SCALED).  W waves, U tiles per round; MASKX: and
// the x fragments with xkeep; CASCADE: the tail form
template <int WF, int XF, bool SCALED, int NS, int NB, int U, int W, bool MASKX, bool CASCADE>
__device__ __forceinline__ void strip_partials(const StripRow (&w)[NS], const StripRow (&x)[NB], int xkeep, int wave, int nk,
                                               f32x4 (&acc)[NS][NB]) {
  static_assert(!CASCADE || U == 4, "the cascade is written for depth 4");
  constexpr int TW = mx_tile_bytes(WF), TX = mx_tile_bytes(XF);
  // C of the wave's K-tiles kt, kt + W, ...: every load first, then the MFMAs in K order
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[NS][C], xf[NB][C];
    int sw[NS][C], sx[NB][C];
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * W;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        wf[s][u] = mx_frag<WF, true>(w[s].q + t * TW);
        if constexpr (SCALED) sw[s][u] = w[s].s[t * 4];
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        xf[b][u] = mx_frag<XF, false>(x[b].q + t * TX);
        if constexpr (SCALED) sx[b][u] = x[b].s[t * 4];
      }
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
      if constexpr (MASKX) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int d = 0; d < 8; ++d) xf[b][u][d] &= xkeep;
      }
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if constexpr (SCALED)
            acc[s][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[s][u], xf[b][u], acc[s][b], WF, XF, 0, sw[s][u], 0, sx[b][u]);
          else
            acc[s][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[s][u], xf[b][u], acc[s][b], WF, XF, 0, 0, 0, 0);
        }
    }
  };
  int kt = wave;
  for (; kt + (U - 1) * W < nk; kt += U * W) round(kt, std::integral_constant<int, U>{});
  if constexpr (CASCADE) {
    const int left = kt < nk ? (nk - kt + W - 1) / W : 0;  // 0 .. 3 tiles of this wave remain
    if (left == 3) round(kt, std::integral_constant<int, 3>{});
    else if (left == 2) round(kt, std::integral_constant<int, 2>{});
    else if (left == 1) round(kt, std::integral_constant<int, 1>{});
  } else {
    for (; kt < nk; kt += W) round(kt, std::integral_constant<int, 1>{});
  }
}

// ---- the wave-order sum through LDS --------------------------------------------------------------------------------------------------
// GEMV form (one row block): every strip's partials at once; wave 0 leaves with sum[s] = part[s][0] + part[s][1] + ..., the other
// waves with nothing: the caller returns them
template <int NS, int W>
__device__ __forceinline__ void strip_sum_wave0(f32x4 (&part)[NS][W][64], const f32x4 (&acc)[NS][1], int wave, int lane, f32x4 (&sum)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) part[s][wave][lane] = acc[s][0];
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int s = 0; s < NS; ++s) sum[s] = part[s][0][lane];
#pragma unroll
  for (int w = 1; w < W; ++w)
#pragma unroll
    for (int s = 0; s < NS; ++s) sum[s] += part[s][w][lane];
}

// experts form: wave b < NB leaves with res[s] = the sum of row block b over the waves, in wave order; one strip at a time through
// the same LDS
template <int NS, int NB, int W, int RB>
__device__ __forceinline__ void strip_sum_blocks(f32x4 (&part)[W][RB][64], const f32x4 (&acc)[NS][NB], int wave, int lane, f32x4 (&res)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s) __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) part[wave][b][lane] = acc[s][b];
    __syncthreads();
    if (wave < NB) {
      f32x4 sum = part[0][wave][lane];
#pragma unroll
      for (int w = 1; w < W; ++w) sum += part[w][wave][lane];
      res[s] = sum;
    }
  }
}

// ---- the member table of the multi launches ------------------------------------------------------------------------------------------
// the weight matrices of one launch, passed by value; member i owns the strips first[i] .. first[i + 1] - 1 of the grid.  S: what a
// member has beside its codes -- uint8_t scale bytes (MX) or float column factors (FP8)
template <class S>
struct StripMembers {
  const uint8_t* wq[STRIP_MAX_MEMBERS];
  const S* ws[STRIP_MAX_MEMBERS];
  const uint16_t* bias[STRIP_MAX_MEMBERS];
  uint16_t* y[STRIP_MAX_MEMBERS];
  int64_t N[STRIP_MAX_MEMBERS];
  int first[STRIP_MAX_MEMBERS + 1];
  int y_vec_ok[STRIP_MAX_MEMBERS];
  int n;
};

template <class S>
__device__ __forceinline__ int strip_member(const StripMembers<S>& mem, int strip) {
  int mi = 0;
  for (int i = 1; i < mem.n; ++i)
    if (strip >= mem.first[i]) mi = i;
  return mi;
}

// host: fills the table of n members (the pointers are non-null, N[i] > 0); mem.first[n] is the grid
template <class S>
int strip_members_fill(StripMembers<S>& mem, int n, const uint8_t* const* wq, const S* const* ws, const void* const* bias, void* const* y,
                       const int64_t* N) {
  int64_t strips = 0;
  for (int i = 0; i < n; ++i) {
    INC_CHECK_ARG((reinterpret_cast<uintptr_t>(wq[i]) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws[i]) & 3) == 0);
    mem.wq[i] = wq[i];
    mem.ws[i] = ws[i];
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
  return INC_OK;
}

// ---- the FP8 quad epilogue -----------------------------------------------------------------------------------------------------------
// v[e] = (rs * alpha[nb + e]) * sum[e] + bias[nb + e]: the factor product is one fp32 multiply; the multiply by the sum and the bias
// add (0.f without a bias) may contract to one fma
template <bool IS_BF16>
__device__ __forceinline__ void fp8_quad(float rs, const float* alpha, const uint16_t* bias, int64_t nb, int64_t N, const f32x4& sum,
                                         float (&v)[4]) {
  const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float al = nb + e < N ? alpha[nb + e] : 0.f;
    v[e] = (rs * al) * sum[e] + bq.b[e];
  }
}
