// gemm_fp8_block_moe.hip -- K18e: the routed GEMM of the fused MoE experts for the block-scaled FP8 cell (128 x 128 weight blocks,
// 1 x 128 activation groups: the experts of DeepSeek-V3 / R1, Qwen3-FP8 and FineGrainedFP8Config checkpoints), inc_fp8_block_gemv's
// product per expert over the rows inc_moe_route sorted, on v_mfma_f32_16x16x128_f8f6f4.
//
// One forward of FP8BlockExperts is six launches and no host synchronisation:
//
//   inc_moe_route -> inc_fp8_quant_groups(x) -> inc_fp8_block_moe_gemm(0) -> inc_fp8_quant_groups(h) -> inc_fp8_block_moe_gemm(1) -> inc_moe_combine
//
//   val[p, n] = sum over waves in wave order of ( sum over the wave's kt ascending of (as[r, kt] * ws[e, blk(n), kt]) * acc_kt[p, n] )
//   mode 0 (gate_up): h[p, j] = rd16( silu(g) * u ),  g = val[p, j],  u = val[p, I + j],  r = order[p] / top_k   (bf16 / fp16)
//   mode 1 (down):    y[p, n] = w[order[p]] * val[p, n],  r = p                                                   (fp32)
//   mode 2 (plain):   y[p, n] = val[p, n],  r = order[p] / top_k                                                  (fp32)
//
// The launch shape, the route reads, the operand map, the tile-to-wave map and the wave-order sum are gemm_strip_moe.hip's (workgroup =
// (strip of 16 output columns, 64-row tile of the route's table), 8 waves, wave w takes the K-tiles w, w + 8, ... ascending, only the
// ceil(rows / 16) row blocks a tile has are loaded and multiplied, strip_sum_blocks through 32 KiB of LDS).  What that kernel cannot do
// is this cell's factor: it changes with every K-tile, so a tile's matrix-pipe sum cannot stay in the instruction's accumulator.  Here
// every (strip, block, K-tile) is one MFMA from a literal-zero C operand into a 4-register temporary, promoted into the fp32 partial
// with the plain multiply-add of fp8_block_gemv_kernel (this file is built with the packed fp32 instructions off, as that one is):
//   x factor   by the C/D map a lane's four accumulator registers of block b are columns of ONE row 16 b + (lane & 15), so as[r, kt] is
//              one 4-byte load per lane, block and K-tile (the four lane groups read the same word);
//   w factor   a strip of 16 columns lies inside one 128-row block (in mode 0 the gate half and the up half are each blocked from their
//              own row 0, so this holds for every I), so ws[e, blk, kt] is one workgroup-uniform word per strip and K-tile;
//   round      U K-tiles of a wave in flight: the loads of the round -- per tile NS weight fragments and w factors, then per chunk of
//              row blocks its x fragments and x factors -- are issued in front of the chunk's first MFMA; then per tile, block outer
//              and strip inner, the MFMA, the factor product (one fp32 multiply) and four multiply-adds.  The promotion of one
//              (strip, block) runs under the MFMA of the next.  Behind the full rounds one tile at a time.  U, the chunks and the
//              tail form change no sum.
// For one expert's <= 16 rows the partial of every wave, and so the sum, is inc_fp8_block_gemv's bit for bit.
// Lanes past the end of the expert's range re-read the tile's first row (codes and factors) and lanes of a weight row past the strip's
// end re-read its last row: what they produce is never stored.  Source rows that no valid position names are never read, and ws is
// never read past block row NBLK - 1 (n0 < Nout).  No global hand-off, no workspace, no counters: repeated calls are bit-identical.
// Algorithmic bytes per launch: the weights of the experts that were hit once per 64-row tile, 4 * KB bytes of ws per strip and tile,
// the activation rows and their KB factors once per strip.
#include "moe_common.hpp"
#include "strip_frame.hpp"

namespace {

constexpr int RB = MOE_BM / 16;  // row blocks of a tile
constexpr int BW = 8;            // waves of a workgroup = ways of the K split: inc_fp8_block_gemv's, hence fixed
constexpr int WB = 128;          // rows of a weight scale block
constexpr int E4M3 = INC_MX_FP8_E4M3;

struct BlockMoeArgs {
  const uint8_t* aq;
  const float* as;
  const int* route;
  const uint8_t* wq;
  const float* ws;
  const void* rw;
  void* out;
  int64_t N, Kp;
  int wdt, out_bf16, inplace, vec_ok, S, top_k, E, strips;
};

// K-tiles of a wave whose loads are in flight together, per (weight strips, row blocks): 8 (NS + BC) U fragment registers and
// (NS + BC) U factor words per round beside the 4 NS NB partial registers, the temporaries and two pointers per block.  The table is
// moe_unroll's of gemm_strip_moe.hip; with it and the chunks below both kernels stay inside 128 VGPRs (launch bounds (512, 4): two
// workgroups per CU) without scratch.  With all four blocks of the gated kernel in flight at once it took 128 VGPRs and 28 bytes of
// scratch per lane; the compiler's report per instantiation is in DESIGN section 8c ("FP8 block-scaled experts")
__host__ __device__ constexpr int block_moe_unroll(int ns, int nb) { return ns + nb <= 2 ? 4 : ns + nb <= 4 ? 2 : 1; }

// row blocks whose x fragments are in flight together: all of them, except beside two weight strips, where three or four blocks go in
// chunks of two (the 16 or 8 fragment registers less are what keeps the gated kernel out of scratch)
__host__ __device__ constexpr int block_moe_chunk(int ns, int nb) { return ns == 2 && nb > 2 ? 2 : nb; }

// one (strip, tile) with NB row blocks; part: the workgroup's LDS
template <bool GATED, int NB>
__device__ __forceinline__ void block_moe_body(const BlockMoeArgs& a, f32x4 (&part)[BW][RB][64], int e, int p0, int rows, int strip) {
  constexpr int NS = GATED ? 2 : 1;  // weight strips: gate and up rows of the same j
  constexpr int U = block_moe_unroll(NS, NB);
  constexpr int BC = block_moe_chunk(NS, NB);
  const int64_t Nout = GATED ? a.N / 2 : a.N;
  const int64_t n0 = (int64_t)strip * STRIP;
  const StripLane L = strip_lane(n0, Nout);
  const int r = L.r, g = L.g, wave = L.wave;
  const int nk = (int)(a.Kp / XK);
  const int* const order = a.route + moe_route_layout(a.S, a.E).order;
  const int64_t hblk = (Nout + WB - 1) / WB;  // block rows of one half (mode 0) or of the matrix: NBLK = NS * hblk

  const uint8_t* wp[NS];
  const float* wsp[NS];  // uniform over the workgroup
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    wp[s] = strip_row<E4M3, false>(a.wq, nullptr, (int64_t)e * a.N + s * Nout + L.wrow, nk, g).q;
    wsp[s] = a.ws + (((int64_t)e * NS + s) * hblk + n0 / WB) * nk;
  }
  const uint8_t* xp[NB];
  const float* xsp[NB];  // the lane's accumulator registers of block b are columns of row 16 b + r
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int rr = 16 * b + r;
    const int p = rr < rows ? p0 + rr : p0;  // past the range: the tile's first row again; that column of D is never stored
    const int64_t src = a.inplace ? p : order[p] / a.top_k;
    xp[b] = strip_row<E4M3, false>(a.aq, nullptr, src, nk, g).q;
    xsp[b] = a.as + src * nk;
  }

  f32x4 acc[NS][NB];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[s][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // C of the wave's K-tiles kt, kt + BW, ...: the weight fragments and factors of the round, then per chunk of BC row blocks its x
  // fragments and factors, every load of a chunk in front of its first MFMA; per tile, block and strip the MFMA and its promotion
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[NS][C];
    float sw[NS][C];
#pragma unroll
    for (int u = 0; u < C; ++u)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        wf[s][u] = mx_frag<E4M3, true>(wp[s] + (int64_t)(kt + u * BW) * XK);
        sw[s][u] = wsp[s][kt + u * BW];
      }
#pragma unroll
    for (int b0 = 0; b0 < NB; b0 += BC) {
      i32x8 xf[BC][C];
      float sx[BC][C];
#pragma unroll
      for (int u = 0; u < C; ++u)
#pragma unroll
        for (int c = 0; c < BC; ++c)
          if (b0 + c < NB) {
            xf[c][u] = mx_frag<E4M3, false>(xp[b0 + c] + (int64_t)(kt + u * BW) * XK);
            sx[c][u] = xsp[b0 + c][kt + u * BW];
          }
#pragma unroll
      for (int u = 0; u < C; ++u)
#pragma unroll
        for (int c = 0; c < BC; ++c)
          if (b0 + c < NB) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
              const f32x4 tmp = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[s][u], xf[c][u], zero, E4M3, E4M3, 0, 0, 0, 0);
              const float f = sx[c][u] * sw[s][u];
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[s][b0 + c][i] = f * tmp[i] + acc[s][b0 + c][i];
            }
          }
    }
  };
  int kt = wave;
  for (; kt + (U - 1) * BW < nk; kt += U * BW) round(kt, std::integral_constant<int, U>{});
  for (; kt < nk; kt += BW) round(kt, std::integral_constant<int, 1>{});

  f32x4 res[NS];
  strip_sum_blocks<NS, NB, BW, RB>(part, acc, wave, L.lane, res);
  if (wave >= NB) return;

  // C/D map: register i of lane l is position 16 wave + r, column n0 + 4 g + i
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
    uint16_t* dst = static_cast<uint16_t*>(a.out) + p * Nout + nb;  // the 16-bit type is a launch argument here
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

template <bool GATED>
__global__ __launch_bounds__(BW * 64, 4) void fp8_block_moe_gemm_kernel(const BlockMoeArgs a) {
  __shared__ f32x4 part[BW][RB][64];
  const int tile = (int)(blockIdx.x / (unsigned)a.strips), strip = (int)(blockIdx.x - (unsigned)tile * (unsigned)a.strips);
  if (tile >= a.route[0]) return;  // more tile slots than tiles
  const RouteLayout L = moe_route_layout(a.S, a.E);
  const int e = a.route[L.tiles + 2 * tile], p0 = a.route[L.tiles + 2 * tile + 1];
  const int pe = a.route[L.offsets + e + 1];
  const int rows = pe - p0 < MOE_BM ? pe - p0 : MOE_BM;
  const int blocks = __builtin_amdgcn_readfirstlane((rows + 15) >> 4);  // row blocks of this tile: the same for the whole workgroup
  if (blocks == 1) block_moe_body<GATED, 1>(a, part, e, p0, rows, strip);
  else if (blocks == 2) block_moe_body<GATED, 2>(a, part, e, p0, rows, strip);
  else if (blocks == 3) block_moe_body<GATED, 3>(a, part, e, p0, rows, strip);
  else block_moe_body<GATED, 4>(a, part, e, p0, rows, strip);
}

}  // namespace

extern "C" int inc_fp8_block_moe_gemm(int mode, const uint8_t* aq, const float* as, const int32_t* route, const uint8_t* wq,
                                      const float* ws, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T,
                                      int top_k, int64_t E, int64_t N, int64_t Kp, inc_stream_t stream) {
  // inc_fp8_moe_gemm's checks, in its order
  INC_CHECK_ARG(mode >= 0 && mode <= 2);
  INC_CHECK_ARG(aq && as && route && wq && ws && out && T > 0 && top_k > 0 && E > 0 && N > 0 && Kp > 0);
  INC_CHECK_ARG(mode != 1 || routing_weights);
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  if (E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  if (mode == 0 && (N % 2) != 0) return INC_ERR_UNSUPPORTED;
  if (mode == 0 ? (odtype != INC_BF16 && odtype != INC_F16) : odtype != INC_F32) return INC_ERR_UNSUPPORTED;
  if (mode == 1 && wdtype != INC_F32 && wdtype != INC_F16 && wdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(aq) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(as) | reinterpret_cast<uintptr_t>(ws)) & 3) == 0);
  const int64_t S = T * top_k, Nout = mode == 0 ? N / 2 : N;
  const int64_t strips = ceil_div64(Nout, STRIP), units = strips * moe_tiles_max(S, E);
  if (units >= ((int64_t)1 << 31)) return INC_ERR_UNSUPPORTED;
  BlockMoeArgs a = {};
  a.aq = aq; a.as = as; a.route = route; a.wq = wq; a.ws = ws; a.rw = routing_weights; a.out = out;
  a.N = N; a.Kp = Kp;
  a.wdt = wdtype; a.out_bf16 = odtype == INC_BF16; a.inplace = mode == 1;
  a.vec_ok = (Nout % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & (mode == 0 ? 7 : 15)) == 0;
  a.S = (int)S; a.top_k = top_k; a.E = (int)E; a.strips = (int)strips;
  const unsigned grid = (unsigned)units;
  if (mode == 0)
    fp8_block_moe_gemm_kernel<true><<<grid, BW * 64, 0, inc_s(stream)>>>(a);
  else
    fp8_block_moe_gemm_kernel<false><<<grid, BW * 64, 0, inc_s(stream)>>>(a);
  INC_LAUNCH_RETURN();
}
