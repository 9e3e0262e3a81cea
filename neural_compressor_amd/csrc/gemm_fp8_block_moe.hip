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
// The kernel, the route reads, the operand map, the tile-to-wave map, the wave-order sum, the epilogue and the argument checks are
// strip_moe_frame.hpp's, with 8 waves.  What strip_partials, the K loop of that frame's other cells, cannot do is this cell's factor:
// it changes with every K-tile, so a tile's matrix-pipe sum cannot stay in the instruction's accumulator.  Here
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
#include "strip_moe_frame.hpp"

namespace {

constexpr int BW = 8;    // waves of a workgroup = ways of the K split: inc_fp8_block_gemv's, hence fixed
constexpr int WB = 128;  // rows of a weight scale block
constexpr int E4M3 = INC_MX_FP8_E4M3;

// row blocks whose x fragments are in flight together: all of them, except beside two weight strips, where three or four blocks go in
// chunks of two (the 16 or 8 fragment registers less are what keeps the gated kernel out of scratch: with all four blocks in flight at
// once it took 128 VGPRs and 28 bytes of scratch per lane; the compiler's report per instantiation is in DESIGN section 8c)
__host__ __device__ constexpr int block_moe_chunk(int ns, int nb) { return ns == 2 && nb > 2 ? 2 : nb; }

struct BlockCell {
  using Scale = float;
  static constexpr int MW = BW;
  static constexpr bool FP4 = false, FACTOR = false;  // the factors are inside the partials
  static constexpr uintptr_t SCALE_ALIGN = 4;

  template <int AF, int WF, int NS, int NB, class Args>
  static __device__ __forceinline__ void partials(const Args& a, const int64_t (&wrow)[NS], const int64_t (&src)[NB], int e, int64_t n0,
                                                  int64_t Nout, int nk, const StripLane& L, f32x4 (&acc)[NS][NB]) {
    constexpr int U = moe_unroll(NS, NB);
    constexpr int BC = block_moe_chunk(NS, NB);
    const int wave = L.wave;
    const int64_t hblk = (Nout + WB - 1) / WB;  // block rows of one half (mode 0) or of the matrix: NBLK = NS * hblk

    const uint8_t* wp[NS];
    const float* wsp[NS];  // uniform over the workgroup
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      wp[s] = strip_row<E4M3, false>(a.wq, nullptr, wrow[s], nk, L.g).q;
      wsp[s] = a.ws + (((int64_t)e * NS + s) * hblk + n0 / WB) * nk;
    }
    const uint8_t* xp[NB];
    const float* xsp[NB];  // the lane's accumulator registers of block b are columns of row 16 b + r
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      xp[b] = strip_row<E4M3, false>(a.aq, nullptr, src[b], nk, L.g).q;
      xsp[b] = a.as + src[b] * nk;
    }

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
  }
};

}  // namespace

extern "C" int inc_fp8_block_moe_gemm(int mode, const uint8_t* aq, const float* as, const int32_t* route, const uint8_t* wq,
                                      const float* ws, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T,
                                      int top_k, int64_t E, int64_t N, int64_t Kp, inc_stream_t stream) {
  return moe_run<BlockCell>(mode, aq, as, E4M3, route, wq, ws, E4M3, routing_weights, wdtype, out, odtype, T, top_k, E, N, Kp, stream);
}
