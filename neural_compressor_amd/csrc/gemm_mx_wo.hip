// gemm_mx_wo.hip -- K16w: the weight-only MX cell.  MXFP4 / MXFP8 weights (the codes and E8M0 block scales inc_mx_quant stores)
// against bf16 activations on the bf16 MFMAs, the weights dequantised in registers by the scaled conversions of gfx950:
//
//   y[m, n] = rd16( sum_{k < K} x[m, k] * W[n, k]  +  bias[n] ),   W[n, k] = value(code[n, k]) * 2^(ws[n, k / 32] - 127)
//
// v_cvt_scalef32_pk_bf16_fp4 / _fp8 take packed codes and an fp32 scale and return two bf16 values: half a VALU instruction per
// weight.  Every W[n, k] is exact in bf16 (1 or 3 mantissa bits against 7, the exponent range of fp32), so the product is that of x
// with MXLinear.recover(bfloat16), accumulated in fp32.  What the conversions do -- which nibble / byte pair a selector names, that the
// result is exact for every code at scale bytes 16 .. 240, a zero code gives zero at every scale byte, what happens below 2^-126 -- is
// pinned on the device by tools/mx_cvt_lab.hip (profiles/mx/mx_cvt_lab.log); the scale operand of a block is
// as_float(byte << 23), one shift.
//
// inc_mx_wo_gemv, 1 <= M <= 16: the strip shape of strip_frame.hpp on v_mfma_f32_16x16x32_bf16.  One workgroup per 16 weight rows, the
//   K-tiles of 128 split over its 8 waves in ascending order, the partials added in wave order through LDS (strip_sum_wave0): no
//   workspace, no counters, repeated calls are bit-identical.  Lane (r = l & 15, g = l >> 4) loads the 16 bytes (fp4: one whole MX
//   block) or 32 bytes (fp8) of weight row r that cover k = 32 g .. 32 g + 31 of the tile and their one scale byte, non-temporal,
//   straight into registers; dword s (fp8: dwords 2 s, 2 s + 1) converted is its A fragment of MFMA step s, and its B fragment of that
//   step is x[m = r][k0 + 32 g + 8 s .. + 7], one 16-byte load (x stays in L2: every strip re-reads it).  The k order inside a tile
//   is free as long as A and B agree.  All loads of a round (UNROLL tiles) are issued in front of its first MFMA.
// inc_mx_wo_gemm, any M: the direct-to-register design of gemm_d2r.hip.  256 x 256 tile, four waves, wave w owns all 256 rows of x
//   against output columns 64 w .. 64 w + 63 on v_mfma_f32_32x32x16_bf16 (2 x 8 accumulators of 32 x 32).  x comes in by LDS-DMA through
//   the frame's row stage (RowStage<128, 8>: stages of 64 k, three of them, two steps ahead); the weights never touch LDS: lane (row
//   l & 31, kg = l >> 5) loads the 32 k of its row and K-step straight from global memory two K-steps ahead (16 bytes = one MX block
//   for fp4, 2 x 16 bytes for fp8, one scale byte) and converts 8 k per MFMA step, so MFMA step j of a K-step multiplies
//   k = 32 kg + 8 j .. + 7 and reads the 16-byte chunk 4 kg + j of the x rows.  Every request of the loop (weight loads and DMA) is an
//   asm statement and every wait a counted s_waitcnt: the compiler's own wait insertion does not see the DMA.  No split-K.
// Edges, both kernels: rows of x past M contribute nothing that is stored (GEMV: zero fragments; GEMM: row M - 1 again), weight rows
// past N re-read row N - 1, and for K < Kp the 8-element chunks of x at k >= K are not read (GEMV: zero fragments; GEMM: the DMA
// re-reads the row's last real chunk and the weight codes there are replaced by zero codes).
#include "mx_wo_frag.hpp"  // the conversions: wo_step, wo_cvt_fp4 / _fp8, wo_scale

namespace {

// ==== the decode GEMV ====================================================================================================================
constexpr int VW = 8;      // waves of a workgroup = ways of the in-workgroup K split
constexpr int VUNROLL = 4; // K-tiles of a wave whose loads are in flight together

template <bool IS_BF16, int WF>
__global__ __launch_bounds__(VW * 64) void mx_wo_gemv_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ wq,
                                                             const uint8_t* __restrict__ ws, const uint16_t* __restrict__ bias,
                                                             uint16_t* __restrict__ y, int M, int64_t N, int64_t K, int64_t Kp,
                                                             int y_vec_ok) {
  __shared__ f32x4 part[1][VW][64];
  const int64_t n0 = (int64_t)blockIdx.x * STRIP;
  const StripLane L = strip_lane(n0, N, M);
  constexpr int TW = mx_tile_bytes(WF), LB = TW / 4;  // bytes of a row's K-tile / of a lane's 32 k
  const uint8_t* const wp = wq + L.wrow * (Kp / XK * TW) + LB * L.g;
  const uint8_t* const wsp = ws + L.wrow * (Kp / 32) + L.g;
  const uint16_t* const xp = x + (int64_t)L.xrow * K + 32 * L.g;
  const int nk = (int)(Kp / XK);
  const int klane = 32 * L.g;  // the lane's first k inside a tile

  f32x4 acc[1][1] = {{{0.f, 0.f, 0.f, 0.f}}};
  // C of the wave's K-tiles kt, kt + VW, ...: every load first, then the MFMAs in K order
  auto round = [&](int kt, auto count) {
    constexpr int C = decltype(count)::value;
    i32x8 wf[C];
    i32x4 xf[C][4];
    int sb[C];
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int64_t t = kt + u * VW;
      const i32x4* const q = reinterpret_cast<const i32x4*>(wp + t * TW);  // streamed once: non-temporal
      const i32x4 lo = __builtin_nontemporal_load(q);
      wf[u][0] = lo[0]; wf[u][1] = lo[1]; wf[u][2] = lo[2]; wf[u][3] = lo[3];
      if constexpr (WF == INC_MX_FP8_E4M3) {
        const i32x4 hi = __builtin_nontemporal_load(q + 1);
        wf[u][4] = hi[0]; wf[u][5] = hi[1]; wf[u][6] = hi[2]; wf[u][7] = hi[3];
      }
      sb[u] = wsp[t * 4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int64_t k = t * XK + klane + 8 * s;  // K % 8 == 0: a chunk lies whole on one side of K
        xf[u][s] = (L.xkeep && k < K) ? *reinterpret_cast<const i32x4*>(xp + t * XK + 8 * s) : i32x4{0, 0, 0, 0};
      }
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const float sc = wo_scale(sb[u]);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        wo_bf16x8 b;
        __builtin_memcpy(&b, &xf[u][s], 16);
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wo_step<WF>(wf[u], s, sc), b, acc[0][0], 0, 0, 0);
      }
    }
  };
  int kt = L.wave;
  for (; kt + (VUNROLL - 1) * VW < nk; kt += VUNROLL * VW) round(kt, std::integral_constant<int, VUNROLL>{});
  const int left = kt < nk ? (nk - kt + VW - 1) / VW : 0;  // 0 .. VUNROLL - 1 tiles of this wave remain
  if (left == 3) round(kt, std::integral_constant<int, 3>{});
  else if (left == 2) round(kt, std::integral_constant<int, 2>{});
  else if (left == 1) round(kt, std::integral_constant<int, 1>{});

  f32x4 sum[1];
  strip_sum_wave0<1, VW>(part, acc, L.wave, L.lane, sum);
  if (L.wave != 0) return;
  // C/D map of the 16 x 16 MFMA: register e of lane l is D[4 (l >> 4) + e][l & 15] = y[m = l & 15][n0 + 4 g + e]
  const int64_t nb = n0 + 4 * L.g;
  if (L.r >= M || nb >= N) return;
  const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = sum[0][e] + bq.b[e];
  store_quad16<IS_BF16>(y, L.r, nb, N, y_vec_ok, v);
}

// ==== the tile GEMM ======================================================================================================================
// The 2 x 8 accumulators of 32 x 32 are the AGPR half of the register file, addressed literally by asm statements only -- accumulator
// j = 8 nf + mf is a[16 j : 16 j + 15] -- as in gemm_d2r.hip: written as `f32x16 acc[2][8]` the compiler moved them between the two
// halves of the file and spilled (2.5 KiB of scratch per lane).  The first statement clobbers a0 .. a255, which makes the kernel
// descriptor allocate them; the kernel's own values fit the 256 VGPRs, so the compiler has no use for an AGPR.
template <int B, int E, class F>
__device__ __forceinline__ void wo_static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    wo_static_for<B + 1, E>(f);
  }
}
template <int R>
__device__ __forceinline__ float wo_acc_read() {
  float v;
  asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(v) : "i"(R));
  return v;
}
#define WO_A10(P) "a" #P "0", "a" #P "1", "a" #P "2", "a" #P "3", "a" #P "4", "a" #P "5", "a" #P "6", "a" #P "7", "a" #P "8", "a" #P "9"
#define WO_AGPR_CLOBBERS                                                                                                             \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", WO_A10(1), WO_A10(2), WO_A10(3), WO_A10(4), WO_A10(5), WO_A10(6),      \
  WO_A10(7), WO_A10(8), WO_A10(9), WO_A10(10), WO_A10(11), WO_A10(12), WO_A10(13), WO_A10(14), WO_A10(15), WO_A10(16), WO_A10(17),   \
  WO_A10(18), WO_A10(19), WO_A10(20), WO_A10(21), WO_A10(22), WO_A10(23), WO_A10(24), "a250", "a251", "a252", "a253", "a254", "a255"

constexpr int WO_TM = 256, WO_TN = 256, WO_TK = 64;  // a K-step is 64 k: 128 bytes of an x row, two MX blocks of a weight row
constexpr int WO_THREADS = 256;
constexpr int WO_NS = 3;                             // x stages; the DMA and the weight loads run WO_NS - 1 steps ahead
constexpr int WO_STAGE = WO_TM * WO_TK * 2;          // 32 KiB

template <bool IS_BF16, int WF>
__global__ __launch_bounds__(WO_THREADS) void mx_wo_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ wq,
                                                                const uint8_t* __restrict__ ws, const uint16_t* __restrict__ bias,
                                                                uint16_t* __restrict__ y, int64_t M, int64_t N, int64_t K, int64_t Kp,
                                                                int y_vec_ok) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool FP4 = WF == INC_MX_FP4_E2M1;
  constexpr int NQ = FP4 ? 1 : 2;        // 16-byte loads per weight row and K-step
  constexpr int NREQ = 2 * NQ + 2 + 8;   // requests of one step: the weight loads and scale bytes of two rows, 8 DMA pieces
  using XStage = RowStage<WO_TK * 2, 8>;
  const int tiles_n = (int)((N + WO_TN - 1) / WO_TN);
  const int tiles_m = (int)((M + WO_TM - 1) / WO_TM);
  const int tiles = tiles_m * tiles_n;
  const int wg = xcd_remap(blockIdx.x, tiles);
  int tm, tn;
  banded_tile_decode(wg, tiles_m, tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * WO_TM, n0 = (int64_t)tn * WO_TN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const int nk = (int)((K + WO_TK - 1) / WO_TK);            // a K-step that is all padding is not run
  const int tail_chunks = (int)((K - (int64_t)(nk - 1) * WO_TK) / 8);  // real 16-byte chunks of an x row in the last step: 1 .. 8

  // ---- x by LDS-DMA: the frame's swizzled row stage, 8 pieces per wave.  The last step of a K that is no multiple of 64 has offsets
  // of its own: a chunk at k >= K re-reads the row's last real chunk (finite, and multiplied by zero codes)
  uint32_t xoff[8], xoff_tail[8];
  XStage::offsets(wave, lane, m0, M, 2 * K, xoff);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int R = (wave * 8 + i) * XStage::RPI + lane / XStage::CPR;
    const int c = (lane % XStage::CPR) ^ XStage::swz(R);
    xoff_tail[i] = c < tail_chunks ? xoff[i] : xoff[i] - 16 * (c - (tail_chunks - 1));
  }
  const char* const xtile = reinterpret_cast<const char*>(x + m0 * K);
  auto issue_x = [&](int kt, int stage) {  // kt <= nk - 1
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + stage * WO_STAGE + wave * 8192);
    const char* src = xtile + (int64_t)kt * (WO_TK * 2);
    if (kt == nk - 1)
      lds_dma_8x1k<1024>(src, dst, xoff_tail[0], xoff_tail[1], xoff_tail[2], xoff_tail[3], xoff_tail[4], xoff_tail[5], xoff_tail[6], xoff_tail[7]);
    else
      lds_dma_8x1k<1024>(src, dst, xoff[0], xoff[1], xoff[2], xoff[3], xoff[4], xoff[5], xoff[6], xoff[7]);
  };

  // ---- weights: rows n0 + 64 wave + 32 nf + l31 (clamped), the 32 k at 32 kg of the K-step; byte offsets from the tile's first row
  uint32_t woff[2], soff[2];
  const int64_t ldw = FP4 ? Kp / 2 : Kp, lds_ = Kp / 32;
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    int64_t r = n0 + wave * 64 + nf * 32 + l31;
    if (r > N - 1) r = N - 1;
    woff[nf] = (uint32_t)((r - n0) * ldw + (FP4 ? 16 : 32) * kg);
    soff[nf] = (uint32_t)((r - n0) * lds_ + kg);
  }
  const uint8_t* const wtile = wq + n0 * ldw;
  const uint8_t* const stile = ws + n0 * lds_;
  wo_u32x4 W[WO_NS][2][NQ];
  uint32_t SB[WO_NS][2];
#define WO_LOAD16(DST, VOFF, BASE, OFF) asm volatile("global_load_dwordx4 %0, %1, %2 offset:%c3" : "=&v"(DST) : "v"(VOFF), "s"(BASE), "i"(OFF) : "memory")
#define WO_LOAD1(DST, VOFF, BASE) asm volatile("global_load_ubyte %0, %1, %2" : "=&v"(DST) : "v"(VOFF), "s"(BASE) : "memory")
  auto issue_w = [&W, &SB, &woff, &soff, wtile, stile](int kt, auto set) {  // kt <= nk - 1
    constexpr int S = decltype(set)::value;
    const uint8_t* wsrc = wtile + (int64_t)kt * (FP4 ? 32 : 64);
    const uint8_t* ssrc = stile + (int64_t)kt * 2;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      WO_LOAD16(W[S][nf][0], woff[nf], wsrc, 0);
      if constexpr (!FP4) WO_LOAD16(W[S][nf][NQ - 1], woff[nf], wsrc, 16);
      WO_LOAD1(SB[S][nf], soff[nf], ssrc);
    }
  };
  // the counted wait in front of step t: the requests of step t - 2 (weights and x of step t) are back, those of step t - 1 may be out
  auto wait_set = [&W, &SB](auto set, auto outstanding) {
    constexpr int S = decltype(set)::value;
    if constexpr (FP4)
      asm volatile("s_waitcnt vmcnt(%c4)" : "+v"(W[S][0][0]), "+v"(W[S][1][0]), "+v"(SB[S][0]), "+v"(SB[S][1]) : "i"(decltype(outstanding)::value) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%c6)" : "+v"(W[S][0][0]), "+v"(W[S][0][NQ - 1]), "+v"(W[S][1][0]), "+v"(W[S][1][NQ - 1]), "+v"(SB[S][0]), "+v"(SB[S][1])
                   : "i"(decltype(outstanding)::value) : "memory");
  };

  asm volatile("" : : : WO_AGPR_CLOBBERS);
  wo_static_for<0, 256>([&](auto R) { asm volatile("v_accvgpr_write_b32 a%c0, 0" : : "i"(R.value)); });

  // LDS byte offset of this lane's chunk 4 kg + j of row l31 (the rows of a fragment are 32 mf + l31: the same swizzle bits)
  const int sw = XStage::swz(l31);
  int xrd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xrd[j] = l31 * 128 + XStage::chunk_off(4 * kg + j, sw);

  // one K-step on register set S = t % 3
  auto step = [&](int t, auto set) {
    constexpr int S = decltype(set)::value;
    constexpr int S2 = (S + 2) % WO_NS;
    wait_set(set, std::integral_constant<int, NREQ>{});
    __builtin_amdgcn_s_barrier();  // stage t has landed for every wave, and every wave has left stage t - 1 = (t + 2) % 3
    {
      const int kn = t + 2 > nk - 1 ? nk - 1 : t + 2;  // past the end: the last step again (valid memory), into a stage nobody reads
      issue_w(kn, std::integral_constant<int, S2>{});
      issue_x(kn, S2);
    }
    if (t == nk - 1 && tail_chunks < 8) {  // zero codes at k >= K
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * kg + j >= tail_chunks) {
            if constexpr (FP4) W[S][nf][0][j] = 0u;
            else { W[S][nf][j >> 1][2 * (j & 1)] = 0u; W[S][nf][j >> 1][2 * (j & 1) + 1] = 0u; }
          }
    }
    const char* const stage = smem + S * WO_STAGE;
    const float sc[2] = {wo_scale((int)SB[S][0]), wo_scale((int)SB[S][1])};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wo_bf16x8 xb[8], wa[2];
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) xb[mf] = *reinterpret_cast<const wo_bf16x8*>(stage + mf * 4096 + xrd[j]);
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        if constexpr (FP4) wa[nf] = wo_cvt_fp4(W[S][nf][0][j], sc[nf]);
        else wa[nf] = wo_cvt_fp8(W[S][nf][j >> 1][2 * (j & 1)], W[S][nf][j >> 1][2 * (j & 1) + 1], sc[nf]);
      }
      // s_nop 1 in front of every MFMA: whatever the compiler places between two statements (a conversion, a read's wait), the
      // operands are two wait states old; it issues in the shadow of the previous MFMA
      wo_static_for<0, 16>([&wa, &xb](auto J) {
        constexpr int nf = J.value >> 3, mf = J.value & 7;
        asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 a[%c2:%c2+15], %0, %1, a[%c2:%c2+15]" : : "v"(wa[nf]), "v"(xb[mf]), "i"(16 * J.value));
      });
    }
  };

  // prologue: the requests of steps 0 and 1
  issue_w(0, std::integral_constant<int, 0>{});
  issue_x(0, 0);
  issue_w(nk > 1 ? 1 : 0, std::integral_constant<int, 1>{});
  issue_x(nk > 1 ? 1 : 0, 1);
  for (int t = 0; t < nk; t += 3) {
    step(t, std::integral_constant<int, 0>{});
    if (t + 1 >= nk) break;
    step(t + 1, std::integral_constant<int, 1>{});
    if (t + 2 >= nk) break;
    step(t + 2, std::integral_constant<int, 2>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests past the end
#undef WO_LOAD16
#undef WO_LOAD1

  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the last MFMAs' results: nothing may read them early
  // the frame's C/D map (tile256_frame.hpp) with eight row blocks per wave, walked at compile time because the accumulators have
  // literal names: register r = 4 rq + e of accumulator 8 nf + mf is y[m0 + 32 mf + l31][n0 + 64 wave + 32 nf + 8 rq + 4 kg + e]
  wo_static_for<0, 8>([&](auto Q) {
    constexpr int nf = Q.value >> 2, rq = Q.value & 3;
    const int64_t nb = n0 + wave * 64 + nf * 32 + 8 * rq + 4 * kg;
    const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
    wo_static_for<0, 8>([&](auto MF) {
      constexpr int mf = MF.value, r0 = 16 * (8 * nf + mf) + 4 * rq;
      const float v[4] = {wo_acc_read<r0>() + bq.b[0], wo_acc_read<r0 + 1>() + bq.b[1], wo_acc_read<r0 + 2>() + bq.b[2],
                          wo_acc_read<r0 + 3>() + bq.b[3]};
      const int64_t m = m0 + mf * 32 + l31;
      if (m < M && nb < N) store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
    });
  });
}

template <int WF>
int wo_gemv_launch(const uint16_t* x, const uint8_t* wq, const uint8_t* ws, const void* bias, void* y, int ydtype, int64_t M, int64_t N,
                   int64_t K, int64_t Kp, int y_vec_ok, inc_stream_t stream) {
  const unsigned grid = (unsigned)ceil_div64(N, STRIP);
  if (ydtype == INC_BF16)
    mx_wo_gemv_kernel<true, WF><<<grid, VW * 64, 0, inc_s(stream)>>>(x, wq, ws, (const uint16_t*)bias, (uint16_t*)y, (int)M, N, K, Kp, y_vec_ok);
  else
    mx_wo_gemv_kernel<false, WF><<<grid, VW * 64, 0, inc_s(stream)>>>(x, wq, ws, (const uint16_t*)bias, (uint16_t*)y, (int)M, N, K, Kp, y_vec_ok);
  INC_LAUNCH_RETURN();
}

template <int WF>
int wo_gemm_launch(const uint16_t* x, const uint8_t* wq, const uint8_t* ws, const void* bias, void* y, int ydtype, int64_t M, int64_t N,
                   int64_t K, int64_t Kp, int y_vec_ok, inc_stream_t stream) {
  constexpr int smem = WO_NS * WO_STAGE;  // 96 KiB
  static std::atomic<uint64_t> attr_set{0};
  if (inc_attr_needed(attr_set)) {
    (void)hipFuncSetAttribute((const void*)mx_wo_gemm_kernel<true, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    (void)hipFuncSetAttribute((const void*)mx_wo_gemm_kernel<false, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    inc_attr_done(attr_set);
  }
  const unsigned grid = (unsigned)(ceil_div64(M, WO_TM) * ceil_div64(N, WO_TN));
  if (ydtype == INC_BF16)
    mx_wo_gemm_kernel<true, WF><<<grid, WO_THREADS, smem, inc_s(stream)>>>(x, wq, ws, (const uint16_t*)bias, (uint16_t*)y, M, N, K, Kp, y_vec_ok);
  else
    mx_wo_gemm_kernel<false, WF><<<grid, WO_THREADS, smem, inc_s(stream)>>>(x, wq, ws, (const uint16_t*)bias, (uint16_t*)y, M, N, K, Kp, y_vec_ok);
  INC_LAUNCH_RETURN();
}

// the checks both entry points share, in the order of the header's text; nothing is launched unless all pass
int wo_check(const void* x, const uint8_t* wq, const uint8_t* ws, int wfmt, const void* y, int ydtype, int64_t M, int64_t N, int64_t K,
             int64_t Kp, int64_t max_m) {
  INC_CHECK_ARG(x && wq && ws && y && M > 0 && N > 0 && K > 0 && Kp > 0);
  if (max_m && M > max_m) return INC_ERR_UNSUPPORTED;
  if (ydtype != INC_BF16 && ydtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0 || (K % 8) != 0 || K > Kp || Kp - K >= XK) return INC_ERR_UNSUPPORTED;
  if (wfmt != INC_MX_FP8_E4M3 && wfmt != INC_MX_FP4_E2M1) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 3) == 0);
  return INC_OK;
}

}  // namespace

extern "C" int inc_mx_wo_gemv(const void* x, const uint8_t* wq, const uint8_t* ws, int wfmt, const void* bias, void* y, int ydtype,
                              int64_t M, int64_t N, int64_t K, int64_t Kp, inc_stream_t stream) {
  const int rc = wo_check(x, wq, ws, wfmt, y, ydtype, M, N, K, Kp, INC_MX_GEMV_MAX_M);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG(ceil_div64(N, STRIP) < ((int64_t)1 << 31));
  const int y_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  const uint16_t* xb = static_cast<const uint16_t*>(x);
  if (wfmt == INC_MX_FP4_E2M1) return wo_gemv_launch<INC_MX_FP4_E2M1>(xb, wq, ws, bias, y, ydtype, M, N, K, Kp, y_vec_ok, stream);
  return wo_gemv_launch<INC_MX_FP8_E4M3>(xb, wq, ws, bias, y, ydtype, M, N, K, Kp, y_vec_ok, stream);
}

extern "C" int inc_mx_wo_gemm(const void* x, const uint8_t* wq, const uint8_t* ws, int wfmt, const void* bias, void* y, int ydtype,
                              int64_t M, int64_t N, int64_t K, int64_t Kp, inc_stream_t stream) {
  const int rc = wo_check(x, wq, ws, wfmt, y, ydtype, M, N, K, Kp, 0);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG((int64_t)WO_TM * Kp * 2 < ((int64_t)1 << 32));  // 32-bit request offsets inside a tile
  INC_CHECK_ARG(ceil_div64(M, WO_TM) * ceil_div64(N, WO_TN) < ((int64_t)1 << 31));
  const int y_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  const uint16_t* xb = static_cast<const uint16_t*>(x);
  if (wfmt == INC_MX_FP4_E2M1) return wo_gemm_launch<INC_MX_FP4_E2M1>(xb, wq, ws, bias, y, ydtype, M, N, K, Kp, y_vec_ok, stream);
  return wo_gemm_launch<INC_MX_FP8_E4M3>(xb, wq, ws, bias, y, ydtype, M, N, K, Kp, y_vec_ok, stream);
}
