// gemm_mx.hip -- K16: MXFP8 / MXFP4 GEMM on v_mfma_scale_f32_32x32x64_f8f6f4 (the block-scaled matrix instruction of gfx950).
//
//   y[m, n] = sum_blocks 2^(xs[m,b] + ws[n,b] - 254) * sum_{k in block b} x[m,k] * w[n,k]  +  bias[n]
//
// xq / wq are the e4m3 or e2m1 codes and xs / ws the E8M0 block scales of inc_mx_quant (include/inc_mi355x.h has the specification).
// The instruction dequantises inside the matrix pipe: a lane supplies 32 codes of one row and the scale byte of one of its blocks.
// Operand maps, pinned on the device with tools/mx_lab.hip (profiles/mx/mx_lab.log):
//   lane l holds row / column l & 31; h = l >> 5.  fp4: the 32 elements of block h of the 64-wide K step, element j in nibble j of
//   the first 4 dwords (element 2i in the low nibble of byte i -- the stored order; dwords 4 .. 7 are not read).  fp8: dwords 0 .. 3
//   are bytes 16 h .. 16 h + 15 and dwords 4 .. 7 bytes 32 + 16 h .. of the step (two back-to-back 8-bit MFMAs of K = 32), so a
//   block is spread over both lane halves.  For either format lane half h supplies the scale of block h of its row, in the byte of
//   the scale register that opsel names; C/D is the 32 x 32 map of every other 32x32 MFMA (tile256_frame.hpp).
//
// The kernel stands on the wave frame of tile256_frame.hpp (wave grid, operand roles, swizzled LDS image, C/D map) with a K-tile of 128
// elements: both operands are K-contiguous, so a tile is 256 rows of 128 bytes (fp8) or 64 bytes (fp4).  Two stages, the DMA of tile
// t+1 issued at the top of step t.
// Scales: a row has 4 scale bytes per K-tile, one dword.  Each lane loads the dwords of its 2 W rows and 4 x rows one step ahead
// (before that step's DMA is issued; they are first touched behind the barrier that ends the step, so no wait for them is placed in
// front of an MFMA), shifts them right by 8 * (l >> 5) once -- the two lane halves supply different blocks -- and the two 64-wide
// steps of a tile take bytes 0 and 2 of the result through opsel.
// One workgroup per tile and no split-K tail; M <= 16 has a kernel of its own (gemm_mx_gemv.hip), this one serves it with clamped rows.
// Algorithmic work per launch: 2*M*N*Kp flop; bytes (M + N) * Kp * (1 or 1/2) + (M + N) * Kp / 32 + 2*M*N.
#include "mx_stage.hpp"  // the frame's row stage issued as 1 KiB pieces, and the operand of the scaled MFMA read from it

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int XM = 256, XN = 256, XK = INC_MX_KTILE;

__host__ __device__ constexpr int mx_row_bytes(int fmt) { return fmt == INC_MX_FP8_E4M3 ? XK : XK / 2; }  // of one K-tile

template <bool IS_BF16, int XF, int WF>
__global__ __launch_bounds__(512) void mx_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                                      const uint8_t* __restrict__ wq, const uint8_t* __restrict__ ws,
                                                      const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t M,
                                                      int64_t N, int64_t Kp, int y_vec_ok) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using SX = MxStage<mx_row_bytes(XF)>;
  using SW = MxStage<mx_row_bytes(WF)>;
  constexpr int STAGE = SX::TILE + SW::TILE;
  const int tiles_n = (int)((N + XN - 1) / XN);
  const int tiles_m = (int)((M + XM - 1) / XM);
  const int tiles = tiles_m * tiles_n;
  const int wg = xcd_remap(blockIdx.x, tiles);
  int tm, tn;
  banded_tile_decode(wg, tiles_m, tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * XM, n0 = (int64_t)tn * XN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const int64_t ldx = XF == INC_MX_FP8_E4M3 ? Kp : Kp / 2, ldw = WF == INC_MX_FP8_E4M3 ? Kp : Kp / 2;
  const int64_t lds_ = Kp / 32;  // scale bytes per row

  uint32_t xoff[SX::NI], woff[SW::NI];
  SX::offsets(wave, lane, m0, M, ldx, xoff);
  SW::offsets(wave, lane, n0, N, ldw, woff);
  const uint8_t* const xtile = xq + m0 * ldx;
  const uint8_t* const wtile = wq + n0 * ldw;
  const int nk = (int)(Kp / XK);
  auto issue = [&](int kt, int stage) {
    kt = kt > nk - 1 ? nk - 1 : kt;
    SX::issue(xtile + (int64_t)kt * SX::CPR * 16, lds0 + stage * STAGE, wave, xoff);
    SW::issue(wtile + (int64_t)kt * SW::CPR * 16, lds0 + stage * STAGE + SX::TILE, wave, woff);
  };

  const int hi = lane >> 5;
  const int x_row = wm * 128 + (lane & 31);
  const int w_row = wn * 64 + (lane & 31);
  const int swx = SX::swz(lane & 31), sww = SW::swz(lane & 31);  // row bases are multiples of 32: the swizzle bits are the lane's

  // scale dwords of this lane's rows (clamped like the DMA rows), one per K-tile
  const uint32_t* xsp[4];
  const uint32_t* wsp[2];
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
    int64_t r = m0 + x_row + 32 * mf;
    if (r > M - 1) r = M - 1;
    xsp[mf] = reinterpret_cast<const uint32_t*>(xs + r * lds_);
  }
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    int64_t r = n0 + w_row + 32 * nf;
    if (r > N - 1) r = N - 1;
    wsp[nf] = reinterpret_cast<const uint32_t*>(ws + r * lds_);
  }
  uint32_t sxn[4], swn[2];
  int sxh[4], swh[2];  // this step's scale dwords, already shifted to the lane half's bytes
  auto load_scales = [&](int kt, uint32_t (&sx)[4], uint32_t (&sw)[2]) {
    kt = kt > nk - 1 ? nk - 1 : kt;
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) sx[mf] = xsp[mf][kt];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) sw[nf] = wsp[nf][kt];
  };

  f32x16 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  load_scales(0, sxn, swn);
  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  auto take_scales = [&]() {  // an ALU result on every path into the loop: no wait for a load is ever placed in front of an MFMA
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) sxh[mf] = (int)(sxn[mf] >> (8 * hi));
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) swh[nf] = (int)(swn[nf] >> (8 * hi));
  };
  take_scales();

#define MX_SB() __builtin_amdgcn_sched_barrier(0)
  for (int t = 0; t < nk; ++t) {
    const char* S = smem + (t & 1) * STAGE;
    load_scales(t + 1, sxn, swn);  // ahead of the DMA: in order behind nothing that is still in flight
    issue(t + 1, (t + 1) & 1);     // the other stage was last read in step t-1, which every wave left through the barrier
    i32x8 xa[2][4], wa[2][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) xa[kk][mf] = SX::frag(S, x_row + 32 * mf, kk, hi, swx);
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) wa[kk][nf] = SW::frag(S + SX::TILE, w_row + 32 * nf, kk, hi, sww);
    }
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
        acc[nf][mf] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa[0][nf], xa[0][mf], acc[nf][mf], WF, XF, 0, swh[nf], 0, sxh[mf]);
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
        acc[nf][mf] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa[1][nf], xa[1][mf], acc[nf][mf], WF, XF, 2, swh[nf], 2, sxh[mf]);
    // the two scheduling fences keep every use of sxn / swn (and so the wait for them, which would also wait for this step's DMA)
    // behind the MFMAs, and the MFMAs with the waits for their LDS reads in front of the barrier that frees this stage
    MX_SB();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 and its scales have landed (this wave's share; the barrier covers the rest)
    __builtin_amdgcn_s_barrier();
    MX_SB();
    take_scales();
  }
#undef MX_SB

  // the frame's C/D walk and its 8-byte store, written out: with this text the kernel's machine code is the parent's, byte for byte;
  // through tile256_walk or store_quad16 the epilogue grew by 160 instructions and every launch measured 0.1 - 1 % slower
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int64_t nb = n0 + wn * 64 + nf * 32 + 8 * rq + 4 * (lane >> 5);
      const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
      const float (&bv)[4] = bq.b;
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) {
        const int64_t m = m0 + wm * 128 + mf * 32 + (lane & 31);
        if (m >= M) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[nf][mf][4 * rq + e] + bv[e];
        uint16_t* dst = y + m * N + nb;
        if (y_vec_ok && nb + 4 <= N) {
          *reinterpret_cast<uint2*>(dst) = make_uint2(cvt_pair<IS_BF16>(v[0], v[1]), cvt_pair<IS_BF16>(v[2], v[3]));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (nb + e < N) dst[e] = IS_BF16 ? f32_to_bf16_bits(v[e]) : f32_to_f16_bits(v[e]);
        }
      }
    }
  }
}

template <int XF, int WF>
int mx_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws, const void* bias, void* y, int ydtype,
              int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  const size_t smem = (size_t)2 * 256 * (mx_row_bytes(XF) + mx_row_bytes(WF));  // 128 / 96 / 64 KiB
  static std::atomic<uint64_t> attr_set{0};
  if (inc_attr_needed(attr_set)) {
    (void)hipFuncSetAttribute((const void*)mx_gemm_kernel<true, XF, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    (void)hipFuncSetAttribute((const void*)mx_gemm_kernel<false, XF, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    inc_attr_done(attr_set);
  }
  const unsigned grid = (unsigned)(ceil_div64(M, XM) * ceil_div64(N, XN));
  const int y_vec_ok = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  if (ydtype == INC_BF16)
    mx_gemm_kernel<true, XF, WF><<<grid, 512, smem, inc_s(stream)>>>(xq, xs, wq, ws, (const uint16_t*)bias, (uint16_t*)y, M, N, Kp, y_vec_ok);
  else
    mx_gemm_kernel<false, XF, WF><<<grid, 512, smem, inc_s(stream)>>>(xq, xs, wq, ws, (const uint16_t*)bias, (uint16_t*)y, M, N, Kp, y_vec_ok);
  INC_LAUNCH_RETURN();
}

}  // namespace

extern "C" int inc_mx_gemm(const uint8_t* xq, const uint8_t* xs, int xfmt, const uint8_t* wq, const uint8_t* ws, int wfmt,
                           const void* bias, void* y, int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream) {
  INC_CHECK_ARG(xq && xs && wq && ws && y && M > 0 && N > 0 && Kp > 0);
  if (ydtype != INC_BF16 && ydtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if ((Kp % XK) != 0) return INC_ERR_UNSUPPORTED;
  const bool p88 = xfmt == INC_MX_FP8_E4M3 && wfmt == INC_MX_FP8_E4M3;
  const bool p84 = xfmt == INC_MX_FP8_E4M3 && wfmt == INC_MX_FP4_E2M1;
  const bool p44 = xfmt == INC_MX_FP4_E2M1 && wfmt == INC_MX_FP4_E2M1;
  if (!p88 && !p84 && !p44) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0);
  INC_CHECK_ARG(((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(ws)) & 3) == 0);
  INC_CHECK_ARG((int64_t)XM * Kp < ((int64_t)1 << 32));          // 32-bit DMA offsets inside a tile
  INC_CHECK_ARG(ceil_div64(M, XM) * ceil_div64(N, XN) < ((int64_t)1 << 31));
  if (p88) return mx_launch<INC_MX_FP8_E4M3, INC_MX_FP8_E4M3>(xq, xs, wq, ws, bias, y, ydtype, M, N, Kp, stream);
  if (p84) return mx_launch<INC_MX_FP8_E4M3, INC_MX_FP4_E2M1>(xq, xs, wq, ws, bias, y, ydtype, M, N, Kp, stream);
  return mx_launch<INC_MX_FP4_E2M1, INC_MX_FP4_E2M1>(xq, xs, wq, ws, bias, y, ydtype, M, N, Kp, stream);
}
