// gemm_tile256.hip -- the 256 x 256 x 64 kernels of the fused dequant-GEMM that stage the dequantised weights in LDS: the two-stage
// "big" kernel, "3A2B" (three x stages + two W stages, 4- and 8-bit) and, in the harness build, the producer / consumer kernel -- and the
// slab reduce that ends every split-K launch of a 256-row kernel.  (gemm_d2r.hip took over the large-M 4-bit path from them.)
#include "gemm_common.hpp"
#include "tile256_frame.hpp"

namespace {

// =============================================================================================
// large-M fast path (4-bit, K % 64 == 0, group_size % 32 == 0): 256x256x64 workgroup tile
// =============================================================================================
// The wave frame of tile256_frame.hpp with 32x32x16 MFMAs and a K-tile of 64 elements; one workgroup per CU (128 KiB LDS, two stages):
//   x tile      the frame's swizzled row stage (XStage: 256 rows x 128 B by LDS-DMA).
//   W tile      each thread fetches 4 packed words (4 packed rows of ONE column: the wave reads 256
//               contiguous bytes per row), dequantises them once for the whole workgroup and writes
//               the 4 x 16 B in MFMA-fragment order [n-frag][k16][lane] -> both the ds_write_b128 and
//               the ds_read_b128 are lane-linear (conflict-free).
using XStage = RowStage<TK * 2>;  // the x tile of every kernel of this file

// ABL != 0: timing-only ablations for tools/kbench (results are WRONG): 1 = no dequant arithmetic, 2 = x fragments read
// once per K-step, 3 = no global traffic inside the K-loop, 4 = no MFMA
template <bool IS_BF16, int ABL = 0>
__global__ __launch_bounds__(512) void woq_gemm_w4_big_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight,
    const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t M, int64_t N, int64_t K,
    int64_t NW, int g_shift, int y_vec_ok) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Abase = smem;                 // 2 stages
  char* const Bbase = smem + 2 * T_ASTAGE;  // 2 stages

  const int tiles_n = (int)((N + TN - 1) / TN);
  const int tiles_m = (int)((M + TM - 1) / TM);
  const int nwg = tiles_m * tiles_n;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
  const int64_t m0 = (int64_t)tm * TM, n0 = (int64_t)tn * TN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inv_u = fp8_unit_inverse();
  const int wm = wave >> 2, wn = wave & 3;

  // ---- x staging (LDS-DMA) ----------------------------------------------------------------------
  uint32_t avoff[4];  // byte offset of this lane's 16-byte chunk from x + m0*K + kt*TK
  XStage::offsets(wave, lane, m0, M, 2 * K, avoff);
  const uint16_t* const xtile = x + m0 * K;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;  // LDS byte address of the dynamic segment (low half of the flat address)
  // ---- W staging: this thread's column and packed-row half ---------------------------------------
  const int bcol = tid & 255, kwh = tid >> 8;
  int64_t ncol = n0 + bcol;
  if (ncol > N - 1) ncol = N - 1;
  const uint32_t* wsrc = qweight + (int64_t)(4 * kwh) * N + ncol;
  const int zshift = 4 * (int)(ncol & 7);
  const int64_t zcol = ncol >> 3;
  // LDS slot of word j: [nf = bcol>>5][kk = 2*kwh + (j>>1)][lane' = (bcol&31) + 32*(j&1)]
  const int bdst0 = (((bcol >> 5) * 4 + 2 * kwh) * 64 + (bcol & 31)) * 16;

  // this thread's share of the NEXT W tile, still packed (registers): 4 words + scale + zero word
  uint32_t raw[4], zw;
  uint16_t scb;
  const int voff = (4 * kwh) * (int)N + (int)ncol;  // element offset inside a K-tile of qweight (fits 32 bits)
  auto load_w = [&](int kt) {
    const uint32_t* tile = qweight + (int64_t)kt * (TK / 8) * N;  // wave-uniform base
#pragma unroll
    for (int j = 0; j < 4; ++j) raw[j] = tile[voff + j * (int)N];
    const int64_t g = g_shift >= 0 ? (((int64_t)kt * TK + 32 * kwh) >> g_shift) : 0;
    scb = scales[g * N + ncol];
    zw = qzeros[g * NW + zcol];
  };
  auto stash_regs = [&](int stage, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint16_t sb, uint32_t zword) {
    const float sc0 = f16_bits_to_f32(sb);
    uint32_t zz = ((zword >> zshift) & 15u) + 1u;  // modules.py:407-410 (stored zp-1; wraps above 15)
    zz = zz > 15u ? 0u : zz;
    const float nzs = -(float)zz * sc0;
    const float sc = sc0 * inv_u;
    char* dst = Bbase + stage * T_BSTAGE + bdst0;
    if constexpr (ABL == 1) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(w0, w1, w2, w3);
      *reinterpret_cast<uint4*>(dst + 32 * 16) = make_uint4(w1, w2, w3, w0);
      *reinterpret_cast<uint4*>(dst + 64 * 16) = make_uint4(w2, w3, w0, w1);
      *reinterpret_cast<uint4*>(dst + (64 + 32) * 16) = make_uint4(w3, w0, w1, __float_as_uint(nzs));
      return;
    }
    *reinterpret_cast<uint4*>(dst) = dequant8<IS_BF16>(w0, sc, nzs);                    // kk = 2*kwh,   k-octet 0
    *reinterpret_cast<uint4*>(dst + 32 * 16) = dequant8<IS_BF16>(w1, sc, nzs);          //               k-octet 1
    *reinterpret_cast<uint4*>(dst + 64 * 16) = dequant8<IS_BF16>(w2, sc, nzs);          // kk = 2*kwh+1, k-octet 0
    *reinterpret_cast<uint4*>(dst + (64 + 32) * 16) = dequant8<IS_BF16>(w3, sc, nzs);   //               k-octet 1
  };
  auto stash_w = [&](int stage) { stash_regs(stage, raw[0], raw[1], raw[2], raw[3], scb, zw); };
  auto dma_x = [&](int kt, int stage) {
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + stage * T_ASTAGE + wave * 4096);
    lds_dma_4x1k(xtile + (int64_t)kt * TK, dst, avoff[0], avoff[1], avoff[2], avoff[3]);
  };
  // makes the compiler's own wait for the packed-W registers happen HERE (before the next DMA is
  // issued): its s_waitcnt accounting does not see the DMA and would otherwise drain it later
  auto settle_w = [&]() {
    asm volatile("" : "+v"(raw[0]), "+v"(raw[1]), "+v"(raw[2]), "+v"(raw[3]), "+v"(zw));
    uint32_t t = scb;
    asm volatile("" : "+v"(t));
    scb = (uint16_t)t;
  };

  f32x16 acc[2][4];  // [n-frag][m-frag]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // fragment read offsets
  const int a_row = wm * 128 + (lane & 31);         // + 32*mf
  const int a_sw = XStage::swz(lane & 31);
  const int a_hi = lane >> 5;                        // chunk = 2*kk + a_hi
  const int b_off = (wn * 2 * 4 * 64 + lane) * 16;   // + (nf*4 + kk) * 1024

  uint4 xa_keep[4];
  auto mma_step = [&](const char* As, const char* Bs, int kk) {
    uint4 xa[4], wb[2];
    const int chunk = XStage::chunk_off(2 * kk + a_hi, a_sw);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      if (ABL == 2 && kk != 0) xa[mf] = xa_keep[mf];
      else xa[mf] = *reinterpret_cast<const uint4*>(As + (a_row + 32 * mf) * 128 + chunk);
      if (ABL == 2 && kk == 0) xa_keep[mf] = xa[mf];
    }
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) wb[nf] = *reinterpret_cast<const uint4*>(Bs + (nf * 4 + kk) * 1024);
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) {
        if constexpr (ABL == 4) {
          acc[nf][mf][0] += __uint_as_float(wb[nf].x ^ xa[mf].y);  // keeps the fragment reads alive without the matrix pipe
        } else {
          acc[nf][mf] = mfma32<IS_BF16>(wb[nf], xa[mf], acc[nf][mf]);
        }
      }
  };

  // Two-stage pipeline, one barrier per K-tile.  In iteration kt the LDS-DMA of x tile kt+1 and the
  // packed loads of W tile kt+2 are issued first and land under the 32 MFMAs; the dequantisation of W
  // tile kt+1 (registers -> other LDS stage) sits between the first and second MFMA group so that
  // its VALU work shares the issue slots the matrix pipe leaves free.  vmcnt(0) only at the barrier.
  const int nk = (int)(K / TK);
  dma_x(0, 0);
  load_w(0);
  stash_w(0);
  load_w(nk > 1 ? 1 : 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < nk - 1; ++kt) {
    const int cur = kt & 1;
    const char* As = Abase + cur * T_ASTAGE;
    const char* Bs = Bbase + cur * T_BSTAGE + b_off;
    settle_w();
    if (ABL != 3) dma_x(kt + 1, cur ^ 1);
    const uint32_t r0 = raw[0], r1 = raw[1], r2 = raw[2], r3 = raw[3], zcur = zw;
    const uint16_t scur = scb;
    if (ABL != 3) load_w(kt + 2 < nk ? kt + 2 : nk - 1);   // in flight for the whole K-step
    __builtin_amdgcn_sched_barrier(0);        // keep the loads up here (hipcc would sink them to their use)
    if constexpr (ABL == 5 || ABL == 6) {
      // one packed word per k16 group: ~19 VALU + 1 ds_write next to each group of 8 MFMAs instead of 76 VALU next to
      // the first group (the matrix pipe starves while a wave issues a long VALU run: both waves of a SIMD are in the
      // same phase, profiles/r1_pmc ablation)
      const float sc0 = f16_bits_to_f32(scur);
      uint32_t zz = ((zcur >> zshift) & 15u) + 1u;
      zz = zz > 15u ? 0u : zz;
      const float nzs = -(float)zz * sc0;
      const float sc = sc0 * inv_u;
      char* dst = Bbase + (cur ^ 1) * T_BSTAGE + bdst0;
      const uint32_t rw[4] = {r0, r1, r2, r3};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        mma_step(As, Bs, kk);
        *reinterpret_cast<uint4*>(dst + ((kk >> 1) * 64 + 32 * (kk & 1)) * 16) = dequant8<IS_BF16>(rw[kk], sc, nzs);
        if constexpr (ABL == 6) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);  // 3 VALU
          }
        }
      }
    } else {
    mma_step(As, Bs, 0);
    stash_regs(cur ^ 1, r0, r1, r2, r3, scur, zcur);
    mma_step(As, Bs, 1);
    mma_step(As, Bs, 2);
    mma_step(As, Bs, 3);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  {
    const int cur = (nk - 1) & 1;
    const char* As = Abase + cur * T_ASTAGE;
    const char* Bs = Bbase + cur * T_BSTAGE + b_off;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) mma_step(As, Bs, kk);
  }

  tile256_walk(
      m0, n0, wm, wn, lane, [&](int64_t nb) { return load_bias_quad<IS_BF16>(bias, nb, N); },
      [&](int nf, int mf, int rq, int64_t m, int64_t nb, const BiasQuad& bq) {
        if (m >= M) return;
        const float v[4] = {acc[nf][mf][4 * rq + 0] + bq.b[0], acc[nf][mf][4 * rq + 1] + bq.b[1], acc[nf][mf][4 * rq + 2] + bq.b[2],
                            acc[nf][mf][4 * rq + 3] + bq.b[3]};
        store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
      });
}

// =============================================================================================
// large-M path "3A2B" (4-bit, K % 128 == 0): 256x256x64 tile, THREE x stages + TWO W stages = all 160 KiB of LDS
// =============================================================================================
// Ablations (tools/kbench ablate, profiles/r1f): with two stages the DMA of x tile t+1 is issued at the start of step t
// and must have landed at its end, so a step can never be shorter than one loaded HBM/L2 round trip (~1.4 us measured
// against ~0.9 us of MFMA work) -- removing the global traffic alone gives +15-25 %, a deeper pipeline with shorter steps
// does not help because its loads still have only ~one round trip to land.  Here the x DMA runs TWO steps ahead (three 32
// KiB stages), the packed W words (8 KiB per step: registers are enough) also two steps ahead, and the dequantised W keeps
// its two 32 KiB stages: 3*32 + 2*32 = 160 KiB, exactly one CU's LDS.  All loop traffic is issued from asm and retired
// with counted waits: per step a wave issues 6 W requests then 4 DMAs; `vmcnt(14)` before the dequantisation leaves
// the previous step's 4 DMAs + this step's 10 requests in flight, `vmcnt(10)` before the barrier retires those 4 DMAs.
// The dequantisation is spread over the four k16 groups (one packed word next to each 8 MFMAs).
// SCHED selects the step's instruction schedule (same data flow, same results):
//   0  as written, the compiler orders the step (it sinks every fragment read to just before the MFMAs that use it and
//      so re-exposes the LDS latency four times per step -- see profiles/r1i)
//   1  sched_barrier fences pin the software pipeline: reads of k16 group g+1 are issued BEFORE the MFMAs of group g
//   3  "ping-pong": compute and load segments separated by barriers, partner waves half a step apart (see below)
//   10-16, 31-37  timing-only ablations (tools/kbench ablate)
// All of 0/1/3 give bit-identical outputs and, measured (profiles/r1i_kbench_*.log), the same speed within 10 %: the step is
// not bound by instruction placement -- a variant that spread the 10 VMEM requests between the carried group's MFMAs
// changed nothing either -- but by the sum of its parts.
#define INC_3A2B_DEFAULT_SCHED 1
// BITS = 8 (weight-only INT8, BASELINE config #1's packed layers): the same kernel with a 16 KiB packed W tile per step --
// a thread fetches 8 words (4 k each) of its column instead of 4 (8 k each), two words make one 16-byte fragment row, the
// integer -> float step is v_cvt_f32_ubyte*, a step has 14 VMEM requests instead of 10 (the counted waits follow).
template <bool IS_BF16, int SCHED, int BITS = 4>
__global__ __launch_bounds__(512) void woq_gemm_w4_3a2b_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight,
    const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t M, int64_t N, int64_t K,
    int64_t NW, int g_shift, int y_vec_ok, float* __restrict__ partial, int steps_per_split) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Abase = smem;                 // 3 stages
  char* const Bbase = smem + 3 * T_ASTAGE;  // 2 stages
  const int tiles_n = (int)((N + TN - 1) / TN);
  const int tiles_m = (int)((M + TM - 1) / TM);
  const int nwg = tiles_m * tiles_n;
  const int wg = xcd_remap(blockIdx.x, nwg);
  // row-major inside an XCD's range: a 2 x 16 strip shares the 32 KiB x tiles 16 ways and the 8 KiB W tiles 2 ways -- 192 KiB of
  // unique operand bytes per K-step for 32 tiles; the 8 x 4 patch of banded_tile_decode needs 288 KiB and measured 15 % slower
  const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
  const int64_t m0 = (int64_t)tm * TM, n0 = (int64_t)tn * TN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inv_u = fp8_unit_inverse();
  const int wm = wave >> 2, wn = wave & 3;
  // timing-only ablations (tools/kbench ablate; results are wrong by construction): which part of a step costs what
  // 30 + mask: the ping-pong schedule (3) minus {1: loads, 2: dequantisation + W writes, 4: fragment reads}
  constexpr bool PP = SCHED == 3 || SCHED >= 30;
  constexpr int PPM = SCHED >= 30 ? SCHED - 30 : 0;
  constexpr bool NO_DEQ = SCHED == 10 || SCHED == 15 || SCHED == 16 || (PPM & 2);  // no int4 -> bf16 arithmetic
  constexpr bool NO_WR = SCHED == 11 || SCHED == 15 || SCHED == 16 || (PPM & 2);   // no ds_write of the dequantised W
  constexpr bool NO_RD = SCHED == 12 || SCHED == 15 || SCHED == 16 || (PPM & 4);   // no fragment reads
  constexpr bool NO_LD = SCHED == 13 || SCHED == 15 || SCHED == 16 || (PPM & 1);   // no global loads / LDS-DMA
  constexpr bool NO_BAR = SCHED == 14 || SCHED == 16;                 // no per-step barrier
  constexpr bool NO_VMWAIT = SCHED == 17;                             // loads issued, their counted waits dropped
  constexpr bool FIXED_ADDR = SCHED == 18;                            // loads always fetch K-tile 0 (address arithmetic hoisted)
  constexpr bool NO_WLD = SCHED == 19;                                // x LDS-DMA kept, the 6 W-side loads dropped
  constexpr bool NO_DMA = SCHED == 20;                                // W-side loads kept, the 4 x LDS-DMAs dropped
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;

  uint32_t avoff[4];
  XStage::offsets(wave, lane, m0, M, 2 * K, avoff);
  const uint16_t* const xtile = x + m0 * K;
  const int bcol = tid & 255, kwh = tid >> 8;
  int64_t ncol = n0 + bcol;
  if (ncol > N - 1) ncol = N - 1;
  constexpr int NPK = 32 / BITS;       // codes per packed word: 8 / 4
  constexpr int NWD = 32 / NPK;        // words of one column per thread and step (32 k): 4 / 8
  uint32_t wvoff[8];
#pragma unroll
  for (int j = 0; j < NWD; ++j) wvoff[j] = (uint32_t)(((int64_t)(NWD * kwh + j) * N + ncol) * 4);
  const uint32_t svoff = (uint32_t)(ncol * 2), zvoff = (uint32_t)((ncol / NPK) * 4);
  const int zshift = BITS * (int)(ncol % NPK);
  const int bdst0 = (((bcol >> 5) * 4 + 2 * kwh) * 64 + (bcol & 31)) * 16;
  const int kwh_s = __builtin_amdgcn_readfirstlane(tid >> 8);
  // split-K (medium M: fewer tiles than CUs): this workgroup multiplies K-tiles [kbase, kbase + nk) and, when `partial`
  // is given, stores its fp32 tile into slab blockIdx.y; inc_woq_gemm's finalize kernel adds the slabs in a fixed order
  const int nk_all = (int)(K / TK);
  const int kbase = blockIdx.y * steps_per_split;
  const int nk = min(steps_per_split, nk_all - kbase);

  // one step's requests: 6 for W (4 packed words, scale, zero word) FIRST, then 4 x DMAs
  auto issue_w = [&](int kt, uint32_t (&w)[8], uint32_t& sb, uint32_t& zw) {
    if (NO_LD || NO_WLD) {
      asm volatile("" : "=v"(w[0]), "=v"(w[1]), "=v"(w[2]), "=v"(w[3]), "=v"(sb), "=v"(zw));
      return;
    }
    kt = FIXED_ADDR ? 0 : kbase + (kt > nk - 1 ? nk - 1 : kt);
    const uint32_t* wbase = qweight + (int64_t)kt * (TK / NPK) * N;
    const int64_t g = g_shift >= 0 ? (((int64_t)kt * TK + 32 * kwh_s) >> g_shift) : 0;  // wave-uniform (kwh is)
    const uint16_t* sbase = scales + g * N;
    const uint32_t* zbase = qzeros + g * NW;
    asm volatile(
        "s_nop 4\n\t"
        "global_load_dword %0, %6, %12\n\t"
        "global_load_dword %1, %7, %12\n\t"
        "global_load_dword %2, %8, %12\n\t"
        "global_load_dword %3, %9, %12\n\t"
        "global_load_ushort %4, %10, %13\n\t"
        "global_load_dword %5, %11, %14"
        : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(sb), "=&v"(zw)
        : "v"(wvoff[0]), "v"(wvoff[1]), "v"(wvoff[2]), "v"(wvoff[3]), "v"(svoff), "v"(zvoff), "s"(wbase), "s"(sbase), "s"(zbase)
        : "memory");
    if constexpr (BITS == 8)
      asm volatile(
          "global_load_dword %0, %4, %8\n\t"
          "global_load_dword %1, %5, %8\n\t"
          "global_load_dword %2, %6, %8\n\t"
          "global_load_dword %3, %7, %8"
          : "=&v"(w[4]), "=&v"(w[5]), "=&v"(w[6]), "=&v"(w[7])
          : "v"(wvoff[4]), "v"(wvoff[5]), "v"(wvoff[6]), "v"(wvoff[7]), "s"(wbase)
          : "memory");
  };
  auto issue_dma = [&](int kt, int astage) {
    if (NO_LD || NO_DMA) return;
    kt = FIXED_ADDR ? 0 : kbase + (kt > nk - 1 ? nk - 1 : kt);
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + astage * T_ASTAGE + wave * 4096);
    lds_dma_4x1k(xtile + (int64_t)kt * TK, dst, avoff[0], avoff[1], avoff[2], avoff[3]);
  };

  f32x16 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  const int a_row = wm * 128 + (lane & 31);
  const int a_sw = XStage::swz(lane & 31);
  const int a_hi = lane >> 5;
  const int b_off = (wn * 2 * 4 * 64 + lane) * 16;
  auto read_frags = [&](const char* As, const char* Bs, int kk, uint4 (&xa)[4], uint4 (&wbv)[2]) {
    const int chunk = XStage::chunk_off(2 * kk + a_hi, a_sw);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) xa[mf] = *reinterpret_cast<const uint4*>(As + (a_row + 32 * mf) * 128 + chunk);
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) wbv[nf] = *reinterpret_cast<const uint4*>(Bs + (nf * 4 + kk) * 1024);
  };
  auto mma8 = [&](const uint4 (&xa)[4], const uint4 (&wbv)[2]) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) acc[nf][mf] = mfma32<IS_BF16>(wbv[nf], xa[mf], acc[nf][mf]);
  };
  auto mma1 = [&](int i, const uint4 (&xa)[4], const uint4 (&wbv)[2]) {
    acc[i >> 2][i & 3] = mfma32<IS_BF16>(wbv[i >> 2], xa[i & 3], acc[i >> 2][i & 3]);
  };
#define INC_SB() __builtin_amdgcn_sched_barrier(0)
  // the kk-th 8-k fragment row of this thread's column: one 4-bit word, or two 8-bit words
  auto dequant_into = [&](int bstage, int kk, const uint32_t (&wd)[8], float sc, float nzs) {
    char* dst = Bbase + bstage * T_BSTAGE + bdst0;
    uint4 v;
    if constexpr (BITS == 4) {
      const uint32_t word = wd[kk];
      v = NO_DEQ ? make_uint4(word, word, word, word) : dequant8<IS_BF16>(word, sc, nzs);
    } else {
      v = dequant8_from_bytes<IS_BF16>(wd[2 * kk], wd[2 * kk + 1], sc, (int)nzs);  // 8-bit: `nzs` carries the zero point itself
    }
    if (NO_WR) asm volatile("" : : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
    else *reinterpret_cast<uint4*>(dst + ((kk >> 1) * 64 + 32 * (kk & 1)) * 16) = v;
  };
  auto group_params = [&](uint32_t sb, uint32_t zw, float& sc, float& nzs) {
    const float sc0 = f16_bits_to_f32((uint16_t)sb);
    constexpr uint32_t qmax = (1u << BITS) - 1u;
    uint32_t zz = ((zw >> zshift) & qmax) + 1u;  // modules.py:407-410
    zz = zz > qmax ? 0u : zz;
    nzs = BITS == 4 ? -(float)zz * sc0 : (float)zz;  // 8-bit: the zero point itself (the int8 wrap of q - z needs it as an integer)
    sc = BITS == 4 ? sc0 * inv_u : sc0;               // the 4-bit path converts through the fp8 decoder (q * 2^-9)
  };

  // ---- prologue: x stage 0 and W stage 0 complete; queue = [W words of tile 1 (6), DMA of x tile 1 (4)] ---------------
  uint32_t wa[8], wsa, wza;  // W register set A: tiles with ODD index (4-bit: entries 0..3 only)
  uint32_t wb_[8], wsb, wzb; // W register set B: tiles with EVEN index >= 2
  {
    uint32_t w0[8], s0, z0;
    issue_w(0, w0, s0, z0);
    issue_dma(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(w0[0]), "+v"(w0[1]), "+v"(w0[2]), "+v"(w0[3]), "+v"(s0), "+v"(z0) : : "memory");
    if constexpr (BITS == 8) asm volatile("" : "+v"(w0[4]), "+v"(w0[5]), "+v"(w0[6]), "+v"(w0[7]) : : "memory");
    float sc, nzs;
    group_params(s0, z0, sc, nzs);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) dequant_into(0, kk, w0, sc, nzs);
  }
  if (PP && wm) issue_w(1, wb_, wsb, wzb);  // the second half enters the loop one load segment later: sets swapped
  else issue_w(1, wa, wsa, wza);
  issue_dma(1, 1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // Fragment registers: X and Y alternate over the four k16 groups of a step.  The LAST group of step t is multiplied
  // AFTER the barrier that ends the step, while the first fragments of step t+1 are already on their way from LDS and the
  // next loads are being issued: the matrix pipe has work during what used to be a ~90-instruction bubble per step.
  uint4 xX[4], wX[2], xY[4], wY[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) xY[i] = make_uint4(0u, 0u, 0u, 0u);  // "previous step's last group" of step 0: adds zeros
  wY[0] = wY[1] = make_uint4(0u, 0u, 0u, 0u);
  read_frags(Abase, Bbase + b_off, 0, xX, wX);

  // step t: x stage t%3, W stage t&1.  Issues W words of tile t+2 and the DMA of x tile t+2 (stage (t+2)%3), dequantises
  // tile t+1 (words issued in step t-1) into W stage (t+1)&1.
  // SCHED 3 ("ping-pong"): a step is split into a compute segment (32 MFMAs + their 24 fragment reads) and a load segment
  // (10 VMEM requests, dequantisation, 4 LDS writes) with a barrier after each.  The waves of the second half (wm = 1:
  // wave w+4 shares a SIMD with wave w) run one extra load segment before the loop, so from then on one wave of every SIMD
  // computes while its partner loads -- the two instruction streams never compete for the matrix pipe and the VMEM/VALU
  // issue of one hides behind the MFMAs of the other.  Half-step h: wm 0 computes tile h/2 at even h, wm 1 at odd h.  To
  // keep every tile complete one half-step before its first reader, wm 1 works one tile further ahead in its load segment
  // (loads tile t+3, dequantises tile t+2); stage numbers become wave-uniform run-time values, the loop body is one code.
  // counted waits: a step issues NVM = NWD + 2 + 4 requests (W words, scale, zero word, 4 x DMAs); "words" retires the
  // W-side requests of the PREVIOUS step (that step's 4 DMAs and this step's NVM stay in flight), "tile" retires the
  // previous step's DMAs (this step's NVM stay in flight)
  auto wait_words = [&](uint32_t (&dw)[8], uint32_t& ds, uint32_t& dz) {
    if (NO_VMWAIT) asm volatile("" : "+v"(dw[0]), "+v"(dw[1]), "+v"(dw[2]), "+v"(dw[3]), "+v"(ds), "+v"(dz) : : "memory");
    else if constexpr (BITS == 4) asm volatile("s_waitcnt vmcnt(14)" : "+v"(dw[0]), "+v"(dw[1]), "+v"(dw[2]), "+v"(dw[3]), "+v"(ds), "+v"(dz) : : "memory");
    else asm volatile("s_waitcnt vmcnt(18)" : "+v"(dw[0]), "+v"(dw[1]), "+v"(dw[2]), "+v"(dw[3]), "+v"(ds), "+v"(dz) : : "memory");
    if constexpr (BITS == 8) asm volatile("" : "+v"(dw[4]), "+v"(dw[5]), "+v"(dw[6]), "+v"(dw[7]) : : "memory");
  };
  auto wait_tile = [&]() {
    if (NO_VMWAIT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else if constexpr (BITS == 4) asm volatile("s_waitcnt vmcnt(10)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(14)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
  };
#define INC_3A2B_COMPUTE(As, Bs)                                                                                   \
  {                                                                                                                \
    if (!NO_RD) read_frags(As, Bs, 0, xX, wX);                                                                                 \
    if (!NO_RD) read_frags(As, Bs, 1, xY, wY);                                                                                 \
    INC_SB();                                                                                                      \
    mma8(xX, wX);                                                                                                  \
    INC_SB();                                                                                                      \
    if (!NO_RD) read_frags(As, Bs, 2, xX, wX);                                                                                 \
    INC_SB();                                                                                                      \
    mma8(xY, wY);                                                                                                  \
    INC_SB();                                                                                                      \
    if (!NO_RD) read_frags(As, Bs, 3, xY, wY);                                                                                 \
    INC_SB();                                                                                                      \
    mma8(xX, wX);                                                                                                  \
    INC_SB();                                                                                                      \
    mma8(xY, wY);                                                                                                  \
    INC_SB();                                                                                                      \
  }
#define INC_3A2B_LOADSEG(T, LW, LWS, LWZ, DW, DWS, DWZ)                                                           \
  {                                                                                                                \
    issue_w((T) + 2, LW, LWS, LWZ);                                                                                \
    issue_dma((T) + 2, ((T) + 2) % 3);                                                                             \
    wait_words(DW, DWS, DWZ);                                                                                      \
    float sc_, nzs_;                                                                                               \
    group_params(DWS, DWZ, sc_, nzs_);                                                                             \
    dequant_into(((T) & 1) ^ 1, 0, DW, sc_, nzs_);                                                                 \
    dequant_into(((T) & 1) ^ 1, 1, DW, sc_, nzs_);                                                                 \
    dequant_into(((T) & 1) ^ 1, 2, DW, sc_, nzs_);                                                                 \
    dequant_into(((T) & 1) ^ 1, 3, DW, sc_, nzs_);                                                                 \
    INC_SB();                                                                                                      \
  }
#define INC_3A2B_STEP3(T, LW, LWS, LWZ, DW, DWS, DWZ)                                                              \
  {                                                                                                                \
    const int t_ = (T);                                                                                            \
    const char* As = Abase + (t_ % 3) * T_ASTAGE;                                                                  \
    const char* Bs = Bbase + (t_ & 1) * T_BSTAGE + b_off;                                                          \
    INC_3A2B_COMPUTE(As, Bs)                                                                                       \
    __builtin_amdgcn_s_barrier();                                                                                  \
    INC_SB(); /* keep the load segment's address arithmetic on its own side of the barrier */                     \
    INC_3A2B_LOADSEG(t_ + wm, LW, LWS, LWZ, DW, DWS, DWZ)                                                          \
    wait_tile();                                                                                                   \
    __builtin_amdgcn_s_barrier();                                                                                  \
  }
#define INC_3A2B_STEP(T, LW, LWS, LWZ, DW, DWS, DWZ)                                                              \
  {                                                                                                                \
    const int t_ = (T);                                                                                            \
    const int as_ = t_ % 3, bs_ = t_ & 1;                                                                          \
    const char* As = Abase + as_ * T_ASTAGE;                                                                       \
    const char* Bs = Bbase + bs_ * T_BSTAGE + b_off;                                                               \
    issue_w(t_ + 2, LW, LWS, LWZ);                                                                                 \
    issue_dma(t_ + 2, (t_ + 2) % 3);                                                                               \
    if (SCHED != 0) INC_SB();                                                                                      \
    mma8(xY, wY);                       /* group 3 of the previous step */                                         \
    if (SCHED != 0) INC_SB();                                                                                      \
    if (!NO_RD) read_frags(As, Bs, 1, xY, wY);                                                                               \
    if (SCHED != 0) INC_SB();                                                                                           \
    wait_words(DW, DWS, DWZ);                                                                                      \
    float sc_, nzs_;                                                                                               \
    group_params(DWS, DWZ, sc_, nzs_);                                                                             \
    if (SCHED != 0) dequant_into(bs_ ^ 1, 0, DW, sc_, nzs_);                                                         \
    mma8(xX, wX);                       /* group 0 */                                                              \
    if (SCHED == 0) dequant_into(bs_ ^ 1, 0, DW, sc_, nzs_);                                                        \
    if (SCHED != 0) INC_SB();                                                                                           \
    if (!NO_RD) read_frags(As, Bs, 2, xX, wX);                                                                                 \
    if (SCHED != 0) INC_SB();                                                                                           \
    if (SCHED != 0) dequant_into(bs_ ^ 1, 1, DW, sc_, nzs_);                                                         \
    mma8(xY, wY);                       /* group 1 */                                                              \
    if (SCHED == 0) dequant_into(bs_ ^ 1, 1, DW, sc_, nzs_);                                                        \
    if (SCHED != 0) INC_SB();                                                                                           \
    if (!NO_RD) read_frags(As, Bs, 3, xY, wY);                                                                                 \
    if (SCHED != 0) INC_SB();                                                                                           \
    if (SCHED != 0) { dequant_into(bs_ ^ 1, 2, DW, sc_, nzs_); dequant_into(bs_ ^ 1, 3, DW, sc_, nzs_); }         \
    mma8(xX, wX);                       /* group 2 */                                                              \
    if (SCHED == 0) { dequant_into(bs_ ^ 1, 2, DW, sc_, nzs_); dequant_into(bs_ ^ 1, 3, DW, sc_, nzs_); }        \
    if (SCHED != 0) INC_SB();                                                                                           \
    wait_tile();                                                                                                   \
    if (!NO_BAR) __builtin_amdgcn_s_barrier();                                                                                  \
    if (!NO_RD) read_frags(Abase + ((t_ + 1) % 3) * T_ASTAGE, Bbase + (bs_ ^ 1) * T_BSTAGE + b_off, 0, xX, wX);               \
    if (SCHED != 0) INC_SB();                                                                                           \
  }
  if (PP) {
    if (wm) {  // load segment "-1": tile 2 -> x stage 2 / set A, tile 1 (set B) -> W stage 1
      INC_3A2B_LOADSEG(0, wa, wsa, wza, wb_, wsb, wzb)
      wait_tile();
      __builtin_amdgcn_s_barrier();
    }
    for (int t0 = 0; t0 < nk; t0 += 2) {
      INC_3A2B_STEP3(t0, wb_, wsb, wzb, wa, wsa, wza)
      INC_3A2B_STEP3(t0 + 1, wa, wsa, wza, wb_, wsb, wzb)
    }
    if (!wm) __builtin_amdgcn_s_barrier();  // the first half has executed one barrier fewer
  } else {
    for (int t0 = 0; t0 < nk; t0 += 2) {
      INC_3A2B_STEP(t0, wb_, wsb, wzb, wa, wsa, wza)        // even step: load tile t+2 (even) -> set B, dequantise tile t+1 (odd) <- set A
      INC_3A2B_STEP(t0 + 1, wa, wsa, wza, wb_, wsb, wzb)    // odd step: the reverse
    }
    mma8(xY, wY);  // group 3 of the last step
  }
#undef INC_3A2B_STEP
#undef INC_3A2B_STEP3
#undef INC_3A2B_COMPUTE
#undef INC_3A2B_LOADSEG
#undef INC_SB
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  if (partial) {  // split-K: raw fp32 tile into this split's slab (bias and conversion happen in the finalize kernel).  The frame's walk
    // written out: through tile256_walk the compiler split the 16-byte store into 12 + 4 bytes and the slab launches lost 10-16 %
    float* slab = partial + (int64_t)blockIdx.y * M * N;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int64_t nb = n0 + wn * 64 + nf * 32 + 8 * rq + 4 * (lane >> 5);
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
          const int64_t m = m0 + wm * 128 + mf * 32 + (lane & 31);
          if (m >= M) continue;
          float* dst = slab + m * N + nb;
          if (nb + 4 <= N && (N % 4) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(acc[nf][mf][4 * rq + 0], acc[nf][mf][4 * rq + 1], acc[nf][mf][4 * rq + 2], acc[nf][mf][4 * rq + 3]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (nb + e < N) dst[e] = acc[nf][mf][4 * rq + e];
          }
        }
      }
    return;
  }
  // (written out like the slab store above: with tile256_walk here the 4-bit kernel took one more VGPR than it had)
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int64_t nb = n0 + wn * 64 + nf * 32 + 8 * rq + 4 * (lane >> 5);
      const BiasQuad bq = load_bias_quad<IS_BF16>(bias, nb, N);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) {
        const int64_t m = m0 + wm * 128 + mf * 32 + (lane & 31);
        if (m >= M) continue;
        const float v[4] = {acc[nf][mf][4 * rq + 0] + bq.b[0], acc[nf][mf][4 * rq + 1] + bq.b[1], acc[nf][mf][4 * rq + 2] + bq.b[2],
                            acc[nf][mf][4 * rq + 3] + bq.b[3]};
        store_quad16<IS_BF16>(y, m, nb, N, y_vec_ok, v);
      }
    }
  }
}

#ifdef INC_KBENCH  // superseded by the direct-to-register kernel (gemm_d2r.hip); kept in the harness build as its bitwise A/B partner (tools/kbench d2r)
#include "../../tools/kbench_gemm_1.inc"
#endif  // INC_KBENCH

template <bool IS_BF16>
__global__ void splitk_slab_reduce_kernel(const float* __restrict__ partial, const uint16_t* __restrict__ bias,
                                          uint16_t* __restrict__ y, int64_t M, int64_t N, int splits) {
  const int64_t total4 = M * N / 4;  // N % 4 == 0 on this path
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = reinterpret_cast<const float4*>(partial)[i];
    for (int z = 1; z < splits; ++z) {  // fixed order: deterministic
      const float4 p = reinterpret_cast<const float4*>(partial + (int64_t)z * M * N)[i];
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    if (bias) {
      const int64_t n = (i * 4) % N;
      v.x += cvt16<IS_BF16>(bias[n]); v.y += cvt16<IS_BF16>(bias[n + 1]); v.z += cvt16<IS_BF16>(bias[n + 2]); v.w += cvt16<IS_BF16>(bias[n + 3]);
    }
    reinterpret_cast<uint2*>(y)[i] = make_uint2(cvt_pair<IS_BF16>(v.x, v.y), cvt_pair<IS_BF16>(v.z, v.w));
  }
}

}  // namespace

// sum of the split-K slabs (+ bias) -> y: the second launch of every 256-row kernel that ran with slabs
int inc_launch_slab_reduce(const WoqGemmArgs& a, const float* part, int splits) {
  int64_t rb = ceil_div64(a.M * a.N / 4, 256);
  if (rb > 4096) rb = 4096;
  if (a.bf) splitk_slab_reduce_kernel<true><<<(unsigned)rb, 256, 0, a.s>>>(part, a.bias, a.y, a.M, a.N, splits);
  else splitk_slab_reduce_kernel<false><<<(unsigned)rb, 256, 0, a.s>>>(part, a.bias, a.y, a.M, a.N, splits);
  INC_LAUNCH_RETURN();
}

int inc_launch_woq_gemm_big(const WoqGemmArgs& a, int y_vec_ok) {
  const size_t smem = (size_t)2 * T_ASTAGE + 2 * T_BSTAGE;  // 128 KiB
  static std::atomic<uint64_t> big_attr_set{0};
  if (inc_attr_needed(big_attr_set)) {
    (void)hipFuncSetAttribute((const void*)woq_gemm_w4_big_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    (void)hipFuncSetAttribute((const void*)woq_gemm_w4_big_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    inc_attr_done(big_attr_set);
  }
  const unsigned grid = (unsigned)(ceil_div64(a.M, TM) * ceil_div64(a.N, TN));
  if (a.bf) woq_gemm_w4_big_kernel<true><<<grid, 512, smem, a.s>>>(a.x, a.qw, a.scales, a.qz, a.bias, a.y, a.M, a.N, a.K, a.NW, a.g_shift, y_vec_ok);
  else woq_gemm_w4_big_kernel<false><<<grid, 512, smem, a.s>>>(a.x, a.qw, a.scales, a.qz, a.bias, a.y, a.M, a.N, a.K, a.NW, a.g_shift, y_vec_ok);
  INC_LAUNCH_RETURN();
}

// `part`: the fp32 slabs of a split-K launch (then reduced here), or NULL
int inc_launch_woq_gemm_3a2b(const WoqGemmArgs& a, int bits, int y_vec_ok, float* part, int steps, int splits, int dbg) {
  const size_t smem = (size_t)3 * T_ASTAGE + 2 * T_BSTAGE;  // 160 KiB: the whole LDS of a CU
  static std::atomic<uint64_t> a3_attr_set{0};
  if (inc_attr_needed(a3_attr_set)) {
#define INC_A3_ATTR(...) (void)hipFuncSetAttribute((const void*)woq_gemm_w4_3a2b_kernel<__VA_ARGS__>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)
    INC_A3_ATTR(true, INC_3A2B_DEFAULT_SCHED); INC_A3_ATTR(false, INC_3A2B_DEFAULT_SCHED);
    INC_A3_ATTR(true, INC_3A2B_DEFAULT_SCHED, 8); INC_A3_ATTR(false, INC_3A2B_DEFAULT_SCHED, 8);
    inc_attr_done(a3_attr_set);
  }
  const unsigned grid = (unsigned)(ceil_div64(a.M, TM) * ceil_div64(a.N, TN));
  dim3 g2(grid, (unsigned)splits);
#define INC_A3(...) woq_gemm_w4_3a2b_kernel<__VA_ARGS__><<<g2, 512, smem, a.s>>>(a.x, a.qw, a.scales, a.qz, a.bias, a.y, a.M, a.N, a.K, a.NW, a.g_shift, y_vec_ok, part, steps)
  if (bits == 8) { if (a.bf) INC_A3(true, INC_3A2B_DEFAULT_SCHED, 8); else INC_A3(false, INC_3A2B_DEFAULT_SCHED, 8); }
  else if (!a.bf) INC_A3(false, INC_3A2B_DEFAULT_SCHED);
#ifdef INC_KBENCH
#define INC_A3H(S) { INC_A3_ATTR(true, S); INC_A3(true, S); }
  // harness build: flag 4 / 6 time the other schedules of the bf16 kernel, 20..37 its timing-only ablations (attribute set per launch)
  else if (dbg == 4) INC_A3H(1 - INC_3A2B_DEFAULT_SCHED)
  else if (dbg == 6) INC_A3H(3)
  else if (dbg == 31) INC_A3H(31)
  else if (dbg == 32) INC_A3H(32)
  else if (dbg == 34) INC_A3H(34)
  else if (dbg == 37) INC_A3H(37)
  else if (dbg == 20) INC_A3H(10)  // 20..26: timing-only ablations of schedule 1 (wrong results by construction)
  else if (dbg == 21) INC_A3H(11)
  else if (dbg == 22) INC_A3H(12)
  else if (dbg == 23) INC_A3H(13)
  else if (dbg == 24) INC_A3H(14)
  else if (dbg == 25) INC_A3H(15)
  else if (dbg == 26) INC_A3H(16)
  else if (dbg == 27) INC_A3H(17)
  else if (dbg == 28) INC_A3H(18)
  else if (dbg == 29) INC_A3H(19)
  else if (dbg == 30) INC_A3H(20)
#undef INC_A3H
#endif
  else INC_A3(true, INC_3A2B_DEFAULT_SCHED);
#undef INC_A3
#undef INC_A3_ATTR
  if (part) return inc_launch_slab_reduce(a, part, splits);
  INC_LAUNCH_RETURN();
}

#ifdef INC_KBENCH
#include "../../tools/kbench_gemm_2.inc"
#endif  // INC_KBENCH
