// gemm_d2r.hip -- K4a, third generation: fused INT4 -> bf16 dequant-GEMM with the weights DIRECT TO REGISTERS.
//
// Replaces INCWeightOnlyLinear.forward (reference modules.py:594-610 = recover() once + F.linear) for M > 64 rows, like the
// producer / consumer kernel (tools/kbench_gemm_1.inc, built into gemm_tile256.hip by the harness), with the same 256 x 256 x 64 tile and bit-identical outputs (every accumulator
// receives the same MFMAs in the same order).  What changes is who touches the weights:
//
//   * a packed word of the optimum layout (8 consecutive k of ONE output column, modules.py:254-260) IS one lane's A operand
//     of v_mfma_f32_32x32x16_bf16 once dequantised.  The workgroup has FOUR waves, one per SIMD, and wave w owns ALL 256 rows
//     of the tile x the 64 columns [64 w, 64 w + 64): every weight of the tile is needed by exactly one wave, so that wave
//     loads its packed words straight from global memory (two 128-byte segments per request), dequantises them in registers
//     (the fp8-decoder arithmetic of dequant8: bit-identical to inc_woq_dequant) and multiplies -- the dequantised tile never
//     exists in LDS: no producer waves, no 32 KiB of ds_write_b128 per K-step, no W fragment reads, no redundant arithmetic;
//   * one wave per SIMD owns the SIMD's whole 512-entry register file: 2 x 8 accumulator tiles of 32 x 32 (256 registers),
//     two x-fragment sets and two W-fragment sets (software pipeline one k16 group deep), three sets of packed words (loaded
//     two K-steps ahead);
//   * LDS holds only x: NS stages of 32 KiB filled by LDS-DMA (global_load_lds_dwordx4, 8 pieces of 1 KiB per wave and step,
//     XOR-swizzled chunks, NS - 1 steps ahead), read as 8 conflict-free ds_read_b128 per k16 group and wave.
//
// Per K-step and wave: 64 MFMAs, 32 fragment reads, 8 packed words (152 VALU) + 2 group parameters, 12 small loads, 8 DMA pieces,
// one barrier.  With a single wave per SIMD nothing else hides an instruction, so the step is written as 16 sub-regions of
// 4 MFMAs, each carrying its share of the reads / arithmetic / requests, pinned with sched_barrier fences.
#include <type_traits>

#include "gemm_common.hpp"
#include "tile256_frame.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
constexpr int D2R_THREADS = 256;
constexpr int D2R_CPITCH = TN * 2 + 16;  // epilogue image of the bf16 tile in LDS: 528-byte rows

template <int NS>
constexpr int d2r_smem_bytes() {
  return NS * T_ASTAGE > TM * D2R_CPITCH ? NS * T_ASTAGE : TM * D2R_CPITCH;
}


// compile-time loop: f(std::integral_constant<int, B>) ... f(std::integral_constant<int, E - 1>)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}
// one accumulator register (AGPR R) of the direct-to-register kernel
template <int R>
__device__ __forceinline__ float acc_read() {
  float v;
  asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(v) : "i"(R));
  return v;
}
template <int R>
__device__ __forceinline__ void acc_zero() {
  asm volatile("v_accvgpr_write_b32 a%c0, 0" : : "i"(R));
}
// a0 .. a255 as an asm clobber list: reserves the accumulator half of the register file in the kernel descriptor
#define INC_D2R_AGPR_CLOBBERS \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", \
  "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", \
  "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", \
  "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", \
  "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", \
  "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", \
  "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", \
  "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", \
  "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", \
  "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", \
  "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", \
  "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", \
  "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", \
  "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", \
  "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", \
  "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"
#define INC_D2R_ZERO_ACC()                                 \
  asm volatile("" : : : INC_D2R_AGPR_CLOBBERS);            \
  static_for<0, 256>([&](auto R) { acc_zero<R.value>(); })
#define INC_SB() __builtin_amdgcn_sched_barrier(0)

#ifdef INC_KBENCH
// harness build only (tools/kbench d2rtl, ABL bit 8 = 256): per-workgroup time stamps of wave 0 -- [0..3] s_memrealtime (100 MHz) at
// entry / first K-step / after the K-loop / after the last store was acknowledged, [4..7] s_memtime (shader clock) at the same
// points, [8] XCC id, [9] HW_ID
__device__ unsigned long long* g_d2r_timeline = nullptr;
#define INC_D2R_STAMP(SLOT)                                                                                   \
  if constexpr ((ABL & 256) != 0) {                                                                            \
    /* no divergent branch (it broke the scalar-register bookkeeping of the asm statements): EVERY thread stores, threads other  \
       than 0 into a scratch area behind the records (the buffer holds 10 * workgroups + 256 words) */                           \
    const unsigned long long rt_ = __builtin_amdgcn_s_memrealtime(), ct_ = __builtin_amdgcn_s_memtime();        \
    unsigned xcc_, hw_;                                                                                         \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                                         \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                                           \
    unsigned long long* const tl_ = g_d2r_timeline;                                                             \
    const size_t rec_ = (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 10, scratch_ = (size_t)gridDim.x * gridDim.y * 10 + threadIdx.x; \
    const bool first_ = threadIdx.x == 0;                                                                       \
    tl_[first_ ? rec_ + (SLOT) : scratch_] = rt_;                                                               \
    tl_[first_ ? rec_ + 4 + (SLOT) : scratch_] = ct_;                                                           \
    if ((SLOT) == 0) {                                                                                          \
      tl_[first_ ? rec_ + 8 : scratch_] = xcc_ & 15u;                                                           \
      tl_[first_ ? rec_ + 9 : scratch_] = hw_;                                                                  \
    }                                                                                                           \
  }
#else
#define INC_D2R_STAMP(SLOT)
#endif

// ABL (harness build only, timing-only, WRONG results): bit 2 no x LDS-DMA, 3 no W loads, 6 no per-step barrier, 7 no epilogue stores,
// 9 no scalar pointer arithmetic (every step re-reads the first tiles)
template <bool IS_BF16, int NS, int ABL>
__global__ __launch_bounds__(D2R_THREADS) void woq_gemm_w4_d2r_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t M, int64_t N,
    int64_t K, int64_t NW, int g_shift, int y_vec_ok, float* __restrict__ partial, int steps_per_split) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  INC_D2R_STAMP(0)
  constexpr int D = NS - 1;                   // the x DMA runs D steps ahead
  constexpr int VM_STEADY = D >= 3 ? 22 : 14;  // see "counted waits" below
  const int tiles_n = (int)((N + TN - 1) / TN);
  const int tiles_m = (int)((M + TM - 1) / TM);
  const int nwg = tiles_m * tiles_n;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
  const int64_t m0 = (int64_t)tm * TM, n0 = (int64_t)tn * TN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nk_all = (int)(K / TK);
  const int kbase = blockIdx.y * steps_per_split;
  const int nk = min(steps_per_split, nk_all - kbase);
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const bool lds_epilogue = !partial && (y_vec_ok & 2) && m0 + TM <= M && n0 + TN <= N && (ABL & 128) == 0;
  const float inv_u = fp8_unit_inverse();

  // ---- x tile by LDS-DMA: the swizzled row stage of tile256_frame.hpp, 8 pieces per wave ----
  // Running state (scalar registers, advanced once per step in a fenced slot far from the requests that read them): `xptr` = the
  // tile the NEXT pieces fetch (clamped at the last tile: the tail requests re-read valid memory and are never used), `dma_off` = the
  // LDS stage they fill.
  using XStage = RowStage<TK * 2, 8>;  // the frame's x tile, staged by four waves
  uint32_t avoff[8];
  XStage::offsets(wave, lane, m0, M, 2 * K, avoff);
  const uint16_t* xptr = x + m0 * K + (int64_t)kbase * TK;
  int xt = 0;
  uint32_t dma_off = 0;
  const uint32_t dma_lds0 = __builtin_amdgcn_readfirstlane(lds0 + wave * 8192);
#define INC_D2R_DMA(I)                                                                                                        \
  if constexpr ((ABL & 4) == 0) {                                                                                             \
    /* M0 = LDS base of the piece (s_nop 0: M0 write -> LDS-DMA); xptr was advanced and pinned a sub-region earlier */                          \
    asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(avoff[I]), "s"(xptr), "s"(dma_lds0 + dma_off), "i"((I)*1024) : "memory", "scc"); \
  }
  const uint16_t* const xbase = xptr;
  auto advance_x = [&]() {  // scalar arithmetic only (no branch): the tile index saturates at the last tile
    if constexpr ((ABL & 512) != 0) return;  // (harness, timing-only: the step without its scalar pointer arithmetic)
    asm volatile("" : "+s"(xt), "+s"(dma_off));  // inputs pinned too: the arithmetic starts HERE, behind the slot's MFMA
    xt = min(xt + 1, nk - 1);
    xptr = xbase + (uint32_t)(xt * TK);
    dma_off = dma_off + T_ASTAGE == NS * T_ASTAGE ? 0u : dma_off + T_ASTAGE;
    asm volatile("" : "+s"(xptr), "+s"(dma_off), "+s"(xt));  // computed HERE, in this slot (the compiler would sink it to its first use)
  };

  // ---- packed words: this lane's A operands.  Accumulator row r = lane & 31 of fragment nf IS column n0 + 64 wave + 2 r + nf: the
  // lane's two columns are adjacent in memory, so ONE 8-byte request fetches the words of both fragments for a k-octet (2 kk +
  // (lane >> 5)), one dword both fp16 scales, one dword the zero-point word of both -- 6 requests per step instead of 12.  (Which
  // columns a wave's MFMA rows stand for is free: the epilogue writes them where they belong.)
  uint32_t wvoff[4], svoff, zvoff;  // wvoff[kk]
  int zshift[2];
  {
    int64_t ncol = n0 + wave * 64 + 2 * (lane & 31);
    if (ncol > N - 2) ncol = N - 2;  // N is even (launcher); columns past N are computed from valid words and never stored
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) wvoff[kk] = (uint32_t)((((int64_t)(2 * kk + (lane >> 5))) * N + ncol) * 4);
    svoff = (uint32_t)(ncol * 2);
    zvoff = (uint32_t)((ncol / 8) * 4);
    zshift[0] = 4 * (int)(ncol % 8);
    zshift[1] = zshift[0] + 4;
  }
  // running pointers of the NEXT register loads (tile `wt`, clamped at the last tile) and of its group's parameters
  const uint32_t* wptr = qweight + (int64_t)kbase * (TK / 8) * N;
  const int64_t g0 = g_shift >= 0 ? (((int64_t)kbase * TK) >> g_shift) : 0;
  const uint16_t* sptr = scales + g0 * N;
  const uint32_t* zptr = qzeros + g0 * NW;
  const uint16_t* const sbase = sptr;
  const uint32_t* const zbase = zptr;
  const int g0base = (int)g0;
  int wt = 0;
  const uint32_t* const wbase = wptr;
  const int64_t wstride = (int64_t)(TK / 8) * N;
  const int gsh = g_shift >= 6 ? g_shift - 6 : -1;  // tiles per group = 1 << gsh; -1: a single group
  uint32_t gi_ = 0;
  const uint32_t wstride32 = (uint32_t)wstride, n32 = (uint32_t)N, nw32 = (uint32_t)NW;  // every offset below is < 2^31 elements (inc_woq_gemm checks)
  auto advance_w = [&](int part) {  // scalar arithmetic only (no branch), in three small pieces for three gaps of the step
    if constexpr ((ABL & 512) != 0) return;
    if (part == 0) {
      asm volatile("" : "+s"(wt));
      wt = min(wt + 1, nk - 1);
      wptr = wbase + (uint32_t)wt * wstride32;
      asm volatile("" : "+s"(wptr), "+s"(wt));  // see advance_x
    } else if (part == 1) {
      gi_ = gsh >= 0 ? (uint32_t)((kbase + wt) >> gsh) - (uint32_t)g0base : 0u;
      sptr = sbase + gi_ * n32;
      asm volatile("" : "+s"(sptr), "+s"(gi_));
    } else {
      asm volatile("" : "+s"(gi_));
      zptr = zbase + gi_ * nw32;
      asm volatile("" : "+s"(zptr));
    }
  };
  u32x2 W[3][4];            // [tile % 3][kk]: .x = word of fragment 0, .y = fragment 1
  uint32_t SC[3], ZW[3];    // both fp16 scales / the zero-point word of the lane's two columns
  // the step's 6 register loads as three requests of two: part 0 = words of kk 0, 1; part 1 = kk 2, 3; part 2 = scales + zero word.
  // No s_nop in front: the pointers were advanced (and pinned) a sub-region earlier.
#define INC_D2R_LOADW(SET, PART)                                                                                                   \
  if constexpr ((ABL & 8) != 0) {                                                                                                  \
    asm volatile("" : "=v"(W[SET][2 * (PART)]), "=v"(W[SET][2 * (PART) + 1]));                                                     \
  } else {                                                                                                                         \
    asm volatile(                                                                                                                  \
        "global_load_dwordx2 %0, %2, %4\n\t"                                                                                       \
        "global_load_dwordx2 %1, %3, %4"                                                                                           \
        : "=&v"(W[SET][2 * (PART)]), "=&v"(W[SET][2 * (PART) + 1])                                                                 \
        : "v"(wvoff[2 * (PART)]), "v"(wvoff[2 * (PART) + 1]), "s"(wptr)                                                            \
        : "memory");                                                                                                               \
  }
#define INC_D2R_LOADP(SET)                                                                                                         \
  if constexpr ((ABL & 8) != 0) {                                                                                                  \
    asm volatile("" : "=v"(SC[SET]), "=v"(ZW[SET]));                                                                               \
  } else {                                                                                                                         \
    asm volatile(                                                                                                                  \
        "global_load_dword %0, %2, %4\n\t"                                                                                         \
        "global_load_dword %1, %3, %5"                                                                                             \
        : "=&v"(SC[SET]), "=&v"(ZW[SET])                                                                                           \
        : "v"(svoff), "v"(zvoff), "s"(sptr), "s"(zptr)                                                                             \
        : "memory");                                                                                                               \
  }
  // counted waits.  Program order of a step's 14 requests: 6 register loads (tile t+2), then 8 DMA pieces (tile t+D).  At the
  // wait of step t the words of tile t+1 (issued in step t-1) and the x pieces of tile t+1 (issued in step t+1-D) must be
  // back: D = 2 -> everything up to step t-1, this step's 14 stay in flight; D >= 3 -> step t-1's 8 pieces stay in flight too.
#define INC_D2R_WAIT(SET, NN)                                                                                                       \
  if constexpr ((ABL & 12) == 12)                                                                                                   \
    asm volatile("" : "+v"(W[SET][0]), "+v"(W[SET][1]), "+v"(W[SET][2]), "+v"(W[SET][3]), "+v"(SC[SET]), "+v"(ZW[SET]) : : "memory"); \
  else                                                                                                                              \
    asm volatile("s_waitcnt vmcnt(%6)" : "+v"(W[SET][0]), "+v"(W[SET][1]), "+v"(W[SET][2]), "+v"(W[SET][3]), "+v"(SC[SET]), "+v"(ZW[SET]) : "i"(NN) : "memory");

  // ---- x fragments: B operand (mf): rows 32 mf + (lane & 31), 16-byte chunk 2 kk + (lane >> 5) of the swizzled row ----------------
  const int a_sw = XStage::swz(lane & 31), a_hi = lane >> 5;
  uint32_t xaddr[4];  // LDS byte address of this lane's chunk of row lane & 31, stage 0, per k16 group
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) xaddr[kk] = lds0 + (uint32_t)((lane & 31) * 128) + (uint32_t)XStage::chunk_off(2 * kk + a_hi, a_sw);
  uint32_t rd_off = 0, rd_nxt = 0;  // LDS stage of the tile being multiplied / of the next one
  u32x4 X[2][8];
  uint32_t xa_;
#define INC_PIN1(a) asm volatile("" : "+v"(a))
#define INC_D2R_XADDR(ST, KK) xa_ = xaddr[KK] + (ST); INC_PIN1(xa_)
#define INC_LGKM(NN) asm volatile("s_waitcnt lgkmcnt(%0)" : : "i"(NN) : "memory")

  // The 256 accumulators are the AGPR half of the SIMD's register file, addressed LITERALLY (a[16 j : 16 j + 15] for accumulator
  // j = 8 nf + mf) by asm statements only: the compiler never sees them as values, so it cannot shuffle them between the two halves
  // of the file (it did: 1400 spilled registers with `f32x16 acc[2][8]`).  The first statement clobbers a0..a255, which makes the
  // kernel descriptor allocate them; audit after every edit: no compiler-generated v_accvgpr_* and no scratch (tools/audit_d2r.py).
  uint4 Wf[2][2];
  float sc[2], nzs[2];   // per fragment: scale / 2^-9 (the fp8 decoder's unit) and -zero * scale
  uint32_t mlo, mhi;     // nibble masks of the word being dequantised (half A leaves them for half B)
  float gp_s0;           // group-parameter temporaries that cross a sub-region
  uint32_t gp_z;
  INC_D2R_ZERO_ACC();
  // ==== the K-loop's building block: ONE asm statement per sub-region = 4 MFMAs, each followed by its slot ====================
  // A single wave per SIMD issues in order, so every instruction between two MFMAs is paid for unless there are at most ~5 of
  // them (MI355X_MICROARCH.md); with C++ slots the compiler added a wait-state pad or an s_waitcnt to almost every one.  Inside a
  // statement nothing is added.  Temporaries that live inside one statement are literal registers v246..v255 (clobbered, so the
  // compiler keeps nothing there): cq = v[252:253], dq = v[254:255] (the two halves of a packed fp8 conversion cannot be named
  // through an operand), f0..f3 = v248..v251, f16 conversion temporaries v246, v247.
  // Arithmetic = dequant8's FORM 0 (gemm_common.hpp), instruction for instruction: bit-identical to inc_woq_dequant.
  // accumulator I of the sub-region = a[16 (J + I) : 16 (J + I) + 15], J = %c[aj] (the assembler evaluates the expressions)
#define D2R_MFMA(MN, I) MN " a[%c[aj]+" #I "*16:%c[aj]+" #I "*16+15], %[wf], %[x" #I "], a[%c[aj]+" #I "*16:%c[aj]+" #I "*16+15]\n\t"
#define D2R_RD(I) "ds_read_b128 %[r" #I "], %[xa] offset:%c[o" #I "]\n\t"
  // half A of word %[w]: k 0..3 -> %[oa], %[ob]; leaves the masks in %[mlo], %[mhi]
#define D2R_DQA0 "v_and_b32 %[mlo], 0xf0f0f0f, %[w]\n\tv_lshrrev_b32 %[mhi], 4, %[w]\n\tv_cvt_pk_f32_fp8 v[252:253], %[mlo]\n\tv_and_b32 %[mhi], 0xf0f0f0f, %[mhi]\n\t"
#define D2R_DQA1 "v_cvt_pk_f32_fp8 v[254:255], %[mhi]\n\tv_fma_f32 v248, v252, %[sc], %[nz]\n\tv_fma_f32 v250, v253, %[sc], %[nz]\n\t"
#define D2R_DQA2(CVTP) "v_fma_f32 v249, v254, %[sc], %[nz]\n\tv_fma_f32 v251, v255, %[sc], %[nz]\n\t" CVTP("%[oa]", "v248", "v249") CVTP("%[ob]", "v250", "v251")
  // half B: k 4..7 of the masked word -> %[oa], %[ob]
#define D2R_DQB0 "v_cvt_pk_f32_fp8_sdwa v[252:253], %[mlo] src0_sel:WORD_1\n\tv_cvt_pk_f32_fp8_sdwa v[254:255], %[mhi] src0_sel:WORD_1\n\t"
#define D2R_DQB1 "v_fma_f32 v248, v252, %[sc], %[nz]\n\tv_fma_f32 v249, v254, %[sc], %[nz]\n\tv_fma_f32 v250, v253, %[sc], %[nz]\n\t"
#define D2R_DQB2(CVTP) "v_fma_f32 v251, v255, %[sc], %[nz]\n\t" CVTP("%[oa]", "v248", "v249") CVTP("%[ob]", "v250", "v251")
  // group parameters (modules.py:407-410: the stored zero point is zp - 1 and wraps above 15).  GP0 extracts the fp16 scale (low /
  // high half of the pair's dword) and zero + 1; GP1 finishes: zero > 15 -> 0, %[nz] = -zero * scale, %[sc] = scale * 2^9
#define D2R_GP0_LO "v_cvt_f32_f16 %[gs], %[scw]\n\tv_bfe_u32 %[gz], %[zw], %[zsh], 4\n\tv_add_u32 %[gz], 1, %[gz]\n\t"
#define D2R_GP0_HI "v_cvt_f32_f16_sdwa %[gs], %[scw] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\tv_bfe_u32 %[gz], %[zw], %[zsh], 4\n\tv_add_u32 %[gz], 1, %[gz]\n\t"
#define D2R_GP1 "v_cmp_gt_u32 vcc, 16, %[gz]\n\tv_cndmask_b32 %[gz], 0, %[gz], vcc\n\tv_cvt_f32_u32 %[gz], %[gz]\n\tv_mul_f32_e64 %[nz], %[gs], -%[gz]\n\tv_mul_f32 %[sc], %[iu], %[gs]\n\t"
#define D2R_CVTP_BF16(D, A, B) "v_cvt_pk_bf16_f32 " D ", " A ", " B "\n\t"
#define D2R_CVTP_F16(D, A, B) "v_cvt_f16_f32 v246, " A "\n\tv_cvt_f16_f32 v247, " B "\n\tv_pack_b32_f16 " D ", v246, v247\n\t"
#define D2R_TMPS "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255"
  // inputs every sub-region has: the W fragment (A operand), four x fragments (B operands), the first accumulator's index
#define D2R_IN(CUR, Q)                                                                                                            \
  [wf] "v"(wf_), [x0] "v"(X[CUR][4 * ((Q)&1)]), [x1] "v"(X[CUR][4 * ((Q)&1) + 1]), [x2] "v"(X[CUR][4 * ((Q)&1) + 2]),              \
      [x3] "v"(X[CUR][4 * ((Q)&1) + 3]), [aj] "i"(16 * (8 * ((Q) >> 1) + 4 * ((Q)&1)))
#define D2R_WF(CUR, Q) const u32x4 wf_ = {Wf[CUR][(Q) >> 1].x, Wf[CUR][(Q) >> 1].y, Wf[CUR][(Q) >> 1].z, Wf[CUR][(Q) >> 1].w};
#define D2R_MN_BF16 "v_mfma_f32_32x32x16_bf16"
#define D2R_MN_F16 "v_mfma_f32_32x32x16_f16"

  // kind A (sub-regions 0 / 2 of groups 0..2): reads x fragments MA, MA + 1 of set NXT; half A of WORD -> Wf[NXT][NF].x/.y
#define D2R_ASM_A(MN, CVTP, CUR, Q, NXT, MA, NF)                                                                                  \
  asm volatile(D2R_MFMA(MN, 0) D2R_RD(0) D2R_DQA0 D2R_MFMA(MN, 1) D2R_RD(1) D2R_DQA1 D2R_MFMA(MN, 2) D2R_DQA2(CVTP) D2R_MFMA(MN, 3) \
               : [r0] "=&v"(X[NXT][MA]), [r1] "=&v"(X[NXT][(MA) + 1]), [oa] "=&v"(Wf[NXT][NF].x), [ob] "=&v"(Wf[NXT][NF].y),        \
                 [mlo] "=&v"(mlo), [mhi] "=&v"(mhi)                                                                                \
               : D2R_IN(CUR, Q), [xa] "v"(xa_), [w] "v"(w_), [sc] "v"(sc[NF]), [nz] "v"(nzs[NF]), [o0] "i"((MA)*4096),              \
                 [o1] "i"(((MA) + 1) * 4096)                                                                                       \
               : D2R_TMPS)
#define INC_D2R_SUB_A(CUR, Q, NXT, MA, WORD, NF)                                                                                  \
  {                                                                                                                               \
    D2R_WF(CUR, Q)                                                                                                                \
    const uint32_t w_ = (WORD);                                                                                                   \
    if constexpr (IS_BF16) D2R_ASM_A(D2R_MN_BF16, D2R_CVTP_BF16, CUR, Q, NXT, MA, NF);                                            \
    else D2R_ASM_A(D2R_MN_F16, D2R_CVTP_F16, CUR, Q, NXT, MA, NF);                                                                \
  }
  // kind B (sub-regions 1 / 3): reads x fragments MA, MA + 1 of set NXT; half B of the masked word -> Wf[NXT][NF].z/.w
#define D2R_ASM_B(MN, CVTP, CUR, Q, NXT, MA, NF)                                                                                  \
  asm volatile(D2R_MFMA(MN, 0) D2R_RD(0) D2R_DQB0 D2R_MFMA(MN, 1) D2R_RD(1) D2R_DQB1 D2R_MFMA(MN, 2) D2R_DQB2(CVTP) D2R_MFMA(MN, 3) \
               : [r0] "=&v"(X[NXT][MA]), [r1] "=&v"(X[NXT][(MA) + 1]), [oa] "=&v"(Wf[NXT][NF].z), [ob] "=&v"(Wf[NXT][NF].w)         \
               : D2R_IN(CUR, Q), [xa] "v"(xa_), [mlo] "v"(mlo), [mhi] "v"(mhi), [sc] "v"(sc[NF]), [nz] "v"(nzs[NF]),               \
                 [o0] "i"((MA)*4096), [o1] "i"(((MA) + 1) * 4096)                                                                  \
               : D2R_TMPS)
#define INC_D2R_SUB_B(CUR, Q, NXT, MA, NF)                                                                                        \
  {                                                                                                                               \
    D2R_WF(CUR, Q)                                                                                                                \
    if constexpr (IS_BF16) D2R_ASM_B(D2R_MN_BF16, D2R_CVTP_BF16, CUR, Q, NXT, MA, NF);                                            \
    else D2R_ASM_B(D2R_MN_F16, D2R_CVTP_F16, CUR, Q, NXT, MA, NF);                                                                \
  }
  // kind B + the first half of fragment 0's NEXT group parameters behind the last MFMA (group 2's last sub-region)
#define D2R_ASM_BG(MN, CVTP, CUR, Q, NXT, MA, NF, SET)                                                                            \
  asm volatile(D2R_MFMA(MN, 0) D2R_RD(0) D2R_DQB0 D2R_MFMA(MN, 1) D2R_RD(1) D2R_DQB1 D2R_MFMA(MN, 2) D2R_DQB2(CVTP) D2R_MFMA(MN, 3) \
                   D2R_GP0_LO                                                                                                     \
               : [r0] "=&v"(X[NXT][MA]), [r1] "=&v"(X[NXT][(MA) + 1]), [oa] "=&v"(Wf[NXT][NF].z), [ob] "=&v"(Wf[NXT][NF].w),        \
                 [gs] "=&v"(gp_s0), [gz] "=&v"(gp_z)                                                                               \
               : D2R_IN(CUR, Q), [xa] "v"(xa_), [mlo] "v"(mlo), [mhi] "v"(mhi), [sc] "v"(sc[NF]), [nz] "v"(nzs[NF]),               \
                 [o0] "i"((MA)*4096), [o1] "i"(((MA) + 1) * 4096), [scw] "v"(SC[SET]), [zw] "v"(ZW[SET]), [zsh] "v"(zshift[0])      \
               : D2R_TMPS)
#define INC_D2R_SUB_BG(CUR, Q, NXT, MA, NF, SET)                                                                                  \
  {                                                                                                                               \
    D2R_WF(CUR, Q)                                                                                                                \
    if constexpr (IS_BF16) D2R_ASM_BG(D2R_MN_BF16, D2R_CVTP_BF16, CUR, Q, NXT, MA, NF, SET);                                      \
    else D2R_ASM_BG(D2R_MN_F16, D2R_CVTP_F16, CUR, Q, NXT, MA, NF, SET);                                                          \
  }
  // group 3, sub-region 0 (no reads: the next stage is not visible yet): fragment 0's new parameters, then half A of tile t+1's
  // first word of fragment 0 -> Wf[0][0].x/.y
#define D2R_ASM_G0(MN, CVTP, SET)                                                                                                 \
  asm volatile(D2R_MFMA(MN, 0) D2R_GP1 D2R_MFMA(MN, 1) D2R_DQA0 D2R_MFMA(MN, 2) D2R_DQA1 D2R_MFMA(MN, 3) D2R_DQA2(CVTP)            \
               : [oa] "=&v"(Wf[0][0].x), [ob] "=&v"(Wf[0][0].y), [mlo] "=&v"(mlo), [mhi] "=&v"(mhi), [sc] "=&v"(sc[0]),             \
                 [nz] "=&v"(nzs[0]), [gz] "+v"(gp_z)                                                                               \
               : D2R_IN(1, 0), [w] "v"(w_), [gs] "v"(gp_s0), [iu] "v"(inv_u)                                                       \
               : D2R_TMPS, "vcc")
#define INC_D2R_SUB_G0(SET)                                                                                                       \
  {                                                                                                                               \
    D2R_WF(1, 0)                                                                                                                  \
    const uint32_t w_ = W[SET][0].x;                                                                                              \
    if constexpr (IS_BF16) D2R_ASM_G0(D2R_MN_BF16, D2R_CVTP_BF16, SET);                                                           \
    else D2R_ASM_G0(D2R_MN_F16, D2R_CVTP_F16, SET);                                                                               \
  }
  // group 3, sub-region 1 (behind the barrier): x fragments 0..2 of the next stage, half B of fragment 0's word, first half of
  // fragment 1's parameters
#define D2R_ASM_G1(MN, CVTP, SET)                                                                                                 \
  asm volatile(D2R_MFMA(MN, 0) D2R_RD(0) D2R_DQB0 D2R_MFMA(MN, 1) D2R_RD(1) D2R_DQB1 D2R_MFMA(MN, 2) D2R_RD(2) D2R_DQB2(CVTP)      \
                   D2R_MFMA(MN, 3) D2R_GP0_HI                                                                                     \
               : [r0] "=&v"(X[0][0]), [r1] "=&v"(X[0][1]), [r2] "=&v"(X[0][2]), [oa] "=&v"(Wf[0][0].z), [ob] "=&v"(Wf[0][0].w),     \
                 [gs] "=&v"(gp_s0), [gz] "=&v"(gp_z)                                                                               \
               : D2R_IN(1, 1), [xa] "v"(xa_), [mlo] "v"(mlo), [mhi] "v"(mhi), [sc] "v"(sc[0]), [nz] "v"(nzs[0]), [o0] "i"(0),       \
                 [o1] "i"(4096), [o2] "i"(8192), [scw] "v"(SC[SET]), [zw] "v"(ZW[SET]), [zsh] "v"(zshift[1])                       \
               : D2R_TMPS)
#define INC_D2R_SUB_G1(SET)                                                                                                       \
  {                                                                                                                               \
    D2R_WF(1, 1)                                                                                                                  \
    if constexpr (IS_BF16) D2R_ASM_G1(D2R_MN_BF16, D2R_CVTP_BF16, SET);                                                           \
    else D2R_ASM_G1(D2R_MN_F16, D2R_CVTP_F16, SET);                                                                               \
  }
  // group 3, sub-region 2: x fragments 3..5, fragment 1's new parameters, half A of its first word -> Wf[0][1].x/.y
#define D2R_ASM_G2(MN, CVTP, SET)                                                                                                 \
  asm volatile(D2R_MFMA(MN, 0) D2R_RD(0) D2R_GP1 D2R_MFMA(MN, 1) D2R_RD(1) D2R_DQA0 D2R_MFMA(MN, 2) D2R_RD(2) D2R_DQA1            \
                   D2R_MFMA(MN, 3) D2R_DQA2(CVTP)                                                                                 \
               : [r0] "=&v"(X[0][3]), [r1] "=&v"(X[0][4]), [r2] "=&v"(X[0][5]), [oa] "=&v"(Wf[0][1].x), [ob] "=&v"(Wf[0][1].y),     \
                 [mlo] "=&v"(mlo), [mhi] "=&v"(mhi), [sc] "=&v"(sc[1]), [nz] "=&v"(nzs[1]), [gz] "+v"(gp_z)                         \
               : D2R_IN(1, 2), [xa] "v"(xa_), [w] "v"(w_), [gs] "v"(gp_s0), [iu] "v"(inv_u), [o0] "i"(3 * 4096),                   \
                 [o1] "i"(4 * 4096), [o2] "i"(5 * 4096)                                                                            \
               : D2R_TMPS, "vcc")
#define INC_D2R_SUB_G2(SET)                                                                                                       \
  {                                                                                                                               \
    D2R_WF(1, 2)                                                                                                                  \
    const uint32_t w_ = W[SET][0].y;                                                                                              \
    if constexpr (IS_BF16) D2R_ASM_G2(D2R_MN_BF16, D2R_CVTP_BF16, SET);                                                           \
    else D2R_ASM_G2(D2R_MN_F16, D2R_CVTP_F16, SET);                                                                               \
  }

  // ---- prologue: words of tiles 0, 1 and x tiles 0 .. D-1 requested; tile 0 complete ---------------------------------------
  INC_D2R_LOADW(0, 0) INC_D2R_LOADW(0, 1) INC_D2R_LOADP(0)
  INC_D2R_DMA(0) INC_D2R_DMA(1) INC_D2R_DMA(2) INC_D2R_DMA(3) INC_D2R_DMA(4) INC_D2R_DMA(5) INC_D2R_DMA(6) INC_D2R_DMA(7)
  advance_w(0); advance_w(1); advance_w(2);
  advance_x();
  INC_SB();
  INC_D2R_LOADW(1, 0) INC_D2R_LOADW(1, 1) INC_D2R_LOADP(1)
  advance_w(0); advance_w(1); advance_w(2);
#pragma unroll
  for (int d = 1; d < D; ++d) {
    INC_SB();
    INC_D2R_DMA(0) INC_D2R_DMA(1) INC_D2R_DMA(2) INC_D2R_DMA(3) INC_D2R_DMA(4) INC_D2R_DMA(5) INC_D2R_DMA(6) INC_D2R_DMA(7)
    advance_x();
  }
  INC_SB();
  INC_D2R_WAIT(0, VM_STEADY)  // outstanding allowed: tile 1's 6 requests + (D-1) x 8 pieces = 14 (D = 2) or 22 (D = 3)
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {  // tile 0's parameters and first fragments, in plain C++ (once per tile of the output)
    const float s0 = f16_bits_to_f32((uint16_t)(nf ? SC[0] >> 16 : SC[0]));
    uint32_t zz = ((ZW[0] >> zshift[nf]) & 15u) + 1u;
    zz = zz > 15u ? 0u : zz;
    nzs[nf] = -(float)zz * s0;
    sc[nf] = s0 * inv_u;
    Wf[0][nf] = dequant8<IS_BF16>(nf ? W[0][0].y : W[0][0].x, sc[nf], nzs[nf]);
  }
  INC_D2R_XADDR(0u, 0);
  asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:4096\n\tds_read_b128 %2, %8 offset:8192\n\tds_read_b128 %3, %8 offset:12288\n\t"
               "ds_read_b128 %4, %8 offset:16384\n\tds_read_b128 %5, %8 offset:20480\n\tds_read_b128 %6, %8 offset:24576\n\tds_read_b128 %7, %8 offset:28672"
               : "=&v"(X[0][0]), "=&v"(X[0][1]), "=&v"(X[0][2]), "=&v"(X[0][3]), "=&v"(X[0][4]), "=&v"(X[0][5]), "=&v"(X[0][6]), "=&v"(X[0][7])
               : "v"(xa_)
               : "memory");
  INC_SB();

  // One K-step.  `SET` = t % 3 (compile time: register sets); the LDS stages are run-time offsets.
  //   groups 0..2 (kk = g of tile t): multiply fragment set g & 1, prepare kk = g + 1 of the same stage / register set.  Between the
  //            sub-regions sit the step's requests: group 0: the 6 register loads of tile t+2 and DMA piece 0 of tile t+D; group 1:
  //            pieces 1..4; group 2: pieces 5..7 and the counted wait for tile t+1 (words + this wave's x pieces)
  //   group 3: new group parameters, words kk = 0 of tile t+1; the step's barrier after its first sub-region (every fragment read of
  //            this stage has returned: lgkmcnt(0)), then the x fragments kk = 0 of the next stage; the running pointers advance
  //   LDS returns in order: at a group's first MFMA x fragments 0..3 of its set must be back (the last four requests may still
  //   be out: lgkmcnt(4)); at its fifth MFMA fragments 4..7 (only the two reads sub-region 0 has just issued: lgkmcnt(2)).
#define INC_D2R_GROUP(CUR, NXT, KK, SET, P0, P1, P2, P3, LAST)                                                                    \
  INC_D2R_XADDR(rd_off, KK);                                                                                                     \
  P0 INC_LGKM(4); INC_SB();                                                                                                      \
  INC_D2R_SUB_A(CUR, 0, NXT, 0, W[SET][KK].x, 0)                                                                                 \
  INC_SB(); P1 INC_LGKM(2); INC_SB();                                                                                            \
  INC_D2R_SUB_B(CUR, 1, NXT, 2, 0)                                                                                               \
  INC_SB(); P2 INC_SB();                                                                                                         \
  INC_D2R_SUB_A(CUR, 2, NXT, 4, W[SET][KK].y, 1)                                                                                 \
  INC_SB(); P3 INC_SB();                                                                                                         \
  LAST                                                                                                                           \
  INC_SB();
#define INC_D2R_STEP(SET)                                                                                                         \
  {                                                                                                                               \
    constexpr int s1_ = ((SET) + 1) % 3, s2_ = ((SET) + 2) % 3;                                                                    \
    rd_nxt = rd_off + T_ASTAGE == NS * T_ASTAGE ? 0u : rd_off + T_ASTAGE;                                                         \
    INC_D2R_GROUP(0, 1, 1, SET, INC_D2R_LOADW(s2_, 0), INC_D2R_LOADW(s2_, 1), INC_D2R_LOADP(s2_), INC_D2R_DMA(0), INC_D2R_SUB_B(0, 3, 1, 6, 1)) \
    INC_D2R_GROUP(1, 0, 2, SET, INC_D2R_DMA(1), INC_D2R_DMA(2), INC_D2R_DMA(3), INC_D2R_DMA(4), INC_D2R_SUB_B(1, 3, 0, 6, 1))      \
    INC_D2R_GROUP(0, 1, 3, SET, INC_D2R_DMA(5), INC_D2R_DMA(6), INC_D2R_DMA(7), INC_D2R_WAIT(s1_, VM_STEADY), INC_D2R_SUB_BG(0, 3, 1, 6, 1, s1_)) \
    INC_LGKM(4); INC_SB();                                                                                                        \
    INC_D2R_SUB_G0(s1_)                                                                                                           \
    INC_SB();                                                                                                                     \
    advance_x();                                                                                                                  \
    INC_LGKM(0);                                                                                                                  \
    if constexpr ((ABL & 64) == 0) __builtin_amdgcn_s_barrier();                                                                  \
    INC_D2R_XADDR(rd_nxt, 0);                                                                                                     \
    INC_SB();                                                                                                                     \
    INC_D2R_SUB_G1(s1_)                                                                                                           \
    INC_SB();                                                                                                                     \
    advance_w(0);                                                                                                                 \
    INC_SB();                                                                                                                     \
    INC_D2R_SUB_G2(s1_)                                                                                                           \
    INC_SB();                                                                                                                     \
    advance_w(1);                                                                                                                 \
    INC_SB();                                                                                                                     \
    INC_D2R_SUB_B(1, 3, 0, 6, 1)                                                                                                  \
    INC_SB();                                                                                                                     \
    advance_w(2);                                                                                                                 \
    rd_off = rd_nxt;                                                                                                              \
    INC_SB();                                                                                                                     \
  }
  INC_D2R_STAMP(1)
  for (int t0 = 0; t0 < nk; t0 += 3) {
    INC_D2R_STEP(0)
    if (t0 + 1 >= nk) break;
    INC_D2R_STEP(1)
    if (t0 + 2 >= nk) break;
    INC_D2R_STEP(2)
  }
#undef INC_D2R_STEP
#undef INC_D2R_GROUP
#undef INC_D2R_WAIT
#undef INC_D2R_LOADP
#undef INC_D2R_LOADW
#undef INC_D2R_DMA
#undef INC_D2R_XADDR
#undef INC_LGKM
#undef INC_PIN1
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the last MFMAs' results: nothing the compiler emits may read them early
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped tail requests
  INC_D2R_STAMP(2)
  if constexpr ((ABL & 128) != 0) return;

  // ---- epilogue.  Accumulator j = 8 nf + mf, register r = 4 rq + e of it: D row i = e + 8 rq + 4 (lane >> 5), column (m) = lane & 31;
  // row i of fragment nf is output column 64 wave + 2 i + nf (the paired-column assignment above), so for a fixed (rq, lane >> 5) the
  // two fragments hold the EIGHT consecutive columns c0 = 64 wave + 16 rq + 8 (lane >> 5) .. c0 + 7, dword e = (nf 0, nf 1) of i = .. + e:
  // one 16-byte piece of an output row per (rq, mf).
  if (lds_epilogue) {
    // full tile, 16-byte aligned y: through LDS (the stages are dead), then whole 512-byte rows per store instruction
    __builtin_amdgcn_s_barrier();  // every wave has drained its DMA (vmcnt(0) above) and finished its fragment reads
    static_for<0, 4>([&](auto RQ) {
      constexpr int rq = RQ.value;
      const int c0 = wave * 64 + 16 * rq + 8 * (lane >> 5);
      float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = cvt16<IS_BF16>(bias[n0 + c0 + j]);
      }
      static_for<0, 8>([&](auto MF) {
        constexpr int mf = MF.value, r0 = 16 * mf + 4 * rq, r1 = 16 * (8 + mf) + 4 * rq;
        const int ml = mf * 32 + (lane & 31);
        *reinterpret_cast<uint4*>(smem + ml * D2R_CPITCH + c0 * 2) =
            make_uint4(cvt_pair<IS_BF16>(acc_read<r0>() + bv[0], acc_read<r1>() + bv[1]), cvt_pair<IS_BF16>(acc_read<r0 + 1>() + bv[2], acc_read<r1 + 1>() + bv[3]),
                       cvt_pair<IS_BF16>(acc_read<r0 + 2>() + bv[4], acc_read<r1 + 2>() + bv[5]), cvt_pair<IS_BF16>(acc_read<r0 + 3>() + bv[6], acc_read<r1 + 3>() + bv[7]));
      });
    });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    uint16_t* const ytile = y + m0 * N + n0;
#pragma unroll 4
    for (int i = tid; i < TM * (TN / 8); i += D2R_THREADS) {  // 16-byte chunk i: row i / 32, columns 8 (i % 32) .. +7
      const int row = i >> 5, c = i & 31;
      const uint4 v = *reinterpret_cast<const uint4*>(smem + row * D2R_CPITCH + c * 16);
      // write-through (sc1): the 128 KiB tile leaves the L2 as it is stored instead of staying dirty until the end-of-kernel
      // write-back (32 MiB per 4096 x 4096 output: +1.5 % on the whole kernel, tools/kbench d2r "sc1 epilogue stores")
      const u32x4 vv = {v.x, v.y, v.z, v.w};
      asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(ytile + (int64_t)row * N + c * 8), "v"(vv) : "memory");
    }
    if constexpr ((ABL & 256) != 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    INC_D2R_STAMP(3)
    return;
  }
  float* const slab = partial ? partial + (int64_t)blockIdx.y * M * N : nullptr;  // split-K: raw fp32 tile into this split's slab
  static_for<0, 4>([&](auto RQ) {
    constexpr int rq = RQ.value;
    const int64_t nb = n0 + wave * 64 + 16 * rq + 8 * (lane >> 5);
    float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (bias && !slab) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (nb + j < N) bv[j] = cvt16<IS_BF16>(bias[nb + j]);
    }
    static_for<0, 8>([&](auto MF) {
      constexpr int mf = MF.value, r0 = 16 * mf + 4 * rq, r1 = 16 * (8 + mf) + 4 * rq;
      const float vv_[8] = {acc_read<r0>() + bv[0],     acc_read<r1>() + bv[1],     acc_read<r0 + 1>() + bv[2], acc_read<r1 + 1>() + bv[3],
                           acc_read<r0 + 2>() + bv[4], acc_read<r1 + 2>() + bv[5], acc_read<r0 + 3>() + bv[6], acc_read<r1 + 3>() + bv[7]};
      const int64_t m = m0 + mf * 32 + (lane & 31);
      if (m < M) {
        if (slab) {  // (bias and conversion happen in the finalize kernel)
          float* dst = slab + m * N + nb;
          if (nb + 8 <= N && (N % 4) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(vv_[0], vv_[1], vv_[2], vv_[3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(vv_[4], vv_[5], vv_[6], vv_[7]);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (nb + j < N) dst[j] = vv_[j];
          }
        } else {
          uint16_t* dst = y + m * N + nb;
          if ((y_vec_ok & 1) && nb + 8 <= N) {  // 8-byte aligned rows: two 8-byte stores
            *reinterpret_cast<uint2*>(dst) = make_uint2(cvt_pair<IS_BF16>(vv_[0], vv_[1]), cvt_pair<IS_BF16>(vv_[2], vv_[3]));
            *reinterpret_cast<uint2*>(dst + 4) = make_uint2(cvt_pair<IS_BF16>(vv_[4], vv_[5]), cvt_pair<IS_BF16>(vv_[6], vv_[7]));
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (nb + j < N) dst[j] = IS_BF16 ? f32_to_bf16_bits(vv_[j]) : f32_to_f16_bits(vv_[j]);
          }
        }
      }
    });
  });
  if constexpr ((ABL & 256) != 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  INC_D2R_STAMP(3)
}
#undef INC_SB

}  // namespace

#ifdef INC_KBENCH
int g_d2r_abl_override = 0;  // harness flag 98: which time-stamped instantiation runs (256 | ablation bits)
extern "C" void inc_debug_set_d2r_abl(int abl) { g_d2r_abl_override = abl; }
extern "C" int inc_debug_set_d2r_timeline(void* dev_buffer) {  // harness only: where ABL 256 writes (10 x u64 per workgroup)
  unsigned long long* p = (unsigned long long*)dev_buffer;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_d2r_timeline), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#endif

// Launcher used by inc_woq_gemm (gemm.hip).  `abl` selects a timing-only ablation in the harness build (0 in the product).
int inc_launch_woq_gemm_d2r(const WoqGemmArgs& a, int y_vec_ok, float* part, int steps, int splits, int ns, int abl) {
  const unsigned grid = (unsigned)(ceil_div64(a.M, TM) * ceil_div64(a.N, TN));
  dim3 g2(grid, (unsigned)splits);
#ifdef INC_KBENCH
  if (abl == 256 && g_d2r_abl_override) abl = g_d2r_abl_override;
#endif
#define INC_D2R(B, NS_, A)                                                                                                             \
  {                                                                                                                                    \
    constexpr int smem = d2r_smem_bytes<NS_>();                                                                                        \
    static std::atomic<uint64_t> attr_set{0};                                                                                          \
    if (inc_attr_needed(attr_set)) {                                                                                                   \
      (void)hipFuncSetAttribute((const void*)woq_gemm_w4_d2r_kernel<B, NS_, A>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);    \
      inc_attr_done(attr_set);                                                                                                         \
    }                                                                                                                                  \
    woq_gemm_w4_d2r_kernel<B, NS_, A><<<g2, D2R_THREADS, smem, a.s>>>(a.x, a.qw, a.scales, a.qz, a.bias, a.y, a.M, a.N, a.K, a.NW, a.g_shift, y_vec_ok, part, steps); \
  }
  if (!a.bf) {
    INC_D2R(false, 4, 0)
  }
#ifdef INC_KBENCH
  else if (ns == 3) INC_D2R(true, 3, 0)
  else if (abl == 4) INC_D2R(true, 4, 4)     /* no x LDS-DMA */
  else if (abl == 8) INC_D2R(true, 4, 8)     /* no W loads */
  else if (abl == 12) INC_D2R(true, 4, 12)   /* no global traffic */
  else if (abl == 76) INC_D2R(true, 4, 76)   /* no global traffic, no barrier */
  else if (abl == 128) INC_D2R(true, 4, 128) /* no epilogue stores */
  else if (abl == 256) INC_D2R(true, 4, 256) /* per-workgroup time stamps */
  else if (abl == 260) INC_D2R(true, 4, 260) /* ... of the timing-only ablations */
  else if (abl == 264) INC_D2R(true, 4, 264)
  else if (abl == 268) INC_D2R(true, 4, 268)
  else if (abl == 332) INC_D2R(true, 4, 332)
  else if (abl == 320) INC_D2R(true, 4, 320) /* no barrier only */
  else if (abl == 768) INC_D2R(true, 4, 768) /* no scalar pointer arithmetic */
  else if (abl == 844) INC_D2R(true, 4, 844) /* no global traffic, no barrier, no pointer arithmetic */
#endif
  else INC_D2R(true, 4, 0)
#undef INC_D2R
  return 0;
}
