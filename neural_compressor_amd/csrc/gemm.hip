// gemm.hip -- K4: fused INT4/INT8 unpack + group-wise dequant + bf16/f16 MFMA GEMM.
//
// Replaces INCWeightOnlyLinear.forward (reference neural_compressor/torch/algorithms/weight_only/
// modules.py:594-610), which dequantises the whole weight with a Python loop (recover, :413-443), caches
// it dense and calls F.linear.  Here the dense weight never exists: packed words are read from HBM once,
// unpacked and scaled in registers, and fed to the matrix cores.
//
//   y[M,N] = x[M,K] . W^T + bias,   W[n,k] = rn16( int8(q[n,k] - zp[n,g]) * scale[n,g] )
//
// where rn16 rounds to the compute dtype (bf16 / f16), exactly what inc_woq_dequant produces, so
// y == F.linear(x, recover_in_that_dtype) up to fp32 accumulation order.
//
// Layout facts that shape the kernels (optimum format, modules.py:254-267):
//   qweight [K/8, N] int32 -- one word = 8 consecutive k of ONE output column n.  That is exactly one
//   lane's B-operand of v_mfma_f32_32x32x16_bf16 / 16x16x32 (8 k-values of column j), so a word is
//   dequantised straight into a B fragment with no cross-lane movement, and words are contiguous in n
//   so wave loads of qweight are full-line.
//
// This file decides and dispatches: woq_gemm_plan (host only) picks the kernel of a call, the three entry points check their arguments
// and launch what it says.  The kernels live one family per gemm_*.hip file, each behind a launcher: gemm_common.hpp lists them.
#include "gemm_common.hpp"

// 1: the direct-to-register kernel (gemm_d2r.hip) -- behind it, in the harness build, the producer / consumer kernel
// (tools/kbench_gemm_1.inc) -- takes the large-M 4-bit path whenever it applies
#ifndef INC_GEMM_DEFAULT_D2R
#define INC_GEMM_DEFAULT_D2R 1
#endif
#ifndef INC_GEMM_DEFAULT_PC
#define INC_GEMM_DEFAULT_PC 1
#endif

extern "C" {

// split-K plan of the 3A2B kernel for medium M: enough workgroups to cover the chip, slabs of >= 4 K-steps
static int big_splitk(int64_t M, int64_t N, int64_t K, int* steps_out) {
  const int64_t tiles = ceil_div64(M, TM) * ceil_div64(N, TN);
  const int nk = (int)(K / TK);
  int splits = 1;
  if (tiles < 192 && (K % 128) == 0 && (N % 4) == 0) {
    splits = (int)(256 / tiles);
    const int cap = tiles <= 16 ? 16 : 8;
    if (splits > cap) splits = cap;
    while (splits > 1 && (nk / splits) < 4) --splits;
  }
  int steps = (int)ceil_div64(nk, splits);
  steps += steps & 1;  // the K-loop is unrolled by two
  splits = (int)ceil_div64(nk, steps);
  *steps_out = steps;
  return splits;
}

// how far the streaming kernel's 8-bit form goes (GEMV_MAX_M for 4-bit words): up to 32 rows everywhere, up to 64 rows while N * K <= 2^25 -- measured against the 8-bit tile kernel
// (scripts/w8_gemm_time.py: 4096^2 M = 48 / 64: 17.3 / 18.5 vs 24.4 us; 11008 x 4096 M = 32: 18.7 vs 32.7 us, M = 48 / 64: 40.8 / 43.8 vs 32.7 us)
constexpr int64_t GEMV8_MAX_M = 64, GEMV8_WIDE_MAX_M = 32, GEMV8_WIDE_ELEMS = (int64_t)1 << 25;

// ---- routing: which kernel a call takes, decided once, on the host -----------------------------------------------------------------
// woq_gemm_plan is the ONLY place that decides; inc_woq_gemm launches what it says and inc_woq_gemm_route reports it (the route table
// of tests/test_gemm_routes_cpu.py pins every threshold below: a retuned one has to be acknowledged there).
// <woq-gemm-plan>
// harness-build routes (tools/kbench flags; never returned by libinc_mi355x.so)
constexpr int WOQ_ROUTE_DBG_PC = 100, WOQ_ROUTE_DBG_GEMV16_NT = 103, WOQ_ROUTE_DBG_STREAM_NT = 104;

// above 32 rows a layer of more than this many weights is the strip kernel's, not the streaming kernel's (M = 64, 11008 x 4096: 21 vs 29 us)
constexpr int64_t STRIP_PREF_ELEMS = (int64_t)24 << 20;
static bool strip_m(int64_t M, int64_t N, int64_t K) { return M > GEMV_MAX_M || (M > 32 && N * K > STRIP_PREF_ELEMS); }

// the streaming kernel's launch for M rows x `strips` 64-column strips (of one module or of a batch together) x K:
// 8 steps per wave when that still gives every SIMD two waves (>= 512 workgroups), else 4; row-blocked (M > 16) and 8-bit: always 4
struct StreamPlan { int steps, mb, splitk; };
static StreamPlan stream_plan(int64_t M, int64_t strips, int64_t K, int bits) {
  const bool vs4 = bits == 8 || M > 16 || (strips * ceil_div64(K, 2 * STREAM_SLICE_K) < 512 && ceil_div64(K, STREAM_SLICE_K) <= 64);
  const int steps = vs4 ? 4 : 8;
  return {steps, M > 32 ? 4 : M > 16 ? 2 : 1, (int)ceil_div64(K, STREAM_SLICE_K * steps / 4)};
}

struct WoqGemmPlan {
  int route = 0;
  int splitk = 1;          // K-slices launched
  int steps = 0;           // streaming: K-steps per wave (4 / 8); 256-row kernels: K-steps of TK per slab
  int mb = 0;              // streaming: 16-row blocks per workgroup
  int y_vec_ok = -1, x_vec_ok = -1;
  int g_shift = -2;        // group lookup by shift: log2(group_size), -1 = one group, -2 = not a power of two >= 32
  int kw_per_slice = 0;    // small kernel: packed rows per K-slice
  int64_t need = 0;        // workspace bytes the route uses when it is given enough
};

// of x / y / bias only the alignment is used, of workspace only whether it is NULL: nothing is dereferenced, no HIP call is made
static int woq_gemm_plan(int64_t M, int64_t N, int64_t K, int group_size, int bits, int xdtype, bool has_g_idx, uintptr_t x, uintptr_t y,
                         uintptr_t bias, bool has_ws, int64_t workspace_bytes, WoqGemmPlan* p) {
  if (bits < 1 || bits > 8) return INC_ERR_UNSUPPORTED;
  // g_idx (per-element groups: GPTQ act_order / HF desc_act): the general tile kernel and the small kernel look the group up per k; every
  // other kernel assumes contiguous groups (the module sorts K by group once and calls them without g_idx, modules.py)
  if (!(xdtype == INC_BF16 || xdtype == INC_F16)) return INC_ERR_UNSUPPORTED;
  const int np = 32 / bits;
  // a packed word must not straddle two groups unless g_idx is given per element... (word-granular
  // group lookup): require group boundaries on word boundaries.
  const bool anyw = !(bits == 4 || bits == 8);  // 1 / 2 / 3 / 5 / 6 / 7 bits: the tile kernel's per-element form, any group_size
  if (!anyw && !has_g_idx && (group_size % np) != 0 && group_size < K) return INC_ERR_UNSUPPORTED;
  if (anyw && K >= ((int64_t)1 << 31)) return INC_ERR_UNSUPPORTED;
  const int g_shift = p->g_shift = g_shift_of(group_size, K);
  const bool x16 = (x & 15) == 0;
  const int64_t slices512 = ceil_div64(K, STREAM_SLICE_K);  // K-slices of the streaming kernel at 4 steps per wave (<= 64 for its row-blocked form)
  const int dbg = inc_small_tiles_flag(-1);
  // 4-bit, M <= 64: the streaming kernel (16 < M <= 64 while its K-slices fit the plan, else a 256-row kernel with most rows clamped)
  const bool gemv_ok = !has_g_idx && bits == 4 && g_shift != -2 && (K % 32) == 0 && (N % 4) == 0 && N >= 64 && ceil_div64(N, 64) * 4 <= WS_COUNTER_BYTES &&
                       x16 && !inc_force_small_tiles() && M <= GEMV_MAX_M && dbg != 42;
  const bool big_ok = !has_g_idx && bits == 4 && (K % TK) == 0 && g_shift != -2 && M > 16 && N >= 64 && !(gemv_ok && slices512 <= 64) &&
                      x16 && N * (K / 8) < (int64_t)1 << 31;
  // weight-only INT8 at M <= 64: the streaming kernel's 8-bit form (M <= 16 whatever K; 16 < M <= 64 while its K-slices fit the counters' plan);
  // above that the 3A2B kernel's 8-bit instantiation, same tiling and split-K plan as the 4-bit one
  const bool gemv8_ok = !has_g_idx && bits == 8 && g_shift != -2 && (K % 32) == 0 && (N % 4) == 0 && N >= 64 && M <= GEMV8_MAX_M && dbg == 0 &&
                        (M <= GEMV8_WIDE_MAX_M || N * K <= GEMV8_WIDE_ELEMS) && (M <= 16 || slices512 <= 64) && ceil_div64(N, 64) * 4 <= WS_COUNTER_BYTES && x16;
  const bool big8_ok = !gemv8_ok && !has_g_idx && bits == 8 && (K % 128) == 0 && g_shift != -2 && M > 16 && N >= 64 && dbg == 0 &&
                       x16 && N * (K / 4) < (int64_t)1 << 31;
  if (anyw) {
    p->route = INC_WOQ_ROUTE_TILE_ANYW;
    p->x_vec_ok = (K % 8 == 0) && x16;
    return INC_OK;
  }
  // 64 < M <= 1024 with at most 64 tiles of 256 x 256: the strip kernels (no 256-row tiles, no slab passes).  With more tiles the
  // 256-row kernels fill the chip with <= 2 slabs and win (M = 512, N = 11008: 71 vs 81 us; tools/kbench strip).
  // 32 < M <= 64 on the larger layers too (M = 64, 11008 x 4096: 21 vs 29 us for the streaming kernel, whose x fragments are
  // per-lane 16-byte gathers; at 4096^2 the streaming kernel keeps a 1 us lead).  Harness flags 42 / 40 / 4 / 6 select the tile paths, 83 this kernel for any M > 16.
  const bool strip_ok = !has_g_idx && bits == 4 && g_shift != -2 && (K % 32) == 0 && (N % 4) == 0 && N >= 64 && (strip_m(M, N, K) || (dbg == 83 && M > 16)) && M <= STRIP_MAX_M &&
                        ceil_div64(M, TM) * ceil_div64(N, TN) <= 64 && x16 && (y & 7) == 0 &&
                        (bias & 7) == 0 && (dbg == 0 || (dbg >= 83 && dbg <= 89) || (dbg >= 100 && dbg <= 102));
  // the 256-row kernels' split-K plan: slabs only with 8-byte stores possible and a workspace that holds them
  auto slab_plan = [&](int y_vec_bit) {
    p->steps = (int)(K / TK);
    const int want = big_splitk(M, N, K, &p->steps);
    if (want > 1) {
      p->need = WS_COUNTER_BYTES + (int64_t)want * M * N * 4;
      if (y_vec_bit && has_ws && workspace_bytes >= p->need) p->splitk = want;
      else p->steps = (int)(K / TK);  // no workspace given: single pass (still correct, fewer workgroups)
    }
  };
  auto stream = [&]() {
    const StreamPlan sp = stream_plan(M, ceil_div64(N, 64), K, bits);
    p->steps = sp.steps, p->mb = sp.mb, p->splitk = sp.splitk;
    p->need = WS_COUNTER_BYTES + (int64_t)p->splitk * M * N * 4;
  };
  if (strip_ok && dbg == 0 && M > 128 && M * N < ((int64_t)1 << 30) && inc_woq_gemm_strip8_splitk(M, N, K) == 1) {
    // enough 128 x 128 tiles to fill the chip without K-slices (>= 192): the four-wave kernel that dequantises every weight once per
    // 128 rows (gemm_strip8.hip).  tools/midm_lab, 4096 x 4096: M = 1024 46 vs 57 us; 11008 x 4096, M = 256: 40 vs 48 us.  With K-slices
    // its larger partial tiles lose to the 64-row strips below (M = 512: 34 vs 30 us), so those keep this kernel's predecessor.
    p->route = INC_WOQ_ROUTE_STRIP8;
  } else if (strip_ok && M * N < ((int64_t)1 << 30)) {
    p->route = INC_WOQ_ROUTE_STRIP;
    const int want = inc_woq_gemm_strip_splitk(M, N, K);
    const int64_t wgs = ceil_div64(M, 64) * ceil_div64(N, 128);
    if (want > 1 && wgs * 4 <= WS_COUNTER_BYTES) {
      p->need = WS_COUNTER_BYTES + (int64_t)want * M * N * 4;
      if (has_ws && workspace_bytes >= p->need) p->splitk = want;
    }
  } else if (big8_ok) {
    p->route = INC_WOQ_ROUTE_3A2B_W8;
    p->y_vec_ok = (N % 4 == 0) && ((y & 7) == 0);
    slab_plan(p->y_vec_ok);
  } else if (big_ok && (K % 128) == 0 && (g_shift == -1 || g_shift >= 6) && (N % 2) == 0 && ((dbg == 0 && INC_GEMM_DEFAULT_D2R) || (dbg >= 90 && dbg <= 99))) {
    // weights direct to registers (gemm_d2r.hip): four waves, one per SIMD, no dequantised tile in LDS
    p->route = INC_WOQ_ROUTE_D2R;
    // bit 0: 8-byte stores possible; bit 1: 16-byte stores possible
    p->y_vec_ok = (((N % 4 == 0) && ((y & 7) == 0)) ? 1 : 0) | (((N % 8 == 0) && ((y & 15) == 0)) ? 2 : 0);
    slab_plan(p->y_vec_ok & 1);
#ifdef INC_KBENCH
  } else if (big_ok && (K % 128) == 0 && (g_shift == -1 || g_shift >= 6) && (dbg == 0 || dbg == 42 || (dbg >= 51 && dbg <= 74)) && INC_GEMM_DEFAULT_PC) {
    p->route = WOQ_ROUTE_DBG_PC;  // harness: the producer / consumer kernel (tools/kbench_gemm_2.inc)
    p->y_vec_ok = (((N % 4 == 0) && ((y & 7) == 0)) ? 1 : 0) | (((N % 8 == 0) && ((y & 15) == 0)) ? 2 : 0);
    slab_plan(p->y_vec_ok & 1);
#endif
  } else if (big_ok && (K % 128) == 0 && (dbg == 0 || dbg == 40 || dbg == 4 || dbg == 6 || (dbg >= 20 && dbg <= 30) || (dbg >= 31 && dbg <= 37))) {
    // what the direct-to-register kernel does not take: groups of 32 (two scales per K-step) and odd N
    p->route = INC_WOQ_ROUTE_3A2B_W4;
    p->y_vec_ok = (N % 4 == 0) && ((y & 7) == 0);
    slab_plan(p->y_vec_ok);
  } else if (big_ok && !inc_force_small_tiles()) {
    p->route = INC_WOQ_ROUTE_BIG;  // K % 128 == 64: the two-stage 256x256 kernel, K-steps of 64, no split-K
    p->y_vec_ok = (N % 4 == 0) && ((y & 7) == 0);
  } else if (M > 16 && !gemv8_ok && !(gemv_ok && slices512 <= 64)) {
    p->route = INC_WOQ_ROUTE_TILE;
    p->x_vec_ok = (K % 8 == 0) && x16;
#ifdef INC_KBENCH
  } else if (gemv_ok && M <= 16 && K <= GEMV16_MAX_K && xdtype == INC_BF16 && dbg == 103) {  // harness: the no-split decode kernel with non-temporal weight loads
    p->route = WOQ_ROUTE_DBG_GEMV16_NT;
  } else if (gemv_ok && M <= 16 && xdtype == INC_BF16 && dbg == 104 && (g_shift == -1 || g_shift >= 7)) {  // harness: the streaming kernel, non-temporal weight loads
    p->route = WOQ_ROUTE_DBG_STREAM_NT;
    stream();
#endif
  } else if (gemv_ok && M <= 16 && K <= GEMV16_MAX_K && (dbg == 85 || (dbg == 0 && M <= 4 && N <= 4096 && K <= 4096))) {
    // decode without split-K: one workgroup of 16 waves per 16 columns, the whole of K.  Wins where its N / 16 workgroups are a
    // single round on the chip and x is <= 4 rows (M = 1, 4096^2: 5.9 vs 6.8 us); elsewhere the streaming kernel's 64-column
    // requests and K-slices use the HBM better (M = 1, 11008 x 4096: 8.5 vs 15.9 us; tools/kbench decode; harness flag 85 forces it)
    p->route = INC_WOQ_ROUTE_GEMV16;
  } else if (gemv_ok && (M <= 16 || slices512 <= 64)) {
    p->route = INC_WOQ_ROUTE_STREAM_W4;
    stream();
  } else if (gemv8_ok) {
    // weight-only INT8 decode (BASELINE config #1's format): the streaming kernel's 8-bit form -- 64-column strips x K-slices of 512 k,
    // every wave's 8 KiB of packed weights requested before the first use, same hand-off.  (The generic split-K kernel it replaces
    // here read 16.8 MB in 20.6 us at 4096^2 and 45 MB in 46.7 us at 11008 x 4096: scripts/w8_gemm_time.py.)
    p->route = INC_WOQ_ROUTE_STREAM_W8;
    stream();
  } else {
    p->route = INC_WOQ_ROUTE_SMALL;
    p->splitk = inc_woq_gemm_small_slices(N, K, bits, &p->kw_per_slice);
    p->need = WS_COUNTER_BYTES + (int64_t)p->splitk * M * N * 4;
  }
  return INC_OK;
}
// </woq-gemm-plan>

int inc_woq_gemm_route(int64_t M, int64_t N, int64_t K, int group_size, int bits, int xdtype, int has_g_idx, const void* x,
                       const void* y, const void* bias, const void* workspace, int64_t workspace_bytes, int* splitk,
                       int* row_blocks, int* steps, int* y_vec_ok, int* x_vec_ok, int64_t* workspace_need) {
  INC_CHECK_ARG(M > 0 && N > 0 && K > 0 && group_size > 0);
  WoqGemmPlan p;
  const int rc = woq_gemm_plan(M, N, K, group_size, bits, xdtype, has_g_idx != 0, reinterpret_cast<uintptr_t>(x), reinterpret_cast<uintptr_t>(y),
                               reinterpret_cast<uintptr_t>(bias), workspace != nullptr, workspace_bytes, &p);
  if (rc != INC_OK) return rc;
  if (splitk) *splitk = p.splitk;
  if (row_blocks) *row_blocks = p.mb;
  if (steps) *steps = p.steps;
  if (y_vec_ok) *y_vec_ok = p.y_vec_ok;
  if (x_vec_ok) *x_vec_ok = p.x_vec_ok;
  if (workspace_need) *workspace_need = p.need;
  return p.route;
}

int64_t inc_woq_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  // an upper bound over the routes inc_woq_gemm can take for (M, N, K) (it does not know bits / group size here)
  int64_t need = 0;
  auto at_least = [&](int64_t v) { if (v > need) need = v; };
  if (M > 16) {
    // 256-row tiles (direct-to-register, 3A2B incl. its 8-bit form): split-K slabs behind the counter block.  They split only K % 128 == 0
    // (big_splitk divides by K / 64: K < 64 must not reach it)
    if (N >= 64 && (K % 128) == 0) {
      int steps;
      const int splits = big_splitk(M, N, K, &steps);
      if (splits > 1) at_least(WS_COUNTER_BYTES + (int64_t)splits * M * N * 4);
    }
    // the strip kernel, where inc_woq_gemm routes to it, with the K-slices it would use
    if (strip_m(M, N, K) && M <= STRIP_MAX_M && N >= 64 && (K % 32) == 0 && ceil_div64(M, TM) * ceil_div64(N, TN) <= 64) {
      const int sk = inc_woq_gemm_strip_splitk(M, N, K);
      if (sk > 1) at_least(WS_COUNTER_BYTES + (int64_t)sk * M * N * 4);
    }
    if (M <= GEMV_MAX_M) at_least(WS_COUNTER_BYTES + ceil_div64(K, STREAM_SLICE_K) * M * N * 4);  // streaming kernel, 4 steps per wave
    return need;
  }
  int64_t slices = ceil_div64(K, STREAM_SLICE_K);  // the streaming kernel at 4 steps per wave
  if (slices < 64) slices = 64;                 // the generic split-K path uses up to 64 slices
  return WS_COUNTER_BYTES + slices * M * N * 4;
}

int inc_woq_gemm(const void* x, int xdtype, const int32_t* qweight, const uint16_t* scales,
                 const int32_t* qzeros, const int32_t* g_idx, const void* bias, void* y, int64_t M,
                 int64_t N, int64_t K, int64_t G, int group_size, int bits, void* workspace,
                 int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && qweight && scales && qzeros && y && M > 0 && N > 0 && K > 0 && G > 0 && group_size > 0);
  // the kernel, its K-slices and its store / load forms: decided by woq_gemm_plan (above), launched here
  WoqGemmPlan plan;
  const int plan_rc = woq_gemm_plan(M, N, K, group_size, bits, xdtype, g_idx != nullptr, reinterpret_cast<uintptr_t>(x), reinterpret_cast<uintptr_t>(y),
                                    reinterpret_cast<uintptr_t>(bias), workspace != nullptr, workspace_bytes, &plan);
  if (plan_rc != INC_OK) return plan_rc;
  const int route = plan.route;
  const WoqGemmArgs a = {(const uint16_t*)x, (const uint32_t*)qweight, scales, (const uint32_t*)qzeros, (const uint16_t*)bias, (uint16_t*)y,
                         M, N, K, ceil_div64(N, 32 / bits), plan.g_shift, xdtype == INC_BF16, inc_s(stream)};
  const int dbg = inc_small_tiles_flag(-1);  // harness build: which A/B partner or ablation of the chosen route to launch (0 in the product)
  // the routes that cannot run without their K-slices
  const bool streams = route == INC_WOQ_ROUTE_STREAM_W4 || route == INC_WOQ_ROUTE_STREAM_W8 || route == WOQ_ROUTE_DBG_STREAM_NT;
  if ((streams || route == INC_WOQ_ROUTE_SMALL) && (!workspace || workspace_bytes < plan.need)) return INC_ERR_WORKSPACE;
  // the fp32 partials sit behind the counter block; the strip / 256-row kernels get them only when the plan has K-slices
  const auto [counters, part] = ws_parts(workspace);
  float* const slabs = plan.splitk > 1 ? part : nullptr;
  switch (route) {
    case INC_WOQ_ROUTE_TILE_ANYW:
    case INC_WOQ_ROUTE_TILE: return inc_launch_woq_gemm_tile(a, g_idx, bits, group_size, plan.x_vec_ok);
    case INC_WOQ_ROUTE_STRIP8: return inc_launch_woq_gemm_strip8(a, nullptr, nullptr, 1);
    case INC_WOQ_ROUTE_STRIP: return inc_launch_woq_gemm_strip(a, slabs, counters, plan.splitk, dbg);
    case INC_WOQ_ROUTE_3A2B_W8:
    case INC_WOQ_ROUTE_3A2B_W4: return inc_launch_woq_gemm_3a2b(a, bits, plan.y_vec_ok, slabs, plan.steps, plan.splitk, dbg);
    case INC_WOQ_ROUTE_D2R: {
      static const int d2r_abl[10] = {0, 0, 4, 8, 12, 76, 128, 0, 256, 0};  // harness flags 90..96 (91: three x stages; 92..96 timing-only), 98: time stamps
      const int abl = dbg >= 90 ? d2r_abl[dbg - 90] : 0;
#ifdef INC_KBENCH
      // harness flag 97: the eight-wave form (gemm_d2r8.hip, two waves per SIMD with redundant dequantisation): bit-identical and 6 %
      // SLOWER (1203 vs 1284 TFLOP/s at 4096^3, profiles/r3h_kbench_d2r8.log) -- built into the harness library only
      if (dbg == 97) (void)inc_launch_woq_gemm_d2r8(a, plan.y_vec_ok, slabs, plan.steps, plan.splitk);
      else
#endif
        (void)inc_launch_woq_gemm_d2r(a, plan.y_vec_ok, slabs, plan.steps, plan.splitk, dbg == 91 ? 3 : 4, abl);
      if (slabs) return inc_launch_slab_reduce(a, slabs, plan.splitk);
      INC_LAUNCH_RETURN();
    }
    case INC_WOQ_ROUTE_BIG: return inc_launch_woq_gemm_big(a, plan.y_vec_ok);
    case INC_WOQ_ROUTE_GEMV16: return inc_launch_woq_gemv16(a, nullptr, false);
    case INC_WOQ_ROUTE_STREAM_W4:
    case INC_WOQ_ROUTE_STREAM_W8:
    case WOQ_ROUTE_DBG_STREAM_NT: {  // (the last: harness, non-temporal weight loads)
      StreamLaunch l = {a.x, M, K, a.g_shift, a.bf, a.s, bits, plan.steps, plan.mb, plan.splitk, ceil_div64(N, 64), part, counters, &a};
      l.nt = route == WOQ_ROUTE_DBG_STREAM_NT;
      return inc_launch_woq_gemv_stream(l);
    }
#ifdef INC_KBENCH
    case WOQ_ROUTE_DBG_PC: return inc_launch_woq_gemm_pc(a, plan.y_vec_ok, slabs, plan.steps, plan.splitk, dbg);  // tools/kbench_gemm_2.inc
    case WOQ_ROUTE_DBG_GEMV16_NT: return inc_launch_woq_gemv16(a, nullptr, true);
#endif
    default: return inc_launch_woq_gemm_small(a, g_idx, bits, group_size, part, plan.splitk, plan.kw_per_slice);  // INC_WOQ_ROUTE_SMALL
  }
}

// ---- act_order decode in one launch: y = x[:, k_order] W_sorted^T + bias ------------------------------------------------------
// The plan is woq_gemm_plan's for the same shape without g_idx and a 16-byte aligned x (the gathered x is read 2 bytes at a time);
// only the three streaming routes have a PERM form, everything else is the caller's index_select + inc_woq_gemm.
int inc_woq_gemm_perm(const void* x, int xdtype, const int32_t* k_order, const int32_t* qweight, const uint16_t* scales,
                      const int32_t* qzeros, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int64_t G,
                      int group_size, int bits, void* workspace, int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && k_order && qweight && scales && qzeros && y && M > 0 && N > 0 && K > 0 && G > 0 && group_size > 0);
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 1) == 0);
  if ((reinterpret_cast<uintptr_t>(k_order) & 15) != 0 || M * K >= ((int64_t)1 << 31)) return INC_ERR_UNSUPPORTED;  // (x by 32-bit byte offsets)
  WoqGemmPlan plan;
  const int plan_rc = woq_gemm_plan(M, N, K, group_size, bits, xdtype, false, 0, reinterpret_cast<uintptr_t>(y), reinterpret_cast<uintptr_t>(bias),
                                    workspace != nullptr, workspace_bytes, &plan);
  if (plan_rc != INC_OK) return plan_rc;
  const int route = plan.route;
  if (route != INC_WOQ_ROUTE_GEMV16 && route != INC_WOQ_ROUTE_STREAM_W4 && route != INC_WOQ_ROUTE_STREAM_W8) return INC_ERR_UNSUPPORTED;
  if (route != INC_WOQ_ROUTE_GEMV16 && (!workspace || workspace_bytes < plan.need)) return INC_ERR_WORKSPACE;
  const WoqGemmArgs a = {(const uint16_t*)x, (const uint32_t*)qweight, scales, (const uint32_t*)qzeros, (const uint16_t*)bias, (uint16_t*)y,
                         M, N, K, ceil_div64(N, 32 / bits), plan.g_shift, xdtype == INC_BF16, inc_s(stream)};
  if (route == INC_WOQ_ROUTE_GEMV16) return inc_launch_woq_gemv16(a, k_order, false);
  const auto [counters, part] = ws_parts(workspace);
  StreamLaunch l = {a.x, M, K, a.g_shift, a.bf, a.s, bits, plan.steps, plan.mb, plan.splitk, ceil_div64(N, 64), part, counters, &a};
  l.k_order = k_order;
  return inc_launch_woq_gemv_stream(l);
}

// ---- modules that share x, one launch (decode: q / k / v, gate / up) -----------------------------------------------------------
// plan of the batched streaming launch: strips of 64 columns per module, VSTEPS by the rule inc_woq_gemm applies to ONE module with
// the modules' columns together -> the launch is bit-identical to inc_woq_gemm on the N-concatenated module (strips are independent)
static bool gemv_multi_plan(int n, int64_t M, const int64_t* N, int64_t K, int group_size, int bits, int* g_shift_out, StreamPlan* sp_out,
                            int64_t* strips_out) {
  if (n < 2 || n > GEMV_MAX_BATCH || !(bits == 4 || (bits == 8 && M <= 16)) || M < 1 || M > GEMV_MAX_M || K <= 0 || (K % 32) != 0) return false;
  const int g_shift = g_shift_of(group_size, K);
  if (g_shift == -2) return false;
  int64_t strips = 0, ntot = 0;
  for (int i = 0; i < n; ++i) {
    if (N[i] < 64 || (N[i] % 4) != 0) return false;
    strips += ceil_div64(N[i], 64);
    ntot += N[i];
  }
  if (strips * 4 > WS_COUNTER_BYTES) return false;
  if (M > 16 && ceil_div64(K, STREAM_SLICE_K) > 64) return false;  // (row-blocked form: the single call takes a tile kernel there)
  if (strip_m(M, ntot, K)) return false;                            // inc_woq_gemm prefers the strip kernel there
  *g_shift_out = g_shift;
  *sp_out = stream_plan(M, strips, K, bits);
  *strips_out = strips;
  return true;
}

int64_t inc_woq_gemm_multi_workspace_bytes(int n, int64_t M, const int64_t* N, int64_t K) {
  if (n < 1 || !N) return 0;
  int64_t ntot = 0;
  for (int i = 0; i < n; ++i) ntot += N[i];
  return WS_COUNTER_BYTES + ceil_div64(K, STREAM_SLICE_K) * M * ntot * 4;  // 4 steps per wave: the most slices either form uses
}

// the plain batch (k_order == NULL: inc_woq_gemm_multi) and the gathered one (inc_woq_gemm_multi_perm: one order per member, x read 2
// bytes at a time through 32-bit byte offsets): the same plan, the same rung, the PERM instantiation of the same body
static int woq_gemm_multi_launch(int n, const void* x, int xdtype, const int32_t* const* k_order, const int32_t* const* qweight,
                                 const uint16_t* const* scales, const int32_t* const* qzeros, const void* const* bias, void* const* y, int64_t M,
                                 const int64_t* N, int64_t K, int group_size, int bits, void* workspace, int64_t workspace_bytes, inc_stream_t stream) {
  if (!(xdtype == INC_BF16 || xdtype == INC_F16)) return INC_ERR_UNSUPPORTED;
  int g_shift;
  StreamPlan sp;
  int64_t strips;
  if (!gemv_multi_plan(n, M, N, K, group_size, bits, &g_shift, &sp, &strips)) return INC_ERR_UNSUPPORTED;  // nothing launched: the caller issues inc_woq_gemm per module
  if (k_order ? M * K >= ((int64_t)1 << 31) : (reinterpret_cast<uintptr_t>(x) & 15) != 0) return INC_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) {
    INC_CHECK_ARG(qweight[i] && scales[i] && qzeros[i] && y[i]);
    if (k_order) {
      INC_CHECK_ARG(k_order[i]);
      if ((reinterpret_cast<uintptr_t>(k_order[i]) & 15) != 0) return INC_ERR_UNSUPPORTED;
    }
  }
  GemvBatch args;
  const int64_t floats = gemv_batch_fill(&args, n, k_order, qweight, scales, qzeros, bias, y, sp.splitk, M, N).floats;
  if (!workspace || workspace_bytes < WS_COUNTER_BYTES + floats * 4) return INC_ERR_WORKSPACE;
  const auto [counters, part] = ws_parts(workspace);
  StreamLaunch l = {(const uint16_t*)x, M, K, g_shift, xdtype == INC_BF16, inc_s(stream), bits, sp.steps, sp.mb, sp.splitk, strips, part, counters};
  l.batch = &args;
  l.batch_perm = k_order != nullptr;
  return inc_launch_woq_gemv_stream(l);
}

int inc_woq_gemm_multi(int n, const void* x, int xdtype, const int32_t* const* qweight, const uint16_t* const* scales,
                       const int32_t* const* qzeros, const void* const* bias, void* const* y, int64_t M, const int64_t* N, int64_t K,
                       int group_size, int bits, void* workspace, int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && qweight && scales && qzeros && y && N && n > 0 && M > 0 && K > 0 && group_size > 0);
  return woq_gemm_multi_launch(n, x, xdtype, nullptr, qweight, scales, qzeros, bias, y, M, N, K, group_size, bits, workspace, workspace_bytes, stream);
}

// ---- act_order members in the batched launch: y[i] = x[:, k_order[i]] W_sorted_i^T + bias_i ------------------------------------
int inc_woq_gemm_multi_perm(int n, const void* x, int xdtype, const int32_t* const* k_order, const int32_t* const* qweight,
                            const uint16_t* const* scales, const int32_t* const* qzeros, const void* const* bias, void* const* y, int64_t M,
                            const int64_t* N, int64_t K, int group_size, int bits, void* workspace, int64_t workspace_bytes,
                            inc_stream_t stream) {
  INC_CHECK_ARG(x && k_order && qweight && scales && qzeros && y && N && n > 0 && M > 0 && K > 0 && group_size > 0);
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 1) == 0);
  return woq_gemm_multi_launch(n, x, xdtype, k_order, qweight, scales, qzeros, bias, y, M, N, K, group_size, bits, workspace, workspace_bytes, stream);
}

// ---- gate / up of a dense MLP with the SiLU product in the same launch: h = silu(x Wg^T) * (x Wu^T) ----------------------------
// The batched launch over the two members (gemv_multi_plan for N, N), one row block; the strips of gate and up share a ticket and the
// last arriver forms the product from the two fixed-order fp32 sums (gemm_stream.hip, GATED).
constexpr int64_t GATED_MAX_M = 16;

int64_t inc_woq_gemm_gated_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return WS_COUNTER_BYTES + ceil_div64(K, STREAM_SLICE_K) * M * 2 * N * 4;  // 4 steps per wave: the most slices; both members' slabs
}

int inc_woq_gemm_gated(const void* x, int xdtype, const int32_t* k_order_gate, const int32_t* k_order_up, const int32_t* gate_qweight,
                       const uint16_t* gate_scales, const int32_t* gate_qzeros, const int32_t* up_qweight, const uint16_t* up_scales,
                       const int32_t* up_qzeros, void* h, int64_t M, int64_t N, int64_t K, int group_size, int bits, int act, void* workspace,
                       int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && gate_qweight && gate_scales && gate_qzeros && up_qweight && up_scales && up_qzeros && h && M > 0 && N > 0 && K > 0 && group_size > 0);
  INC_CHECK_ARG((k_order_gate == nullptr) == (k_order_up == nullptr));
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 1) == 0);
  if (!(xdtype == INC_BF16 || xdtype == INC_F16) || bits != 4 || act != 0 || M > GATED_MAX_M) return INC_ERR_UNSUPPORTED;
  const bool perm = k_order_gate != nullptr;
  const int64_t NN[2] = {N, N};
  int g_shift;
  StreamPlan sp;
  int64_t strips;
  if (!gemv_multi_plan(2, M, NN, K, group_size, bits, &g_shift, &sp, &strips)) return INC_ERR_UNSUPPORTED;
  if (perm ? (M * K >= ((int64_t)1 << 31) || ((reinterpret_cast<uintptr_t>(k_order_gate) | reinterpret_cast<uintptr_t>(k_order_up)) & 15) != 0)
           : (reinterpret_cast<uintptr_t>(x) & 15) != 0)
    return INC_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < WS_COUNTER_BYTES + (int64_t)sp.splitk * M * 2 * N * 4) return INC_ERR_WORKSPACE;
  GemvBatch args = {};
  args.n = 2;
  args.k_order[0] = k_order_gate, args.k_order[1] = k_order_up;
  args.qweight[0] = (const uint32_t*)gate_qweight, args.qweight[1] = (const uint32_t*)up_qweight;
  args.scales[0] = gate_scales, args.scales[1] = up_scales;
  args.qzeros[0] = (const uint32_t*)gate_qzeros, args.qzeros[1] = (const uint32_t*)up_qzeros;
  args.y[0] = (uint16_t*)h;
  args.N[0] = args.N[1] = N;
  args.part_off[1] = (int64_t)sp.splitk * M * N;
  args.first[1] = (int)(strips / 2);
  for (int i = 2; i <= GEMV_MAX_BATCH; ++i) args.first[i] = (int)strips;
  const auto [counters, part] = ws_parts(workspace);
  StreamLaunch l = {(const uint16_t*)x, M, K, g_shift, xdtype == INC_BF16, inc_s(stream), bits, sp.steps, sp.mb, sp.splitk, strips, part, counters};
  l.batch = &args;
  l.batch_perm = perm;
  l.gated = true;
  return inc_launch_woq_gemv_stream(l);
}

}  // extern "C"
