// gemm_stream.hip -- the decode kernels of the fused dequant-GEMM (inc_woq_gemm, gemm.hip), M <= 64: the streaming GEMV in its plain,
// gathered (inc_woq_gemm_perm), batched (inc_woq_gemm_multi, gathered: inc_woq_gemm_multi_perm) and gated (inc_woq_gemm_gated) forms,
// which share one body and ONE launch ladder below, and the no-split kernel for M <= 16 on small layers.
#include "gemm_common.hpp"

namespace {

// ---- the streaming kernel (K % 32 == 0, N % 4 == 0, group lookup by shift): HBM-bound -----------------------------------------------
// The whole packed matrix is only N*K/2 bytes (8 MiB at 4096^2), a few microseconds of HBM time, so the
// kernel is built around memory-level parallelism: a wave owns 64 columns x 256 k and issues ALL of its
// weight traffic (8 x 16 B per lane = 8 KiB per wave) before it touches any of it; 4 waves of a workgroup
// take 4 consecutive k-ranges of the same 64-column strip (1024 k), grid = strips x K/1024 workgroups
// (256 at 4096^2: one per CU).  x is the 16-row A operand of v_mfma_f32_16x16x32 (rows >= M zeroed), each
// lane's 16-byte weight load is 4 adjacent columns = 4 B operands (output column 4*(lane&15)+c).
// Reduction: the 4 waves add through LDS; across workgroups each writes its fp32 partial strip, then the
// LAST workgroup to arrive on the strip's counter sums the partials in a fixed order, adds the bias, converts
// and stores -> one launch, deterministic.  The counters live in the caller's workspace, must be zero on entry
// and are returned to zero by the last arriver.  All of that -- the output map and bias prefetch (StripOut), the
// four-wave sum, the partial store, the hand-off (splitk_arrive) and the slice sum -- is strip_finish and its
// pieces in gemm_common.hpp, shared with gemm_anyw.hip; the body below ends in it, the gated pair in a tail of its
// own built from the same pieces.  The hand-off in one line: write-through (`sc1`) partial stores -> every wave
// drains them -> barrier -> ONE relaxed agent-scope ticket; the last arriver reads the slabs with `sc1` loads, so
// neither side needs an agent-scope fence (the release / acquire pair this replaced cost
// ~3.4 us of an 8.4 us kernel).  VSTEPS = MFMA K=32 steps per wave: 8 (a wave streams 8 KiB of weights) for large matrices,
// 4 when that would leave CUs without a workgroup or SIMDs with a single wave (the dequantisation arithmetic of a wave is a
// serial ~60-instruction chain per step).
constexpr int VS = 8;   // largest VSTEPS (sizes the workspace)
// MB = 16-row blocks of x per workgroup (M <= 16 * MB): batched decode (16 < M <= 64) streams the packed weights ONCE like the
// M <= 16 case -- every dequantised B fragment feeds MB MFMAs -- instead of parking a 256-row tile that is mostly clamped rows.
// NT (harness A/B, same results): the packed-weight requests carry the non-temporal hint -- every word is read once by one CU
// The body of one (64-column strip, K-slice) workgroup: `counter` is the strip's arrival counter, `partial` the module's slabs.
// BITS = 8 (weight-only INT8, round 6): a step's 32 k of four columns are TWO packed rows per lane (a word = 4 k of one column), the
// integer -> float step is the int8 wrap of dequant8_from_bytes (bit-identical to inc_woq_dequant); always 4 steps per wave, so a wave
// streams the same 8 KiB as the 4-bit form with 8 steps.  `NW` = words per row of qzeros (N / 8 for 4 bits, N / 4 for 8).
// PERM (inc_woq_gemm_perm: act_order modules, whose packed words are sorted along K by group once): the A operand of a step is
// x[row, k_order[k]] for the step's k instead of x[row, k] -- a lane reads its 8 entries of k_order (two 16-byte loads; k_order is
// 16-byte aligned and the offset a multiple of 8 entries), clamps them to [0, K-1] so that no array can send a read outside x, and
// packs eight 2-byte loads into the uint4 the plain form gets from one 16-byte load.  Nothing else differs: the same values reach
// the same MFMAs in the same order, so the result equals the plain form's on x.index_select(1, k_order) bit for bit.  x is at
// most 64 x K 16-bit values and is read by every workgroup: it stays in L2.
// Order of issue: the entries of k_order for all of a wave's steps first, then the weights, then the gathers -- vector loads
// return in order, so the gathers wait for the indices alone while the weights are on their way from HBM.  An index register is
// done once its gather is issued; x is addressed by 32-bit byte offsets (the entry point requires M * K < 2^31).  perm_load8 /
// perm_gather8 live in gemm_common.hpp: gemm_anyw.hip gathers the same way.

// GATED (inc_woq_gemm_gated: gate_proj / up_proj of a dense MLP, same N): the workgroup is strip `strip` of member `member` (0 = gate,
// 1 = up) and runs the body unchanged up to its fp32 strip sum.  Both members ALWAYS write that sum to their slabs
// partial[member][slice][M][N] (also with one K-slice), and strip j of gate and strip j of up share `counter`: the arriver with ticket
// 2 * splitk - 1 sums gate's slices in slice order, then up's -- the very sums the batched launch would have rounded -- and stores
// rx(g / (1 + expf(-g)) * u), the fp32 expression of gemm_moe.hip's mode 0.  The same hand-off (splitk_arrive), with twice the arrivals.
template <bool IS_BF16, bool G128, int VSTEPS, int MB, bool NT = false, int BITS = 4, bool PERM = false, bool GATED = false>
__device__ __forceinline__ void woq_gemv_w4_body(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counter, int M, int64_t N, int64_t K, int64_t NW,
    int g_shift, int splitk, int strip, int slice, const int32_t* __restrict__ k_order = nullptr, int member = 0) {
  static_assert(!GATED || (MB == 1 && BITS == 4 && !NT), "the gated pair: one row block of 4-bit words");
  constexpr int VS = VSTEPS;  // shadows the file-level maximum inside this kernel
  constexpr int ROWS = 16 * MB;
  constexpr int NOUT = ROWS * 64 / 256;  // outputs per thread of the strip
  __shared__ float red[4 * ROWS * 65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_u = fp8_unit_inverse();
  const int jn = lane & 15, oct = lane >> 4;
  const int64_t n0 = (int64_t)strip * 64;
  int64_t ncol = n0 + 4 * jn;
  if (ncol > N - 4) ncol = N - 4;  // clamped lanes recompute valid columns; their results are not stored
  const int steps_total = (int)(K / 32);
  const int step0 = (slice * 4 + wave) * VS;

  // ---- issue every load of this wave up front ---------------------------------------------------
  constexpr int WPS = BITS == 8 ? 2 : 1;  // 16-byte weight requests per lane and step
  static_assert(BITS == 4 || (BITS == 8 && !NT), "4- or 8-bit words");
  uint4 w[VS * WPS], a[MB][VS];
  PermIdx8 kraw[PERM ? VS : 1];
  if constexpr (PERM) {
#pragma unroll
    for (int s = 0; s < VS; ++s) {
      int st = step0 + s;
      if (st > steps_total - 1) st = steps_total - 1;  // (clamped like the weights' step: inside k_order)
      kraw[s] = perm_load8(k_order + (int64_t)st * 32 + 8 * oct);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int s = 0; s < VS; ++s) {
    int st = step0 + s;
    if (st > steps_total - 1) st = steps_total - 1;  // past-the-end steps re-read the last one and are zeroed via A
    if constexpr (BITS == 8) {
      w[2 * s] = *reinterpret_cast<const uint4*>(qweight + ((int64_t)st * 8 + 2 * oct) * N + ncol);
      w[2 * s + 1] = *reinterpret_cast<const uint4*>(qweight + ((int64_t)st * 8 + 2 * oct + 1) * N + ncol);
    } else if constexpr (NT) {
      typedef uint32_t nt_u32x4 __attribute__((ext_vector_type(4)));
      const nt_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u32x4*>(qweight + ((int64_t)st * 4 + oct) * N + ncol));
      w[s] = make_uint4(v.x, v.y, v.z, v.w);
    } else {
      w[s] = *reinterpret_cast<const uint4*>(qweight + ((int64_t)st * 4 + oct) * N + ncol);
    }
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const int am = 16 * b + jn < M ? 16 * b + jn : M - 1;  // A row (clamped; rows >= M are zeroed below)
      if constexpr (PERM) a[b][s] = perm_gather8(x, 2u * (uint32_t)am * (uint32_t)K, kraw[s], (int)(K - 1));
      else a[b][s] = *reinterpret_cast<const uint4*>(x + (int64_t)am * K + (int64_t)st * 32 + 8 * oct);
    }
  }
  // group parameters: G128 -> one group per 4 steps (step0 is a multiple of 4)
  constexpr int NG = G128 ? (VS + 3) / 4 : VS;
  uint2 sraw[NG];
  uint32_t zraw[NG];
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    int st = step0 + (G128 ? 4 * i : i);
    if (st > steps_total - 1) st = steps_total - 1;
    const int64_t g = g_shift >= 0 ? (((int64_t)st * 32) >> g_shift) : 0;
    sraw[i] = *reinterpret_cast<const uint2*>(scales + g * N + ncol);
    zraw[i] = qzeros[g * NW + (BITS == 8 ? (ncol >> 2) : (ncol >> 3))];
  }
  const int zsh = 4 * (int)(ncol & 7);  // ncol % 4 == 0: the 4 zero nibbles sit at bits zsh .. zsh+15
  // this thread's outputs of the strip and their bias, fetched now (scales: a valid address where there is no bias)
  StripOut<ROWS> out;
  strip_out_prefetch(out, tid, M, N, n0, bias, scales);
  __builtin_amdgcn_sched_barrier(0);  // everything above is in flight before the first use below

  f32x4 acc[MB][4];
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[b][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < VS; ++s) {
    const int gi = G128 ? (s >> 2) : s;
    const bool in_k = step0 + s < steps_total;
    uint4 av[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const bool live = in_k && (16 * b + jn < M);
      av[b] = a[b][s];
      av[b].x = live ? av[b].x : 0u; av[b].y = live ? av[b].y : 0u; av[b].z = live ? av[b].z : 0u; av[b].w = live ? av[b].w : 0u;
    }
    const uint32_t sw[2] = {sraw[gi].x, sraw[gi].y};
    const uint32_t ww[4] = {w[s * WPS].x, w[s * WPS].y, w[s * WPS].z, w[s * WPS].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float sc = f16_bits_to_f32((uint16_t)(sw[c >> 1] >> (16 * (c & 1))));
      if constexpr (BITS == 8) {
        const uint32_t wh[4] = {w[s * WPS + WPS - 1].x, w[s * WPS + WPS - 1].y, w[s * WPS + WPS - 1].z, w[s * WPS + WPS - 1].w};
        uint32_t z8 = ((zraw[gi] >> (8 * c)) & 255u) + 1u;  // ncol % 4 == 0: the word holds exactly this lane's four zero points
        z8 = z8 > 255u ? 0u : z8;
        const uint4 bq8 = dequant8_from_bytes<IS_BF16>(ww[c], wh[c], sc, (int)z8);
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[b][c] = mfma16<IS_BF16>(av[b], bq8, acc[b][c]);
        continue;
      }
      uint32_t zz = ((zraw[gi] >> (zsh + 4 * c)) & 15u) + 1u;
      zz = zz > 15u ? 0u : zz;
      const uint4 bq = dequant8<IS_BF16, 1>(ww[c], sc * inv_u, -(float)zz * sc);  // (packed fp32 FMAs: same values; with four MFMAs per step the VALU is the busy pipe here: - 5 % per launch, tools/gemv_lab)
#pragma unroll
      for (int b = 0; b < MB; ++b) acc[b][c] = mfma16<IS_BF16>(av[b], bq, acc[b][c]);
    }
  }
  // ---- reduce the 4 waves: D col = lane&15 -> column 4*jn + c, row m = 16*b + 4*oct + r ------------------
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * ROWS + 16 * b + 4 * oct + r) * 65 + 4 * jn + c] = acc[b][c][r];
  if constexpr (GATED) {  // both members always write their slabs; the last of the 2 * splitk arrivers forms the product
    float sum[NOUT], gs[NOUT], us[NOUT];
    strip_sum_waves<ROWS>(red, tid, sum);
    const int64_t slab = (int64_t)M * N;
    strip_store_partial<ROWS>(partial + ((int64_t)member * splitk + slice) * slab, out, sum);
    if (!splitk_arrive(counter, 2 * splitk, red)) return;
    splitk_sum_slices<NOUT>(partial, slab, splitk, out.off, gs);
    splitk_sum_slices<NOUT>(partial + (int64_t)splitk * slab, slab, splitk, out.off, us);
#pragma unroll
    for (int i = 0; i < NOUT; ++i)
      if (out.ok[i]) {
        const float g = gs[i], u = us[i];
        const float v = silu_mul_f32(g, u);
        y[out.off[i]] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
      }
  } else {
    strip_finish<IS_BF16, ROWS>(red, tid, out, bias, y, partial, counter, M, N, splitk, slice);
  }
}

template <bool IS_BF16, bool G128, int VSTEPS, int MB, bool NT = false, int BITS = 4>
__global__ __launch_bounds__(256) void woq_gemv_w4_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counters, int M, int64_t N, int64_t K, int64_t NW,
    int g_shift, int splitk) {
  woq_gemv_w4_body<IS_BF16, G128, VSTEPS, MB, NT, BITS>(x, qweight, scales, qzeros, bias, y, partial, counters + blockIdx.x, M, N, K, NW, g_shift, splitk,
                                                 (int)blockIdx.x, (int)blockIdx.y);
}

// the same workgroup with the activations gathered through k_order (PERM above)
template <bool IS_BF16, bool G128, int VSTEPS, int MB, int BITS = 4>
__global__ __launch_bounds__(256) void woq_gemv_w4_perm_kernel(
    const uint16_t* __restrict__ x, const int32_t* __restrict__ k_order, const uint32_t* __restrict__ qweight,
    const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias,
    uint16_t* __restrict__ y, float* __restrict__ partial, unsigned* __restrict__ counters, int M, int64_t N, int64_t K, int64_t NW,
    int g_shift, int splitk) {
  woq_gemv_w4_body<IS_BF16, G128, VSTEPS, MB, false, BITS, true>(x, qweight, scales, qzeros, bias, y, partial, counters + blockIdx.x, M, N, K, NW, g_shift,
                                                                 splitk, (int)blockIdx.x, (int)blockIdx.y, k_order);
}

// Several packed modules that multiply the SAME x (q / k / v of an attention block; gate / up of an MLP) in ONE launch
// (inc_woq_gemm_multi): a decode call of one module is ~2 us of streaming behind ~5 us of launch boundary, first-byte latency and
// split-K hand-off, and the modules of a group are independent given x.  The strips of the modules occupy consecutive ranges of
// blockIdx.x; every strip runs exactly the body above on its own module's tensors -> bit-identical to the single launches.
// PERM (inc_woq_gemm_multi_perm): member p's activations are gathered through args.k_order[p], as in woq_gemv_w4_perm_kernel -- an
// instantiation of its own (one body, one red[] per kernel), bit-identical to the plain one on x.index_select(1, k_order[p]).
template <bool IS_BF16, bool G128, int VSTEPS, int MB, int BITS = 4, bool PERM = false>
__global__ __launch_bounds__(256) void woq_gemv_w4_multi_kernel(GemvBatch args, const uint16_t* __restrict__ x, float* __restrict__ partial,
                                                                unsigned* __restrict__ counters, int M, int64_t K, int g_shift, int splitk) {
  const int b = (int)blockIdx.x;
  int p = 0;
#pragma unroll
  for (int i = 1; i < GEMV_MAX_BATCH; ++i)
    if (i < args.n && b >= args.first[i]) p = i;
  p = __builtin_amdgcn_readfirstlane(p);
  const int64_t N = args.N[p];
  woq_gemv_w4_body<IS_BF16, G128, VSTEPS, MB, false, BITS, PERM>(x, args.qweight[p], args.scales[p], args.qzeros[p], args.bias[p], args.y[p],
                                                                 partial + args.part_off[p], counters + b, M, N, K, BITS == 8 ? (N + 3) / 4 : (N + 7) / 8, g_shift,
                                                                 splitk, b - args.first[p], (int)blockIdx.y, PERM ? args.k_order[p] : nullptr);
}

// gate / up with the SiLU product in the same launch (inc_woq_gemm_gated; GATED above): blockIdx.x < strips is gate's strip, the rest
// up's; strip j of both arrives on counters[j], the output is args.y[0]
template <bool IS_BF16, bool G128, int VSTEPS, bool PERM>
__global__ __launch_bounds__(256) void woq_gemv_w4_gated_kernel(GemvBatch args, const uint16_t* __restrict__ x, float* __restrict__ partial,
                                                                unsigned* __restrict__ counters, int M, int64_t K, int g_shift, int splitk) {
  const int strips = args.first[1];
  const int p = __builtin_amdgcn_readfirstlane((int)blockIdx.x >= strips ? 1 : 0);
  const int strip = (int)blockIdx.x - p * strips;
  const int64_t N = args.N[0];
  woq_gemv_w4_body<IS_BF16, G128, VSTEPS, 1, false, 4, PERM, true>(x, args.qweight[p], args.scales[p], args.qzeros[p], nullptr, args.y[0], partial, counters + strip, M,
                                                                   N, K, (N + 7) / 8, g_shift, splitk, strip, (int)blockIdx.y, PERM ? args.k_order[p] : nullptr, p);
}

// =============================================================================================
// decode kernel without split-K (round 2): M <= 16, K <= GEMV16_MAX_K
// =============================================================================================
// The streaming kernel above splits K over workgroups to put 512+ of them on the chip, and pays for it after the last MFMA:
// write-through partials, a drain, a ticket, and the last arriver's reload -- about 2 us of a 4.5 us kernel.  Here a workgroup
// owns only 16 columns but ALL of K: sixteen waves take a sixteenth of the K-steps each, a lane's packed word (8 k of one
// column) is the B operand of v_mfma_f32_16x16x32 once dequantised, and the sixteen accumulators meet in LDS -- one hop, inside
// the workgroup.  N / 16 workgroups (256 at N = 4096), every byte of W requested before the first use.
constexpr int GEMV16_WAVES = 16;
constexpr int GEMV16_CH = 12;                                              // K-steps per wave and pass whose loads are issued up front
static_assert(GEMV16_MAX_K == (int64_t)32 * GEMV16_WAVES * 2 * GEMV16_CH, "two passes: K <= 12288");

// PERM: x is gathered through k_order (perm_load8 / perm_gather8 above the streaming body; inc_woq_gemm_perm)
template <bool IS_BF16, bool NT = false, bool PERM = false>
__global__ __launch_bounds__(64 * GEMV16_WAVES) void woq_gemv16_w4_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M, int64_t N, int64_t K,
    int64_t NW, int g_shift, const int32_t* __restrict__ k_order = nullptr) {
  // PERM: 8 steps per pass (the product routes K <= 4096 here: at most 8 steps per wave) -- the indices of a pass are in flight next
  // to its weights, and a workgroup of 16 waves leaves a lane 128 registers.  The order of the MFMAs does not depend on CH.
  constexpr int WAVES = GEMV16_WAVES, CH = PERM ? 8 : GEMV16_CH;
  __shared__ float red[WAVES * 16 * 17];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jn = lane & 15, kg = lane >> 4;
  const float inv_u = fp8_unit_inverse();
  const int64_t n0 = (int64_t)blockIdx.x * 16;
  int64_t ncol = n0 + jn;
  if (ncol > N - 1) ncol = N - 1;  // clamped lanes recompute a valid column; their results are not stored
  const int zsh = 4 * (int)(ncol & 7);
  const int am = jn < M ? jn : M - 1;  // A row (clamped; rows >= M only feed outputs that are never stored)
  const uint16_t* const xrow = x + (int64_t)am * K + 8 * kg;
  const uint32_t* const wcol = qweight + (int64_t)kg * N + ncol;
  const int steps_total = (int)(K / 32);
  const int lo = (int)((int64_t)steps_total * wave / WAVES), hi = (int)((int64_t)steps_total * (wave + 1) / WAVES);

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = lo; c0 < hi; c0 += CH) {
    uint32_t w[CH], zraw[CH];
    uint16_t sraw[CH];
    uint4 a[CH];
    PermIdx8 kraw[PERM ? CH : 1];
    if constexpr (PERM) {
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        int st = c0 + s;
        if (st > hi - 1) st = hi - 1;
        kraw[s] = perm_load8(k_order + (int64_t)st * 32 + 8 * kg);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      int st = c0 + s;
      if (st > hi - 1) st = hi - 1;  // steps past the end re-read the last one and are skipped below
      const int64_t g = g_shift >= 0 ? (((int64_t)st * 32) >> g_shift) : 0;
      w[s] = NT ? __builtin_nontemporal_load(wcol + (int64_t)st * 4 * N) : wcol[(int64_t)st * 4 * N];
      sraw[s] = scales[g * N + ncol];
      zraw[s] = qzeros[g * NW + (ncol >> 3)];
      if constexpr (PERM) a[s] = perm_gather8(x, 2u * (uint32_t)am * (uint32_t)K, kraw[s], (int)(K - 1));
      else a[s] = *reinterpret_cast<const uint4*>(xrow + (int64_t)st * 32);
    }
    __builtin_amdgcn_sched_barrier(0);  // everything above is in flight before the first use below
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      if (c0 + s < hi) {
        const float sc = f16_bits_to_f32(sraw[s]);
        uint32_t zz = ((zraw[s] >> zsh) & 15u) + 1u;  // modules.py:407-410 (stored zp - 1; wraps above 15)
        zz = zz > 15u ? 0u : zz;
        const uint4 bq = dequant8<IS_BF16, 1>(w[s], sc * inv_u, -(float)zz * sc);
        acc = mfma16<IS_BF16>(a[s], bq, acc);
      }
    }
  }
  // D of the MFMA: column = lane & 15 (= jn), row = 4 * kg + r
#pragma unroll
  for (int r = 0; r < 4; ++r) red[(wave * 16 + 4 * kg + r) * 17 + jn] = acc[r];
  __syncthreads();
  if (tid < 256) {
    const int m = tid >> 4, c = tid & 15;
    float v = red[m * 17 + c];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) v += red[(wv * 16 + m) * 17 + c];  // fixed order
    const int64_t n = n0 + c;
    if (m < M && n < N) {
      v += bias ? cvt16<IS_BF16>(bias[n]) : 0.f;
      y[(int64_t)m * N + n] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
    }
  }
}

// one rung of the ladder: the kernel of the launch's form at <dtype, group lookup, steps per wave, row blocks, bits>.  The forms take the
// same rung of the same body: that makes the gathered and the batched launch bit-identical to the plain one.  Only rungs that a route
// reaches exist: batched 8-bit with one row block (gemv_multi_plan: M <= 16); non-temporal (harness) in bf16, one group per 4 steps, one row block.
template <bool F, bool GG, int V, int B, int W>
int stream_rung(const StreamLaunch& l) {
  dim3 grid((unsigned)l.strips, (unsigned)l.splitk);
  if (l.batch && l.gated) {
    if constexpr (W == 4 && B == 1) {
      if (l.batch_perm) woq_gemv_w4_gated_kernel<F, GG, V, true><<<grid, 256, 0, l.s>>>(*l.batch, l.x, l.part, l.counters, (int)l.M, l.K, l.g_shift, l.splitk);
      else woq_gemv_w4_gated_kernel<F, GG, V, false><<<grid, 256, 0, l.s>>>(*l.batch, l.x, l.part, l.counters, (int)l.M, l.K, l.g_shift, l.splitk);
    } else return INC_ERR_UNSUPPORTED;
  } else if (l.batch) {
    if constexpr (W == 4 || B == 1) {
      if (l.batch_perm) woq_gemv_w4_multi_kernel<F, GG, V, B, W, true><<<grid, 256, 0, l.s>>>(*l.batch, l.x, l.part, l.counters, (int)l.M, l.K, l.g_shift, l.splitk);
      else woq_gemv_w4_multi_kernel<F, GG, V, B, W><<<grid, 256, 0, l.s>>>(*l.batch, l.x, l.part, l.counters, (int)l.M, l.K, l.g_shift, l.splitk);
    } else return INC_ERR_UNSUPPORTED;
  } else if (l.k_order) {
    woq_gemv_w4_perm_kernel<F, GG, V, B, W><<<grid, 256, 0, l.s>>>(l.x, l.k_order, l.mod->qw, l.mod->scales, l.mod->qz, l.mod->bias, l.mod->y, l.part, l.counters, (int)l.M, l.mod->N, l.K, l.mod->NW, l.g_shift, l.splitk);
  } else if (l.nt) {
#ifdef INC_KBENCH
    if constexpr (F && GG && B == 1 && W == 4) woq_gemv_w4_kernel<F, GG, V, B, true><<<grid, 256, 0, l.s>>>(l.x, l.mod->qw, l.mod->scales, l.mod->qz, l.mod->bias, l.mod->y, l.part, l.counters, (int)l.M, l.mod->N, l.K, l.mod->NW, l.g_shift, l.splitk);
    else
#endif
      return INC_ERR_UNSUPPORTED;
  } else {
    woq_gemv_w4_kernel<F, GG, V, B, false, W><<<grid, 256, 0, l.s>>>(l.x, l.mod->qw, l.mod->scales, l.mod->qz, l.mod->bias, l.mod->y, l.part, l.counters, (int)l.M, l.mod->N, l.K, l.mod->NW, l.g_shift, l.splitk);
  }
  INC_LAUNCH_RETURN();
}

template <bool F, bool GG>  // 8 steps per wave only with one row block of 4-bit words; 8-bit words always 4 steps
int stream_ladder(const StreamLaunch& l) {
  if (l.bits == 8) return l.mb == 4 ? stream_rung<F, GG, 4, 4, 8>(l) : l.mb == 2 ? stream_rung<F, GG, 4, 2, 8>(l) : stream_rung<F, GG, 4, 1, 8>(l);
  if (l.mb == 4) return stream_rung<F, GG, 4, 4, 4>(l);
  if (l.mb == 2) return stream_rung<F, GG, 4, 2, 4>(l);
  return l.steps == 4 ? stream_rung<F, GG, 4, 1, 4>(l) : stream_rung<F, GG, 8, 1, 4>(l);
}

}  // namespace

int inc_launch_woq_gemv_stream(const StreamLaunch& l) {
  const bool g128 = l.g_shift == -1 || l.g_shift >= 7;  // one group per 4 steps: a scale / zero-point fetch per group instead of per step
  if (l.bf) return g128 ? stream_ladder<true, true>(l) : stream_ladder<true, false>(l);
  return g128 ? stream_ladder<false, true>(l) : stream_ladder<false, false>(l);
}

// `k_order`: the gathered form (inc_woq_gemm_perm) or NULL; `nt`: the harness's non-temporal weight loads (bf16, no gather)
int inc_launch_woq_gemv16(const WoqGemmArgs& a, const int32_t* k_order, bool nt) {
  const unsigned grid = (unsigned)ceil_div64(a.N, 16);
#define INC_GEMV16(...) woq_gemv16_w4_kernel<__VA_ARGS__><<<grid, 64 * GEMV16_WAVES, 0, a.s>>>(a.x, a.qw, a.scales, a.qz, a.bias, a.y, (int)a.M, a.N, a.K, a.NW, a.g_shift, k_order)
  if (k_order) { if (a.bf) INC_GEMV16(true, false, true); else INC_GEMV16(false, false, true); }
  else if (nt) {
#ifdef INC_KBENCH
    if (a.bf) INC_GEMV16(true, true); else
#endif
      return INC_ERR_UNSUPPORTED;
  } else if (a.bf) INC_GEMV16(true);
  else INC_GEMV16(false);
#undef INC_GEMV16
  INC_LAUNCH_RETURN();
}
