// gemm_common.hpp -- shared by the dequant-GEMM translation units: the launchers inc_woq_gemm (gemm.hip) dispatches to, one per
// kernel family and file, the constants its route planner shares with them, and the device helpers (MFMA wrappers, the int4 / int8
// -> bf16 / f16 dequantisation arithmetic, the 256 x 256 x 64 tile constants).
#pragma once
#include "common.hpp"

// ---- what the route planner (woq_gemm_plan, gemm.hip) and the kernels' files both need ---------------------------------------------
// workspace layout : [0, 16 KiB) arrival counters of the fast GEMV (uint32 per 64-column
// strip; MUST be zero on first use, the kernel re-arms them), then fp32 split-K partials.
constexpr int64_t WS_COUNTER_BYTES = 16384;
constexpr int64_t GEMV_MAX_M = 64;          // gemm_stream.hip: M <= 64 streams the weights once (woq_gemv_w4_kernel with 1 / 2 / 4 row blocks)
constexpr int64_t GEMV16_MAX_K = 12288;     // gemm_stream.hip: the no-split decode kernel's two passes of 12 K-steps per wave
constexpr int64_t STRIP_MAX_M = 1024;       // gemm_strip.hip: the mid-M strip kernel
constexpr int64_t STREAM_SLICE_K = 32 * 4 * 4;  // k of one K-slice of the streaming kernel at 4 steps per wave (4 waves x 4 steps x 32 k)

// the tensors of one packed module, the shape and the stream: what every launcher below takes
struct WoqGemmArgs {
  const uint16_t* x;
  const uint32_t* qw;
  const uint16_t* scales;
  const uint32_t* qz;
  const uint16_t* bias;
  uint16_t* y;
  int64_t M, N, K, NW;  // NW: words per row of qzeros
  int g_shift;
  bool bf;
  hipStream_t s;
};

// gemm_tile.hip: the 128 x 128 tile kernel (any width, any group size, g_idx) and the generic split-K kernel for M <= 16 with its plan
int inc_launch_woq_gemm_tile(const WoqGemmArgs& a, const int32_t* g_idx, int bits, int group_size, int x_vec_ok);
int inc_woq_gemm_small_slices(int64_t N, int64_t K, int bits, int* kw_per_slice_out);
int inc_launch_woq_gemm_small(const WoqGemmArgs& a, const int32_t* g_idx, int bits, int group_size, float* part, int slices, int kw_per_slice);

// gemm_tile256.hip: the 256 x 256 kernels (two-stage "big"; 3A2B in 4 / 8 bits, `dbg` = the harness flag); the slab reduce of every split-K 256-row launch
int inc_launch_woq_gemm_big(const WoqGemmArgs& a, int y_vec_ok);
int inc_launch_woq_gemm_3a2b(const WoqGemmArgs& a, int bits, int y_vec_ok, float* part, int steps, int splits, int dbg);
int inc_launch_slab_reduce(const WoqGemmArgs& a, const float* part, int splits);
int inc_launch_woq_gemm_pc(const WoqGemmArgs& a, int y_vec_ok, float* part, int steps, int splits, int dbg);  // harness only: tools/kbench_gemm_2.inc

// gemm_strip.hip: the 64 x 128 mid-M strip kernel and its split-K plan (`dbg`: harness ablations)
int inc_woq_gemm_strip_splitk(int64_t M, int64_t N, int64_t K);
int inc_launch_woq_gemm_strip(const WoqGemmArgs& a, float* part, unsigned* counters, int splitk, int dbg);

// gemm_d2r.hip: the direct-to-register dequant-GEMM; the same tile with eight waves, two per SIMD (tools/gemm_d2r8.hip, harness only)
int inc_launch_woq_gemm_d2r(const WoqGemmArgs& a, int y_vec_ok, float* part, int steps, int splits, int ns, int abl);
int inc_launch_woq_gemm_d2r8(const WoqGemmArgs& a, int y_vec_ok, float* part, int steps, int splits);

// gemm_strip8.hip: the 128 x 128 mid-M kernel (four waves, K split inside the workgroup) and its split-K plan
int inc_woq_gemm_strip8_splitk(int64_t M, int64_t N, int64_t K);
int inc_launch_woq_gemm_strip8(const WoqGemmArgs& a, float* part, unsigned* counters, int splitk);

// modules that share x, one launch (inc_woq_gemm_multi / _multi_perm; inc_woq_gemm_gated with gate = 0, up = 1 and y[0] = h): the
// per-module tensors of the batch, passed to the kernels by value
constexpr int GEMV_MAX_BATCH = 8;
struct GemvBatch {
  const int32_t* k_order[GEMV_MAX_BATCH];  // the gathered forms: every member's order (never NULL there); not read otherwise
  const uint32_t* qweight[GEMV_MAX_BATCH];
  const uint16_t* scales[GEMV_MAX_BATCH];
  const uint32_t* qzeros[GEMV_MAX_BATCH];
  const uint16_t* bias[GEMV_MAX_BATCH];
  uint16_t* y[GEMV_MAX_BATCH];
  int64_t N[GEMV_MAX_BATCH];
  int64_t part_off[GEMV_MAX_BATCH];  // first float of the module's split-K slabs in the workspace
  int first[GEMV_MAX_BATCH + 1];     // first strip of every module, then the number of strips
  int n;
};
// fills the batch from the entry points' pointer arrays (k_order / bias may be NULL: no orders / no biases; members past n stay null with
// N = 0): member i's strips start at first[i], its slabs [splitk][M][N[i]] at float part_off[i].  Returns the totals.  No checks: each
// entry point makes its own before it calls this.
struct GemvBatchTotals { int64_t floats, strips; };
inline GemvBatchTotals gemv_batch_fill(GemvBatch* b, int n, const int32_t* const* k_order, const int32_t* const* qweight, const uint16_t* const* scales,
                                       const int32_t* const* qzeros, const void* const* bias, void* const* y, int splitk, int64_t M, const int64_t* N) {
  *b = GemvBatch{};
  b->n = n;
  int64_t off = 0;
  int first = 0;
  for (int i = 0; i < n; ++i) {
    b->k_order[i] = k_order ? k_order[i] : nullptr;
    b->qweight[i] = (const uint32_t*)qweight[i];
    b->scales[i] = scales[i];
    b->qzeros[i] = (const uint32_t*)qzeros[i];
    b->bias[i] = bias ? (const uint16_t*)bias[i] : nullptr;
    b->y[i] = (uint16_t*)y[i];
    b->N[i] = N[i];
    b->part_off[i] = off;
    b->first[i] = first;
    off += (int64_t)splitk * M * N[i];
    first += (int)((N[i] + 63) / 64);
  }
  for (int i = n; i <= GEMV_MAX_BATCH; ++i) b->first[i] = first;
  return {off, first};
}

// the two parts of the workspace (layout above); `slabs` = false: a launch without K-slices gets no partials
struct WsParts { unsigned* counters; float* part; };
inline WsParts ws_parts(void* workspace, bool slabs = true) {
  return {(unsigned*)workspace, workspace && slabs ? (float*)((char*)workspace + WS_COUNTER_BYTES) : nullptr};
}

// group lookup by shift: log2(group_size) for a power of two >= 32, -1 = one group (group_size >= K), -2 = neither
inline int g_shift_of(int group_size, int64_t K) {
  if (group_size >= K) return -1;
  if (group_size < 32 || (group_size & (group_size - 1)) != 0) return -2;
  return __builtin_ctz((unsigned)group_size);
}

// gemm_stream.hip: the streaming GEMV (M <= 64) in all its forms, and the no-split decode kernel.  A launch is x, the plan (steps, mb,
// splitk: woq_gemm_plan / gemv_multi_plan) and the weights: ONE module `mod` (its x, M, K, g_shift, bf, s are not read) -- plain, gathered
// through `k_order` (inc_woq_gemm_perm) or, in the harness, `nt` (non-temporal loads) -- or the `batch` of inc_woq_gemm_multi, gathered
// through the batch's own orders with `batch_perm` (inc_woq_gemm_multi_perm); `gated`: the batch is a gate / up pair whose strips share
// a ticket and leave silu(g) * u in batch->y[0] (inc_woq_gemm_gated: one row block, 4-bit).
struct StreamLaunch {
  const uint16_t* x;
  int64_t M, K;
  int g_shift;
  bool bf;
  hipStream_t s;
  int bits, steps, mb, splitk;
  int64_t strips;      // 64-column strips: blockIdx.x
  float* part;
  unsigned* counters;
  const WoqGemmArgs* mod = nullptr;
  const int32_t* k_order = nullptr;
  const GemvBatch* batch = nullptr;
  bool nt = false;
  bool batch_perm = false, gated = false;
};
int inc_launch_woq_gemv_stream(const StreamLaunch& l);
int inc_launch_woq_gemv16(const WoqGemmArgs& a, const int32_t* k_order, bool nt);

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <bool IS_BF16>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  if constexpr (IS_BF16) {
    return (uint32_t)f32_to_bf16_bits(lo) | ((uint32_t)f32_to_bf16_bits(hi) << 16);
  } else {
    return (uint32_t)f32_to_f16_bits(lo) | ((uint32_t)f32_to_f16_bits(hi) << 16);
  }
}

template <bool IS_BF16>
__device__ __forceinline__ float cvt16(uint16_t b) {
  if constexpr (IS_BF16) return bf16_bits_to_f32(b);
  else return f16_bits_to_f32(b);
}

// group parameters of one (group, column): fp32 scale and integer zero point
struct GroupQ {
  float s;
  int z;
};

template <int BITS>
__device__ __forceinline__ GroupQ load_group(const uint16_t* __restrict__ scales,
                                             const uint32_t* __restrict__ qzeros, int64_t g, int64_t n,
                                             int64_t N, int64_t NW) {
  constexpr int NP = 32 / BITS;
  constexpr uint32_t MASK = (1u << BITS) - 1u;
  GroupQ r;
  r.s = f16_bits_to_f32(scales[g * N + n]);
  uint32_t zz = ((qzeros[g * NW + n / NP] >> (BITS * (uint32_t)(n % NP))) & MASK) + 1u;  // modules.py:407-410
  r.z = zz > MASK ? 0 : (int)zz;
  return r;
}

// dequantise one packed word (NP consecutive k of one column) into NP/2 dwords of 16-bit pairs
template <int BITS, bool IS_BF16>
__device__ __forceinline__ void dequant_word(uint32_t word, const GroupQ& gq, uint32_t (&out)[16 / BITS]) {
  constexpr int NP = 32 / BITS;
  constexpr uint32_t MASK = (1u << BITS) - 1u;
#pragma unroll
  for (int h = 0; h < NP / 2; ++h) {
    const int q0 = (int)((word >> (BITS * (2 * h))) & MASK);
    const int q1 = (int)((word >> (BITS * (2 * h + 1))) & MASK);
    const float v0 = (float)(int8_t)(q0 - gq.z) * gq.s;
    const float v1 = (float)(int8_t)(q1 - gq.z) * gq.s;
    out[h] = pack2<IS_BF16>(v0, v1);
  }
}

// the same with a per-ELEMENT group (g_idx: GPTQ act_order / HF desc_act, modules.py:427-431): column k of the word takes the
// scale / zero point of group g_idx[k] -- one lookup per element, the general (slow) path of the two small-tile kernels
template <int BITS, bool IS_BF16>
__device__ __forceinline__ void dequant_word_gidx(uint32_t word, const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros,
                                                  const int32_t* __restrict__ g_idx, int64_t kk, int64_t K, int64_t n, int64_t N, int64_t NW,
                                                  uint32_t (&out)[16 / BITS]) {
  constexpr int NP = 32 / BITS;
  constexpr uint32_t MASK = (1u << BITS) - 1u;
#pragma unroll
  for (int h = 0; h < NP / 2; ++h) {
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = 2 * h + e;
      const int64_t k = kk + j;
      const GroupQ gq = load_group<BITS>(scales, qzeros, k < K ? (int64_t)g_idx[k] : 0, n, N, NW);
      const int q = (int)((word >> (BITS * j)) & MASK);
      v[e] = (float)(int8_t)(q - gq.z) * gq.s;
    }
    out[h] = pack2<IS_BF16>(v[0], v[1]);
  }
}

template <bool IS_BF16>
__device__ __forceinline__ f32x16 mfma32(const uint4& a, const uint4& b, f32x16 c) {
  if constexpr (IS_BF16) {
    bf16x8 fa, fb;
    __builtin_memcpy(&fa, &a, 16);
    __builtin_memcpy(&fb, &b, 16);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, c, 0, 0, 0);
  } else {
    f16x8 fa, fb;
    __builtin_memcpy(&fa, &a, 16);
    __builtin_memcpy(&fb, &b, 16);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, c, 0, 0, 0);
  }
}
template <bool IS_BF16>
__device__ __forceinline__ f32x4 mfma16(const uint4& a, const uint4& b, f32x4 c) {
  if constexpr (IS_BF16) {
    bf16x8 fa, fb;
    __builtin_memcpy(&fa, &a, 16);
    __builtin_memcpy(&fb, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, c, 0, 0, 0);
  } else {
    f16x8 fa, fb;
    __builtin_memcpy(&fa, &a, 16);
    __builtin_memcpy(&fb, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, fb, c, 0, 0, 0);
  }
}

// the gathered A operand of the decode kernels (PERM: gemm_stream.hip, gemm_anyw.hip): 8 entries of k_order as two 16-byte loads (16-byte
// aligned, offset a multiple of 8), and the 8 two-byte loads of x[row, k_order[..]] they select, clamped to [0, kmax], packed like the
// 16-byte load of the plain form; `row_bytes` = the row's byte offset in x (M * K < 2^31)
struct PermIdx8 { int4 lo, hi; };
__device__ __forceinline__ PermIdx8 perm_load8(const int32_t* __restrict__ ko) {
  return PermIdx8{*reinterpret_cast<const int4*>(ko), *reinterpret_cast<const int4*>(ko + 4)};
}
__device__ __forceinline__ uint4 perm_gather8(const uint16_t* __restrict__ x, uint32_t row_bytes, const PermIdx8& p, int kmax) {
  const int raw[8] = {p.lo.x, p.lo.y, p.lo.z, p.lo.w, p.hi.x, p.hi.y, p.hi.z, p.hi.w};
  uint32_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = raw[j] < 0 ? 0 : (raw[j] > kmax ? kmax : raw[j]);
    v[j] = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(x) + (row_bytes + 2u * (uint32_t)k));
  }
  return make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
}

// 16-byte write-through store / L2-coherent load of split-K partials (the hand-off of MI355X_MICROARCH.md "Valid forms": sc1 stores ->
// vmcnt(0) -> barrier -> one relaxed agent-scope ticket -> sc1 loads by the last arriver); the caller waits for the loads (vmcnt) itself
__device__ __forceinline__ void splitk_store16_sc1(float* p, f32x4 v) {
  // (s_nop: a VMEM store of more than 64 bits reads its data registers AFTER issue -- the next instruction may not overwrite them for two
  // wait states; the compiler's hazard recogniser inserts that for its own stores but cannot see into an asm statement.  Without it this
  // hand-off returned wrong sums a few times per hundred launches.)
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
// pv[sl][i] = 16 bytes at bases[sl] + off[i] (byte offsets < 4 GiB), sl, i in 0..3, sc1 (L2-coherent: the partials were written through by
// other XCDs), and the wait for them -- ONE asm statement: a load whose result the compiler sees before an explicit s_waitcnt may be
// copied or spilled by it before the data has landed (MI355X guide, inline-asm hazards)
__device__ __forceinline__ void splitk_load16x16_sc1(f32x4 (&pv)[4][4], const float* b0, const float* b1, const float* b2, const float* b3,
                                                     uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3) {
  asm volatile(
      "global_load_dwordx4 %0, %16, %20 sc1\n\tglobal_load_dwordx4 %1, %17, %20 sc1\n\tglobal_load_dwordx4 %2, %18, %20 sc1\n\tglobal_load_dwordx4 %3, %19, %20 sc1\n\t"
      "global_load_dwordx4 %4, %16, %21 sc1\n\tglobal_load_dwordx4 %5, %17, %21 sc1\n\tglobal_load_dwordx4 %6, %18, %21 sc1\n\tglobal_load_dwordx4 %7, %19, %21 sc1\n\t"
      "global_load_dwordx4 %8, %16, %22 sc1\n\tglobal_load_dwordx4 %9, %17, %22 sc1\n\tglobal_load_dwordx4 %10, %18, %22 sc1\n\tglobal_load_dwordx4 %11, %19, %22 sc1\n\t"
      "global_load_dwordx4 %12, %16, %23 sc1\n\tglobal_load_dwordx4 %13, %17, %23 sc1\n\tglobal_load_dwordx4 %14, %18, %23 sc1\n\tglobal_load_dwordx4 %15, %19, %23 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(pv[0][0]), "=&v"(pv[0][1]), "=&v"(pv[0][2]), "=&v"(pv[0][3]), "=&v"(pv[1][0]), "=&v"(pv[1][1]), "=&v"(pv[1][2]), "=&v"(pv[1][3]),
        "=&v"(pv[2][0]), "=&v"(pv[2][1]), "=&v"(pv[2][2]), "=&v"(pv[2][3]), "=&v"(pv[3][0]), "=&v"(pv[3][1]), "=&v"(pv[3][2]), "=&v"(pv[3][3])
      : "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(b0), "s"(b1), "s"(b2), "s"(b3)
      : "memory");
}

// ---- the way out of a split-K workgroup -----------------------------------------------------------------------------------------------
// The hand-off after a workgroup's write-through (`sc1`) partial stores: every wave drains them (`s_waitcnt vmcnt(0)`), barrier, ONE
// relaxed agent-scope ticket from thread 0; the arriver with ticket `arrivals` - 1 re-arms the counter for the next call and is told so
// through `lds_word`, an LDS word of the caller's that nothing else reads until the next barrier.  Returns whether this workgroup is that
// last arriver; it then reads the slabs with `sc1` loads (L2-coherent), so neither side needs an agent-scope fence.  The order of these
// steps IS the protocol (MI355X_MICROARCH.md, "Valid forms besides R1/R2"): the stores go before the call, the loads after it.
template <typename T>
__device__ __forceinline__ bool splitk_arrive(unsigned* counter, int arrivals, T* lds_word) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = ticket == (unsigned)(arrivals - 1);
    if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next call
    *lds_word = last ? T(1) : T(0);
  }
  __syncthreads();
  return *lds_word != T(0);
}

// The (64-column strip, K-slice) workgroups of the decode GEMVs (gemm_stream.hip, gemm_anyw.hip): 256 threads, ROWS rows of x, the four
// waves' fp32 strips in red[wave][ROWS][65].  Thread tid owns outputs idx = tid + 256 i -> row idx >> 6, column idx & 63 of the strip.
template <int ROWS>
struct StripOut {
  static constexpr int NOUT = ROWS * 64 / 256;  // outputs per thread
  bool ok[NOUT];                                // inside [M, N]
  int64_t off[NOUT];                            // m * N + n (0 where !ok)
  uint16_t braw[NOUT];                          // the bias of the column, fetched up front
};
// output i of the thread; `fallback`: any valid address (read instead of a NULL bias, so that the loads stay unconditional)
template <int ROWS>
__device__ __forceinline__ void strip_out_prefetch_one(StripOut<ROWS>& o, int i, int tid, int M, int64_t N, int64_t n0, const uint16_t* __restrict__ bias,
                                                       const uint16_t* __restrict__ fallback) {
  const uint16_t* const bsrc = bias ? bias : fallback;
  const int idx = tid + 256 * i, m = idx >> 6, c = idx & 63;
  o.ok[i] = m < M && n0 + c < N;
  o.off[i] = o.ok[i] ? (int64_t)m * N + n0 + c : 0;
  o.braw[i] = bsrc[o.ok[i] ? n0 + c : 0];
}
// all of them, issued with the body's other loads before its sched_barrier: the bias is in flight with the weights
template <int ROWS>
__device__ __forceinline__ void strip_out_prefetch(StripOut<ROWS>& o, int tid, int M, int64_t N, int64_t n0, const uint16_t* __restrict__ bias,
                                                   const uint16_t* __restrict__ fallback) {
#pragma unroll
  for (int i = 0; i < StripOut<ROWS>::NOUT; ++i) strip_out_prefetch_one(o, i, tid, M, N, n0, bias, fallback);
}
// barrier, then the sum of the four waves in wave order
template <int ROWS>
__device__ __forceinline__ void strip_sum_waves(const float* red, int tid, float (&sum)[StripOut<ROWS>::NOUT]) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < StripOut<ROWS>::NOUT; ++i) {
    const int idx = tid + 256 * i, m = idx >> 6, c = idx & 63;
    sum[i] = red[(0 * ROWS + m) * 65 + c] + red[(1 * ROWS + m) * 65 + c] + red[(2 * ROWS + m) * 65 + c] + red[(3 * ROWS + m) * 65 + c];
  }
}
// the strip sum of one slice into its slab [M][N], write-through
template <int ROWS>
__device__ __forceinline__ void strip_store_partial(float* __restrict__ slab, const StripOut<ROWS>& o, const float (&sum)[StripOut<ROWS>::NOUT]) {
#pragma unroll
  for (int i = 0; i < StripOut<ROWS>::NOUT; ++i)
    if (o.ok[i]) __hip_atomic_store(&slab[o.off[i]], sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
}
// the last arriver's fixed-order sum over the K-slices of one module's slabs (`sc1` loads), slice 0 first; up to 32 partial loads of a
// thread in flight (8 slices for M <= 16: one L2 round trip)
template <int NOUT>
__device__ __forceinline__ void splitk_sum_slices(const float* __restrict__ partial, int64_t slab, int splitk, const int64_t (&out_off)[NOUT], float (&sum)[NOUT]) {
#pragma unroll
  for (int i = 0; i < NOUT; ++i) sum[i] = 0.f;
  constexpr int SB = 32 / NOUT;
  for (int sl0 = 0; sl0 < splitk; sl0 += SB) {
    float pv[SB][NOUT];
#pragma unroll
    for (int d = 0; d < SB; ++d) {
      const int sl = sl0 + d < splitk ? sl0 + d : splitk - 1;
#pragma unroll
      for (int i = 0; i < NOUT; ++i) pv[d][i] = __hip_atomic_load(&partial[(int64_t)sl * slab + out_off[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
    }
#pragma unroll
    for (int d = 0; d < SB; ++d)
#pragma unroll
      for (int i = 0; i < NOUT; ++i) sum[i] += (sl0 + d < splitk) ? pv[d][i] : 0.f;
  }
}
// everything after the waves have written red[]: waves 0 + 1 + 2 + 3; with K-slices the partial store, the hand-off on the strip's
// `counter` and, in the last arriver, the slices in slice order; then + bias, ONE rounding, store.  `partial`: the module's slabs [slice][M][N]
template <bool IS_BF16, int ROWS>
__device__ __forceinline__ void strip_finish(float* red, int tid, const StripOut<ROWS>& o, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
                                             float* __restrict__ partial, unsigned* __restrict__ counter, int M, int64_t N, int splitk, int slice) {
  constexpr int NOUT = StripOut<ROWS>::NOUT;
  float sum[NOUT];
  strip_sum_waves<ROWS>(red, tid, sum);
  if (splitk > 1) {
    const int64_t slab = (int64_t)M * N;
    strip_store_partial<ROWS>(partial + (int64_t)slice * slab, o, sum);
    if (!splitk_arrive(counter, splitk, red)) return;
    splitk_sum_slices<NOUT>(partial, slab, splitk, o.off, sum);
  }
#pragma unroll
  for (int i = 0; i < NOUT; ++i)
    if (o.ok[i]) {
      const float v = sum[i] + (bias ? cvt16<IS_BF16>(o.braw[i]) : 0.f);
      y[o.off[i]] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
    }
}

// four adjacent outputs of one row: + bias, one rounding to the 16-bit type, one 8-byte store (y + n with n % 4 == 0 and N % 4 == 0)
template <bool IS_BF16>
__device__ __forceinline__ void store_out4(uint16_t* dst, float4 v, const uint16_t* bias4) {
  if (bias4) {
    const uint2 b = *reinterpret_cast<const uint2*>(bias4);
    v.x += cvt16<IS_BF16>((uint16_t)(b.x & 0xffffu)); v.y += cvt16<IS_BF16>((uint16_t)(b.x >> 16));
    v.z += cvt16<IS_BF16>((uint16_t)(b.y & 0xffffu)); v.w += cvt16<IS_BF16>((uint16_t)(b.y >> 16));
  }
  uint2 o;
  o.x = pack2<IS_BF16>(v.x, v.y);
  o.y = pack2<IS_BF16>(v.z, v.w);
  *reinterpret_cast<uint2*>(dst) = o;
}

constexpr int TM = 256, TN = 256, TK = 64;
constexpr int T_ASTAGE = TM * TK * 2;  // bytes
constexpr int T_BSTAGE = TN * TK * 2;

// 8 nibbles of `w` -> 8 x rn16((q - z) * s), k-ordered, as 4 dwords.
// int -> float goes through the fp8 converter: an e4m3 byte with value q in 0..15 decodes to q * u (u = 2^-9 for the
// OCP format of gfx950: codes 0..7 are subnormals m * 2^-9, codes 8..15 are (1 + m/8) * 2^-6 = (8 + m) * 2^-9), so ONE
// v_cvt_pk_f32_fp8 turns two nibbles (bytes of `w & 0x0F0F0F0F`) into two floats -- 4 instead of 8 conversions per word.
// `s_over_u` = s / u (exact: a power-of-two rescale); fma(q*u, s/u, -z*s) is exact in fp32 (q, z < 32 and s has 11
// significant bits), so the single rounding is the 16-bit conversion: bit-identical to inc_woq_dequant.
__device__ __forceinline__ float fp8_unit_inverse() {
  return 1.0f / __builtin_amdgcn_cvt_pk_f32_fp8(0x00000001, false)[0];  // measured, not assumed: 2^9 on gfx950
}
// one fp32 FMA that the SLP vectoriser cannot fuse into v_pk_fma_f32 (see dequant8's SFMA form)
__device__ __forceinline__ float fma_single(float a, float b, float c) {
  float d;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
// FORM 0 (default): eight v_fma_f32; FORM 1: four v_pk_fma_f32 (the first generation; same values -- each half of the packed op
// is the same fused multiply-add); FORM 2: eight single v_cvt_f32_fp8 (byte select) + eight v_fma_f32.
// MI355X_MICROARCH.md: a packed fp32 VALU op next to MFMAs costs ~22 cycles more than the two scalar ops it replaces -- measured
// here: the producer / consumer GEMM gains 6-10 % from FORM 0 (tools/kbench pcfma), outputs bit-identical.
template <bool IS_BF16, int FORM = 0>
__device__ __forceinline__ uint4 dequant8(uint32_t w, float s_over_u, float nzs) {
  const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;  // bytes: k0,k2,k4,k6 / k1,k3,k5,k7
  if constexpr (FORM == 0) {
    const f32x2 c01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), c23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const f32x2 d01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    uint4 o;
    o.x = cvt_pair<IS_BF16>(fma_single(c01[0], s_over_u, nzs), fma_single(d01[0], s_over_u, nzs));
    o.y = cvt_pair<IS_BF16>(fma_single(c01[1], s_over_u, nzs), fma_single(d01[1], s_over_u, nzs));
    o.z = cvt_pair<IS_BF16>(fma_single(c23[0], s_over_u, nzs), fma_single(d23[0], s_over_u, nzs));
    o.w = cvt_pair<IS_BF16>(fma_single(c23[1], s_over_u, nzs), fma_single(d23[1], s_over_u, nzs));
    return o;
  }
  if constexpr (FORM == 2) {
    float e[4], f[4];
    e[0] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 0); e[1] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 1);
    e[2] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 2); e[3] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 3);
    f[0] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 0); f[1] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 1);
    f[2] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 2); f[3] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 3);
    uint4 o;
    o.x = cvt_pair<IS_BF16>(fma_single(e[0], s_over_u, nzs), fma_single(f[0], s_over_u, nzs));
    o.y = cvt_pair<IS_BF16>(fma_single(e[1], s_over_u, nzs), fma_single(f[1], s_over_u, nzs));
    o.z = cvt_pair<IS_BF16>(fma_single(e[2], s_over_u, nzs), fma_single(f[2], s_over_u, nzs));
    o.w = cvt_pair<IS_BF16>(fma_single(e[3], s_over_u, nzs), fma_single(f[3], s_over_u, nzs));
    return o;
  }
  const f32x2 sv = {s_over_u, s_over_u}, nv = {nzs, nzs};
  const f32x2 e01 = __builtin_elementwise_fma(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), sv, nv);  // k0, k2
  const f32x2 e23 = __builtin_elementwise_fma(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true), sv, nv);   // k4, k6
  const f32x2 o01 = __builtin_elementwise_fma(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), sv, nv);  // k1, k3
  const f32x2 o23 = __builtin_elementwise_fma(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true), sv, nv);   // k5, k7
  uint4 o;
  o.x = cvt_pair<IS_BF16>(e01[0], o01[0]);
  o.y = cvt_pair<IS_BF16>(e01[1], o01[1]);
  o.z = cvt_pair<IS_BF16>(e23[0], o23[0]);
  o.w = cvt_pair<IS_BF16>(e23[1], o23[1]);
  return o;
}

// two 8-bit packed words (k0..3, k4..7 of one column) -> 8 x rn16(int8(q - z) * s).  The difference wraps to int8 exactly like the
// reference's recover(), which unpacks 8-bit codes and zero points into int8 tensors and subtracts there (modules.py:377-443:
// an asymmetric code more than 127 away from its zero point flips sign) -- and like inc_woq_dequant / the first-generation
// kernel (dequant_word).  The product of an int8 and an 11-bit scale is exact in fp32: one rounding, in the 16-bit conversion.
template <bool IS_BF16>
__device__ __forceinline__ uint4 dequant8_from_bytes(uint32_t w0, uint32_t w1, float s, int z) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = (float)(int)(int8_t)(uint8_t)(((w0 >> (8 * j)) & 0xffu) - (uint32_t)z) * s;
    f[4 + j] = (float)(int)(int8_t)(uint8_t)(((w1 >> (8 * j)) & 0xffu) - (uint32_t)z) * s;
  }
  uint4 o;
  o.x = cvt_pair<IS_BF16>(f[0], f[1]);
  o.y = cvt_pair<IS_BF16>(f[2], f[3]);
  o.z = cvt_pair<IS_BF16>(f[4], f[5]);
  o.w = cvt_pair<IS_BF16>(f[6], f[7]);
  return o;
}

}  // namespace
