// gemm_anyw.hip -- K4f: the decode GEMV of the widths whose fields do not fill 8-k fragments by themselves, BITS in {1, 2, 3, 5, 6, 7}
// (n_pack = 32 / BITS = 32, 16, 10, 6, 5, 4 fields per word), optimum layout, 1 <= M <= 16 (inc_woq_gemv_anyw).  A sibling of the
// streaming kernel of gemm_stream.hip: the same (64-column strip, K-slice) workgroups, the same four waves meeting in LDS, the same
// split-K hand-off -- with its own walk over the packed words.
//
// Layout walk.  qweight [ceil(K / n_pack), N]: word `r` of column n holds k = n_pack * r .. n_pack * r + n_pack - 1, BITS bits each from
// bit 0.  A lane owns four adjacent columns (one 16-byte request per packed row, as in the sibling) and WL CONSECUTIVE packed rows; laid
// end to end the fields of one column are F = WL * n_pack consecutive k starting at k0 = (lane's first row) * n_pack.  WL is chosen per
// width so that F is a multiple of 8 (1 / 2 / 3 / 5 / 6 / 7 bits: WL = 2 / 4 / 4 / 8 / 8 / 8, F = 64 / 64 / 40 / 48 / 40 / 32), hence
// k0 % 8 == 0: the stream is cut into F / 8 fragments of 8 consecutive k that START ON A MULTIPLE OF 8 whatever n_pack is -- fragment i
// takes stream elements 8 i .. 8 i + 7, assembled across words where a word ends inside it (3 bits: fields 8, 9 of word 0 and 0 .. 5 of
// word 1 are fragment 1).  A fragment is the B operand of v_mfma_f32_16x16x32 for the lane's k-block (lane >> 4); the A operand is the
// 16-byte aligned x[row, k0 + 8 i .. + 7] of the same lane (row = lane & 15), so the two sides of the MFMA agree on which 32 k they sum
// -- which 32 of the slice's k meet in one instruction is irrelevant to the result.  Wave w of slice s owns rows ((4 s + w) * 4 + (lane >> 4)) * WL ..;
// a workgroup covers 16 F consecutive k (1024 / 1024 / 640 / 768 / 640 / 512), grid = strips x ceil(K / 16 F).
// Every packed word is requested once per launch and ALL of a wave's weight requests (WL x 16 B per lane) are issued before the first
// is consumed (the sched_barrier below), with x, the scales and the zero-point words behind them.
//
// Groups.  The group of a field is g = k >> g_shift (group_size a power of two >= 32, or one group): a WORD straddles a group boundary
// (32 is no multiple of 10, 6 or 5), a FRAGMENT never does -- its 8 k start on a multiple of 8 and 8 divides the group size.  So the
// per-field lookup is one lookup per fragment, and because F <= 64 with k0 a multiple of 8 (of 64 when F = 64, of 16 when F = 48) a lane
// meets at most TWO groups: both are fetched up front, fragment i takes the second from kb = (first boundary) - k0 on.  A ragged last
// group (K = 160, group 64) is just a smaller last group; lookups past it clamp to G - 1 and only feed dead fragments.
// qzeros [G, ceil(N / n_pack)] is packed along N: the zero fields of the lane's four columns sit in up to two words (column quads
// straddle a word for every n_pack but 32, 16 and 4), both fetched, selected per column.  Stored field = zp - 1: z = field + 1, and
// z > 2^BITS - 1 wraps to 0 (modules.py:407-410).
// Padding.  Fields at k >= K in the last word (4096 % 10 = 6) and rows past the last (re-read, clamped) fall into fragments with
// k0 + 8 i >= K, all or nothing since K % 8 == 0: their A operand is zeroed and x is addressed at most at K - 8, never at or beyond K.
// A rows >= M are clamped for the address and zeroed; outputs of rows >= M and of clamped columns are not stored.
//
// Numerics: w = rn16(int8(q - z) * scale), bit-identical to inc_woq_dequant.  q, z <= 127, so q - z is an int8 without wrapping;
// fma((float)q, s, -(float)z * s) is exact in fp32 (8-bit integers times an 11-bit significand) and the ONE rounding is the conversion
// to x's dtype.  Products with x accumulate in fp32 inside the MFMA, the four waves add in fixed order through LDS.
// The multiply is on the matrix cores, not the vector ALUs: at M <= 16 neither is the limit, but the MFMA form costs the same for 1
// and for 16 rows (F / 8 x 4 instructions per wave) where fp32 FMAs grow to 16 x 4 x F per lane -- ~7 us of VALU time at 4096^2, M = 16.
//
// The way out of the workgroup is the sibling's, the same code: strip_finish (gemm_common.hpp) -- the four waves add in fixed order
// through LDS; with K-slices the fp32 strip goes to the slice's slab write-through (`sc1`), splitk_arrive hands off (drain, barrier, ONE
// relaxed agent-scope ticket per strip; the last arriver re-arms the counter), and the last arriver sums the slices in slice order with
// `sc1` loads; then the bias, one rounding, the store.  Bit-identical from call to call.
//
// Forms: plain (inc_woq_gemv_anyw), gathered for act_order modules (inc_woq_gemv_anyw_perm), and batched over modules that share x, plain
// or gathered (inc_woq_gemv_anyw_multi) -- one body, described above it.
//
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): see the table above the body.
#include "gemm_common.hpp"

namespace {

template <int BITS> struct AnywShape {
  static_assert(BITS == 1 || BITS == 2 || BITS == 3 || BITS == 5 || BITS == 6 || BITS == 7, "4 and 8 bits are gemm_stream.hip's");
  static constexpr int NP = 32 / BITS;                                  // fields per word
  static constexpr int WL = BITS == 1 ? 2 : BITS <= 3 ? 4 : 8;          // consecutive packed rows (16-byte requests) per lane
  static constexpr int F = WL * NP;                                     // consecutive k per lane
  static constexpr int NF = F / 8;                                      // fragments (MFMAs per column) per lane
  static constexpr int SLICE_K = 16 * F;                                // k of one workgroup: 4 waves x 4 k-blocks x F
  static_assert(F % 8 == 0 && F <= 64, "fragments start on multiples of 8; at most two groups of >= 32 per lane");
};

// stream element e (compile-time) of column c: field e % NP of the lane's word e / NP
template <int BITS>
__device__ __forceinline__ uint32_t anyw_field(const uint4 (&w)[AnywShape<BITS>::WL], int c, int e) {
  constexpr int NP = AnywShape<BITS>::NP;
  const uint4& q = w[e / NP];
  const uint32_t word = c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
  return (word >> (BITS * (e % NP))) & ((1u << BITS) - 1u);
}

// The body of one (64-column strip, K-slice) workgroup: `counter` is the strip's arrival counter, `partial` the module's slabs
// [slice][M][N].  Three kernels share it, as the forms of gemm_stream.hip share theirs:
// PERM (inc_woq_gemv_anyw_perm: act_order modules, whose packed fields are sorted along K by group once -- ops.sort_packed_k): the A operand
// of fragment i is x[row, k_order[k0 + 8 i + t]], t = 0 .. 7, instead of the 16-byte load of x[row, k0 + 8 i ..]: the lane reads its 8
// entries of k_order (two 16-byte loads: k_order is 16-byte aligned and k0 % 8 == 0), clamps each to [0, K - 1] so that no array can send
// a read outside x, and packs eight 2-byte loads (perm_load8 / perm_gather8, gemm_common.hpp).  Dead fragments read their entries at
// K - 8 like x does in the plain form, and their A is zeroed all the same.  Nothing else differs: the same values reach the same MFMAs in
// the same order, so the result equals the plain form's on x.index_select(1, k_order) bit for bit.  x is addressed by 32-bit byte offsets
// (M * K < 2^31) and needs 2-byte alignment only.  Order of issue: the entries of k_order of all fragments, then the weights, then the
// gathers -- vector loads return in order, so the gathers wait for the indices alone while the weights are on their way from HBM; an
// index register is dead once its gather is issued (up to 64 of them at F = 64: the compiler reuses them for the gathered values).
// Batched (inc_woq_gemv_anyw_multi): the strips of the members occupy consecutive ranges of blockIdx.x, each runs this body on its own
// member's tensors with its own counter and its own slabs -- see woq_gemv_anyw_multi_kernel.
//
// Resource report of the cross-compile (VGPRs bf16 / fp16; every instantiation: 16 AGPRs, 16640 bytes of LDS, 0 bytes of scratch):
//   (VGPRs)   plain      gathered   batched    batched + gathered
//   1 bit     100 / 98   139 / 139  100 / 98   140 / 140
//   2 bits    112 / 110  150 / 150  112 / 110  146 / 146
//   3 bits     90 / 90   127 / 127   90 / 90   130 / 130
//   5 bits    110 / 110  142 / 142  110 / 110  139 / 139
//   6 bits    112 / 108  132 / 132  112 / 108  136 / 136
//   7 bits    106 / 104  124 / 124  106 / 104  116 / 116
// SGPRs: 37 - 42, the gathered 1- and 2-bit forms 98 - 104 (profiles/strip_epilogue/resources.txt holds every instantiation).  Plain and batched: 4 waves per SIMD by registers (4 workgroups per CU); the
// gathered forms hold the gathered halves next to the weights in flight and come to 3 -- a decode grid (448 workgroups at 4096^2, 3 bits)
// puts fewer than that on a CU.  No scratch anywhere; the 16 AGPRs are the four accumulators.
template <bool IS_BF16, int BITS, bool PERM = false>
__device__ __forceinline__ void woq_gemv_anyw_body(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counter, int M, int64_t N, int K, int64_t NW, int G, int g_shift, int splitk,
    int strip, int slice, const int32_t* __restrict__ k_order = nullptr) {
  using S = AnywShape<BITS>;
  constexpr int NP = S::NP, WL = S::WL, F = S::F, NF = S::NF;
  constexpr uint32_t MASK = (1u << BITS) - 1u;
  __shared__ float red[4 * 16 * 65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jn = lane & 15, oct = lane >> 4;
  const int64_t n0 = (int64_t)strip * 64;
  int64_t ncol = n0 + 4 * jn;
  if (ncol > N - 4) ncol = N - 4;  // clamped lanes recompute valid columns; their results are not stored
  const int rows_total = (K + NP - 1) / NP;
  const int row0 = ((slice * 4 + wave) * 4 + oct) * WL;
  const int k0 = row0 * NP;  // % 8 == 0

  // ---- issue every load of this wave up front: (PERM: the entries of k_order,) the weights, x -----
  uint4 w[WL], a[NF];
  PermIdx8 kraw[PERM ? NF : 1];
  if constexpr (PERM) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      int kk = k0 + 8 * i;
      if (kk > K - 8) kk = K - 8;  // dead fragments: the last 8 entries, never at or beyond entry K
      kraw[i] = perm_load8(k_order + kk);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int l = 0; l < WL; ++l) {
    int r = row0 + l;
    if (r > rows_total - 1) r = rows_total - 1;  // rows past the end re-read the last one: all their k are >= K, zeroed via A
    w[l] = *reinterpret_cast<const uint4*>(qweight + (int64_t)r * N + ncol);
  }
  const int am = jn < M ? jn : M - 1;  // A row (clamped; rows >= M are zeroed below)
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    int kk = k0 + 8 * i;
    if (kk > K - 8) kk = K - 8;  // dead fragments read the row's last 16 bytes: never at or beyond column K
    if constexpr (PERM) a[i] = perm_gather8(x, 2u * (uint32_t)am * (uint32_t)K, kraw[i], K - 1);
    else a[i] = *reinterpret_cast<const uint4*>(x + (int64_t)am * K + kk);
  }
  // the (at most two) groups of this lane's k0 .. k0 + F - 1
  int g_lo = 0, kb = F;  // kb: first stream element of the second group
  if (g_shift >= 0) {
    g_lo = k0 >> g_shift;
    kb = ((g_lo + 1) << g_shift) - k0;
  }
  int gsel[2] = {g_lo, g_lo + 1};
  uint2 sraw[2];
  uint32_t zraw[2][2];
  const int nc = (int)ncol;  // N <= 2^18 (the counter block): 32-bit arithmetic for the zero-point fields
  const int zw0 = nc / NP, zw1 = (nc + 3) / NP;  // nc + 3 <= N - 1: inside the row
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (gsel[t] > G - 1) gsel[t] = G - 1;
    sraw[t] = *reinterpret_cast<const uint2*>(scales + (int64_t)gsel[t] * N + ncol);
    zraw[t][0] = qzeros[(int64_t)gsel[t] * NW + zw0];
    zraw[t][1] = qzeros[(int64_t)gsel[t] * NW + zw1];
  }
  // this thread's outputs of the strip and their bias, fetched now (scales: a valid address where there is no bias).  The loop is
  // written here, not taken from strip_out_prefetch: unrolled with the loops above it, the plain 5-bit kernels keep their 110 VGPRs
  // (112 with the helper's loop)
  StripOut<16> out;
#pragma unroll
  for (int i = 0; i < out.NOUT; ++i) strip_out_prefetch_one(out, i, tid, M, N, n0, bias, scales);
  __builtin_amdgcn_sched_barrier(0);  // everything above is in flight before the first use below

  // scale and -z * scale of (group t, column c)
  float sc[2][4], nzs[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t sw = c < 2 ? sraw[t].x : sraw[t].y;
      sc[t][c] = f16_bits_to_f32((uint16_t)(sw >> (16 * (c & 1))));
      const int n = nc + c;
      const uint32_t zw = n / NP == zw0 ? zraw[t][0] : zraw[t][1];
      uint32_t zz = ((zw >> (BITS * (uint32_t)(n % NP))) & MASK) + 1u;  // modules.py:407-410 (stored zp - 1; wraps above 2^BITS - 1)
      zz = zz > MASK ? 0u : zz;
      nzs[t][c] = -(float)zz * sc[t][c];
    }

  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const bool live = (k0 + 8 * i < K) && (jn < M);
    uint4 av = a[i];
    av.x = live ? av.x : 0u; av.y = live ? av.y : 0u; av.z = live ? av.z : 0u; av.w = live ? av.w : 0u;
    const bool second = 8 * i >= kb;  // 8 divides the group size and k0: a fragment lies in ONE group
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float s = second ? sc[1][c] : sc[0][c], nz = second ? nzs[1][c] : nzs[0][c];
      float v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = __builtin_fmaf((float)anyw_field<BITS>(w, c, 8 * i + t), s, nz);  // exact: see the header
      uint4 bq;
      bq.x = cvt_pair<IS_BF16>(v[0], v[1]);
      bq.y = cvt_pair<IS_BF16>(v[2], v[3]);
      bq.z = cvt_pair<IS_BF16>(v[4], v[5]);
      bq.w = cvt_pair<IS_BF16>(v[6], v[7]);
      acc[c] = mfma16<IS_BF16>(av, bq, acc[c]);
    }
  }
  // ---- reduce the 4 waves: D col = lane&15 -> column 4*jn + c, row m = 4*oct + r ------------------
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * 16 + 4 * oct + r) * 65 + 4 * jn + c] = acc[c][r];
  strip_finish<IS_BF16, 16>(red, tid, out, bias, y, partial, counter, M, N, splitk, slice);
}

template <bool IS_BF16, int BITS>
__global__ __launch_bounds__(256) void woq_gemv_anyw_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counters, int M, int64_t N, int K, int64_t NW, int G, int g_shift, int splitk) {
  woq_gemv_anyw_body<IS_BF16, BITS>(x, qweight, scales, qzeros, bias, y, partial, counters + blockIdx.x, M, N, K, NW, G, g_shift, splitk,
                                    (int)blockIdx.x, (int)blockIdx.y);
}

// the same workgroup with the activations gathered through k_order (PERM above)
template <bool IS_BF16, int BITS>
__global__ __launch_bounds__(256) void woq_gemv_anyw_perm_kernel(
    const uint16_t* __restrict__ x, const int32_t* __restrict__ k_order, const uint32_t* __restrict__ qweight,
    const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counters, int M, int64_t N, int K, int64_t NW, int G, int g_shift, int splitk) {
  woq_gemv_anyw_body<IS_BF16, BITS, true>(x, qweight, scales, qzeros, bias, y, partial, counters + blockIdx.x, M, N, K, NW, G, g_shift, splitk,
                                          (int)blockIdx.x, (int)blockIdx.y, k_order);
}

// Several modules of one width that multiply the SAME x (q / k / v; gate / up) in ONE launch (inc_woq_gemv_anyw_multi): grid =
// (the members' strips together) x K-slices.  The slice count depends on K and the width alone, so a member's strip is computed exactly as
// its single launch computes it: bit-identical.  Global strip b arrives on counters[b]; member p's slabs [slice][M][N_p] start at
// args.part_off[p] -- together the [slice][M][sum N] floats of the workspace.  PERM: member p gathers x through args.k_order[p].
template <bool IS_BF16, int BITS, bool PERM>
__global__ __launch_bounds__(256) void woq_gemv_anyw_multi_kernel(GemvBatch args, const uint16_t* __restrict__ x, float* __restrict__ partial,
                                                                  unsigned* __restrict__ counters, int M, int K, int G, int g_shift, int splitk) {
  const int b = (int)blockIdx.x;
  int p = 0;
#pragma unroll
  for (int i = 1; i < GEMV_MAX_BATCH; ++i)
    if (i < args.n && b >= args.first[i]) p = i;
  p = __builtin_amdgcn_readfirstlane(p);
  const int64_t N = args.N[p];
  constexpr int NP = AnywShape<BITS>::NP;
  woq_gemv_anyw_body<IS_BF16, BITS, PERM>(x, args.qweight[p], args.scales[p], args.qzeros[p], args.bias[p], args.y[p], partial + args.part_off[p],
                                          counters + b, M, N, K, (N + NP - 1) / NP, G, g_shift, splitk, b - args.first[p], (int)blockIdx.y,
                                          PERM ? args.k_order[p] : nullptr);
}

// k of one K-slice at this width, 0 for a width that is not this file's
int anyw_slice_k(int bits) {
  switch (bits) {
    case 1: return AnywShape<1>::SLICE_K;
    case 2: return AnywShape<2>::SLICE_K;
    case 3: return AnywShape<3>::SLICE_K;
    case 5: return AnywShape<5>::SLICE_K;
    case 6: return AnywShape<6>::SLICE_K;
    case 7: return AnywShape<7>::SLICE_K;
    default: return 0;
  }
}

// the shapes the kernel takes (host only): every slice of every strip has a workgroup, the strips' counters fit the counter block
bool anyw_shape_ok(int64_t M, int64_t N, int64_t K, int bits) {
  return anyw_slice_k(bits) != 0 && M >= 1 && M <= 16 && K > 0 && (K % 32) == 0 && K <= ((int64_t)1 << 30) && N >= 64 && (N % 4) == 0 &&
         ceil_div64(N, 64) * 4 <= WS_COUNTER_BYTES && ceil_div64(K, anyw_slice_k(bits)) <= 65535;
}

// the batch the kernel takes (host only): 2 .. 8 members of the single launch's shapes, all strips' counters in the counter block
bool anyw_multi_shape_ok(int n, int64_t M, const int64_t* N, int64_t K, int bits, int64_t* strips_out, int64_t* ntot_out) {
  if (n < 2 || n > GEMV_MAX_BATCH) return false;
  int64_t strips = 0, ntot = 0;
  for (int i = 0; i < n; ++i) {
    if (!anyw_shape_ok(M, N[i], K, bits)) return false;
    strips += ceil_div64(N[i], 64);
    ntot += N[i];
  }
  if (strips * 4 > WS_COUNTER_BYTES) return false;
  *strips_out = strips, *ntot_out = ntot;
  return true;
}

// group lookup by shift (g_shift_of): contiguous groups of a power of two >= 32, or one group (g_shift = -1); G = the number of groups
bool anyw_groups(int64_t K, int group_size, int* g_shift_out, int64_t* G_out) {
  const int gs = (group_size == -1 || group_size >= K) ? (int)K : group_size;
  *g_shift_out = g_shift_of(gs, K);
  if (*g_shift_out == -2) return false;
  *G_out = *g_shift_out < 0 ? 1 : ceil_div64(K, gs);
  return true;
}

int anyw_slices(int64_t M, int64_t N, int64_t K, int bits) { return anyw_shape_ok(M, N, K, bits) ? (int)ceil_div64(K, anyw_slice_k(bits)) : 0; }

// inc_woq_gemv_anyw (k_order == NULL: x in 16-byte pieces) and inc_woq_gemv_anyw_perm (x gathered 2 bytes at a time through 32-bit byte
// offsets): the same checks, the same grid, the PERM instantiation of the same body
int anyw_single(const void* x, int xdtype, const int32_t* k_order, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                const void* bias, void* y, int64_t M, int64_t N, int64_t K, int64_t G, int group_size, int bits, void* workspace,
                int64_t workspace_bytes, inc_stream_t stream) {
  if (!(xdtype == INC_BF16 || xdtype == INC_F16) || !anyw_shape_ok(M, N, K, bits)) return INC_ERR_UNSUPPORTED;
  int g_shift;
  int64_t G_want;
  if (!anyw_groups(K, group_size, &g_shift, &G_want)) return INC_ERR_UNSUPPORTED;
  INC_CHECK_ARG(G == G_want);
  if (((reinterpret_cast<uintptr_t>(k_order ? (const void*)k_order : x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(qweight)) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(scales) & 7) != 0 || (k_order && M * K >= ((int64_t)1 << 31)))
    return INC_ERR_UNSUPPORTED;
  const int splitk = anyw_slices(M, N, K, bits);
  if (splitk > 1 && (!workspace || workspace_bytes < WS_COUNTER_BYTES + (int64_t)splitk * M * N * 4)) return INC_ERR_WORKSPACE;
  const auto [counters, part] = ws_parts(workspace, splitk > 1);
  const dim3 grid((unsigned)ceil_div64(N, 64), (unsigned)splitk);
  const bool bf = xdtype == INC_BF16;
#define INC_ANYW_ARGS(B) (const uint32_t*)qweight, scales, (const uint32_t*)qzeros, (const uint16_t*)bias, (uint16_t*)y, part, counters, (int)M, N, (int)K, ceil_div64(N, 32 / B), (int)G, g_shift, splitk
#define INC_ANYW(B)                                                                                                                          \
  case B:                                                                                                                                    \
    if (k_order && bf) woq_gemv_anyw_perm_kernel<true, B><<<grid, 256, 0, inc_s(stream)>>>((const uint16_t*)x, k_order, INC_ANYW_ARGS(B));   \
    else if (k_order) woq_gemv_anyw_perm_kernel<false, B><<<grid, 256, 0, inc_s(stream)>>>((const uint16_t*)x, k_order, INC_ANYW_ARGS(B));   \
    else if (bf) woq_gemv_anyw_kernel<true, B><<<grid, 256, 0, inc_s(stream)>>>((const uint16_t*)x, INC_ANYW_ARGS(B));                       \
    else woq_gemv_anyw_kernel<false, B><<<grid, 256, 0, inc_s(stream)>>>((const uint16_t*)x, INC_ANYW_ARGS(B));                              \
    break;
  switch (bits) {
    INC_ANYW(1) INC_ANYW(2) INC_ANYW(3) INC_ANYW(5) INC_ANYW(6) INC_ANYW(7)
    default: return INC_ERR_UNSUPPORTED;
  }
#undef INC_ANYW
#undef INC_ANYW_ARGS
  INC_LAUNCH_RETURN();
}

}  // namespace

extern "C" {

int inc_woq_gemv_anyw_slices(int64_t M, int64_t N, int64_t K, int bits) {
  return anyw_slices(M, N, K, bits);
}

int64_t inc_woq_gemv_anyw_workspace_bytes(int64_t M, int64_t N, int64_t K, int bits) {
  const int slices = inc_woq_gemv_anyw_slices(M, N, K, bits);
  return slices > 1 ? WS_COUNTER_BYTES + (int64_t)slices * M * N * 4 : 0;
}

int inc_woq_gemv_anyw(const void* x, int xdtype, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, const void* bias,
                      void* y, int64_t M, int64_t N, int64_t K, int64_t G, int group_size, int bits, void* workspace,
                      int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && qweight && scales && qzeros && y && N > 0 && K > 0 && G > 0 && (group_size > 0 || group_size == -1));
  return anyw_single(x, xdtype, nullptr, qweight, scales, qzeros, bias, y, M, N, K, G, group_size, bits, workspace, workspace_bytes, stream);
}

// ---- act_order decode in one launch: y = x[:, k_order] W_sorted^T + bias (PERM) -------------------------------------------------------
int inc_woq_gemv_anyw_perm(const void* x, int xdtype, const int32_t* k_order, const int32_t* qweight, const uint16_t* scales,
                           const int32_t* qzeros, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int64_t G, int group_size,
                           int bits, void* workspace, int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && k_order && qweight && scales && qzeros && y && N > 0 && K > 0 && G > 0 && (group_size > 0 || group_size == -1));
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 1) == 0);
  return anyw_single(x, xdtype, k_order, qweight, scales, qzeros, bias, y, M, N, K, G, group_size, bits, workspace, workspace_bytes, stream);
}

// ---- modules that share x, one launch --------------------------------------------------------------------------------------------------
int64_t inc_woq_gemv_anyw_multi_workspace_bytes(int n, int64_t M, const int64_t* N, int64_t K, int bits) {
  int64_t strips, ntot;
  if (!N || !anyw_multi_shape_ok(n, M, N, K, bits, &strips, &ntot)) return 0;
  const int64_t slices = ceil_div64(K, anyw_slice_k(bits));
  return slices > 1 ? WS_COUNTER_BYTES + slices * M * ntot * 4 : 0;
}

int inc_woq_gemv_anyw_multi(int n, const void* x, int xdtype, const int32_t* const* k_order, const int32_t* const* qweight,
                            const uint16_t* const* scales, const int32_t* const* qzeros, const void* const* bias, void* const* y, int64_t M,
                            const int64_t* N, int64_t K, int group_size, int bits, void* workspace, int64_t workspace_bytes,
                            inc_stream_t stream) {
  INC_CHECK_ARG(x && qweight && scales && qzeros && y && N && n > 0 && K > 0 && (group_size > 0 || group_size == -1));
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 1) == 0);
  int64_t strips, ntot;
  if (!(xdtype == INC_BF16 || xdtype == INC_F16) || !anyw_multi_shape_ok(n, M, N, K, bits, &strips, &ntot)) return INC_ERR_UNSUPPORTED;
  int g_shift;
  int64_t G;
  if (!anyw_groups(K, group_size, &g_shift, &G)) return INC_ERR_UNSUPPORTED;
  if (k_order ? M * K >= ((int64_t)1 << 31) : (reinterpret_cast<uintptr_t>(x) & 15) != 0) return INC_ERR_UNSUPPORTED;
  const int splitk = (int)ceil_div64(K, anyw_slice_k(bits));
  for (int i = 0; i < n; ++i) {
    INC_CHECK_ARG(qweight[i] && scales[i] && qzeros[i] && y[i] && (!k_order || k_order[i]));
    if (((reinterpret_cast<uintptr_t>(y[i]) | reinterpret_cast<uintptr_t>(qweight[i]) | (k_order ? reinterpret_cast<uintptr_t>(k_order[i]) : 0)) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(scales[i]) & 7) != 0)
      return INC_ERR_UNSUPPORTED;
  }
  GemvBatch args;
  const int64_t floats = gemv_batch_fill(&args, n, k_order, qweight, scales, qzeros, bias, y, splitk, M, N).floats;
  if (splitk > 1 && (!workspace || workspace_bytes < WS_COUNTER_BYTES + floats * 4)) return INC_ERR_WORKSPACE;
  const auto [counters, part] = ws_parts(workspace, splitk > 1);
  const dim3 grid((unsigned)strips, (unsigned)splitk);
  const bool bf = xdtype == INC_BF16, perm = k_order != nullptr;
#define INC_ANYW_MULTI(B)                                                                                                                    \
  case B:                                                                                                                                    \
    if (bf && perm) woq_gemv_anyw_multi_kernel<true, B, true><<<grid, 256, 0, inc_s(stream)>>>(args, (const uint16_t*)x, part, counters, (int)M, (int)K, (int)G, g_shift, splitk);        \
    else if (bf) woq_gemv_anyw_multi_kernel<true, B, false><<<grid, 256, 0, inc_s(stream)>>>(args, (const uint16_t*)x, part, counters, (int)M, (int)K, (int)G, g_shift, splitk);          \
    else if (perm) woq_gemv_anyw_multi_kernel<false, B, true><<<grid, 256, 0, inc_s(stream)>>>(args, (const uint16_t*)x, part, counters, (int)M, (int)K, (int)G, g_shift, splitk);        \
    else woq_gemv_anyw_multi_kernel<false, B, false><<<grid, 256, 0, inc_s(stream)>>>(args, (const uint16_t*)x, part, counters, (int)M, (int)K, (int)G, g_shift, splitk);                 \
    break;
  switch (bits) {
    INC_ANYW_MULTI(1) INC_ANYW_MULTI(2) INC_ANYW_MULTI(3) INC_ANYW_MULTI(5) INC_ANYW_MULTI(6) INC_ANYW_MULTI(7)
    default: return INC_ERR_UNSUPPORTED;
  }
#undef INC_ANYW_MULTI
  INC_LAUNCH_RETURN();
}

}  // extern "C"
