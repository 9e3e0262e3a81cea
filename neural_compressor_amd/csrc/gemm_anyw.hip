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
// Split-K: the sibling's hand-off, unchanged -- fp32 slabs stored write-through (`sc1`), every wave drains (`s_waitcnt vmcnt(0)`),
// barrier, ONE relaxed agent-scope ticket per strip; the last arriver re-arms the counter, sums the slices in slice order with `sc1`
// loads, adds the bias, rounds once and stores.  Bit-identical from call to call.
//
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): see the table above the kernel.
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

// Resource report of the cross-compile (VGPRs bf16 / fp16; every instantiation: 16 AGPRs, 40 SGPRs, 16640 bytes of LDS, 0 bytes of scratch):
//   1 bit 100 / 98     2 bits 112 / 110     3 bits 90 / 90     5 bits 110 / 110     6 bits 112 / 108     7 bits 106 / 104
// -> 4 waves per SIMD by registers (4 workgroups per CU), no scratch; the 16 AGPRs are the four accumulators.
template <bool IS_BF16, int BITS>
__global__ __launch_bounds__(256) void woq_gemv_anyw_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counters, int M, int64_t N, int K, int64_t NW, int G, int g_shift, int splitk) {
  using S = AnywShape<BITS>;
  constexpr int NP = S::NP, WL = S::WL, F = S::F, NF = S::NF;
  constexpr uint32_t MASK = (1u << BITS) - 1u;
  constexpr int NOUT = 16 * 64 / 256;  // outputs per thread of the strip
  __shared__ float red[4 * 16 * 65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jn = lane & 15, oct = lane >> 4;
  const int strip = (int)blockIdx.x, slice = (int)blockIdx.y;
  unsigned* const counter = counters + strip;
  const int64_t n0 = (int64_t)strip * 64;
  int64_t ncol = n0 + 4 * jn;
  if (ncol > N - 4) ncol = N - 4;  // clamped lanes recompute valid columns; their results are not stored
  const int rows_total = (K + NP - 1) / NP;
  const int row0 = ((slice * 4 + wave) * 4 + oct) * WL;
  const int k0 = row0 * NP;  // % 8 == 0

  // ---- issue every load of this wave up front: weights first ------------------------------------
  uint4 w[WL], a[NF];
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
    a[i] = *reinterpret_cast<const uint4*>(x + (int64_t)am * K + kk);
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
  // this thread's outputs of the strip: idx = tid + 256*i -> row idx>>6, column idx&63; bias fetched now
  uint16_t braw[NOUT];
  const uint16_t* const bsrc = bias ? bias : scales;  // always a valid address: the loads stay unconditional
  bool out_ok[NOUT];
  int64_t out_off[NOUT];
#pragma unroll
  for (int i = 0; i < NOUT; ++i) {
    const int idx = tid + 256 * i, m = idx >> 6, c = idx & 63;
    out_ok[i] = m < M && n0 + c < N;
    out_off[i] = out_ok[i] ? (int64_t)m * N + n0 + c : 0;
    braw[i] = bsrc[out_ok[i] ? n0 + c : 0];
  }
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
  __syncthreads();
  float sum[NOUT];
#pragma unroll
  for (int i = 0; i < NOUT; ++i) {
    const int idx = tid + 256 * i, m = idx >> 6, c = idx & 63;
    sum[i] = red[(0 * 16 + m) * 65 + c] + red[(1 * 16 + m) * 65 + c] + red[(2 * 16 + m) * 65 + c] + red[(3 * 16 + m) * 65 + c];
  }
  if (splitk > 1) {
    const int64_t slab = (int64_t)M * N;
#pragma unroll
    for (int i = 0; i < NOUT; ++i)
      if (out_ok[i]) __hip_atomic_store(&partial[(int64_t)slice * slab + out_off[i]], sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
    // publish: every wave drains its write-through stores, then one relaxed agent-scope ticket from lane 0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = ticket == (unsigned)(splitk - 1);
      if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next call
      red[0] = last ? 1.f : 0.f;
    }
    __syncthreads();
    if (red[0] == 0.f) return;
    // last arriver: fixed-order sum over the slices, up to 32 partial loads of this thread in flight at a time
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
#pragma unroll
  for (int i = 0; i < NOUT; ++i)
    if (out_ok[i]) {
      const float v = sum[i] + (bias ? cvt16<IS_BF16>(braw[i]) : 0.f);
      y[out_off[i]] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
    }
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

}  // namespace

extern "C" {

int inc_woq_gemv_anyw_slices(int64_t M, int64_t N, int64_t K, int bits) {
  if (!anyw_shape_ok(M, N, K, bits)) return 0;
  return (int)ceil_div64(K, anyw_slice_k(bits));
}

int64_t inc_woq_gemv_anyw_workspace_bytes(int64_t M, int64_t N, int64_t K, int bits) {
  const int slices = inc_woq_gemv_anyw_slices(M, N, K, bits);
  return slices > 1 ? WS_COUNTER_BYTES + (int64_t)slices * M * N * 4 : 0;
}

int inc_woq_gemv_anyw(const void* x, int xdtype, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, const void* bias,
                      void* y, int64_t M, int64_t N, int64_t K, int64_t G, int group_size, int bits, void* workspace,
                      int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && qweight && scales && qzeros && y && N > 0 && K > 0 && G > 0 && (group_size > 0 || group_size == -1));
  if (!(xdtype == INC_BF16 || xdtype == INC_F16) || !anyw_shape_ok(M, N, K, bits)) return INC_ERR_UNSUPPORTED;
  const int gs = (group_size == -1 || group_size >= K) ? (int)K : group_size;
  int g_shift = -1;  // one group
  if (gs < K) {
    if (gs < 32 || (gs & (gs - 1)) != 0) return INC_ERR_UNSUPPORTED;
    g_shift = __builtin_ctz((unsigned)gs);
  }
  INC_CHECK_ARG(G == (g_shift < 0 ? 1 : ceil_div64(K, gs)));
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(qweight)) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(scales) & 7) != 0)
    return INC_ERR_UNSUPPORTED;
  const int splitk = inc_woq_gemv_anyw_slices(M, N, K, bits);
  if (splitk > 1 && (!workspace || workspace_bytes < inc_woq_gemv_anyw_workspace_bytes(M, N, K, bits))) return INC_ERR_WORKSPACE;
  unsigned* const counters = (unsigned*)workspace;
  float* const part = splitk > 1 ? (float*)((char*)workspace + WS_COUNTER_BYTES) : nullptr;
  const dim3 grid((unsigned)ceil_div64(N, 64), (unsigned)splitk);
  const bool bf = xdtype == INC_BF16;
#define INC_ANYW(B)                                                                                                                          \
  case B:                                                                                                                                    \
    if (bf) woq_gemv_anyw_kernel<true, B><<<grid, 256, 0, inc_s(stream)>>>((const uint16_t*)x, (const uint32_t*)qweight, scales, (const uint32_t*)qzeros, \
        (const uint16_t*)bias, (uint16_t*)y, part, counters, (int)M, N, (int)K, ceil_div64(N, 32 / B), (int)G, g_shift, splitk);            \
    else woq_gemv_anyw_kernel<false, B><<<grid, 256, 0, inc_s(stream)>>>((const uint16_t*)x, (const uint32_t*)qweight, scales, (const uint32_t*)qzeros, \
        (const uint16_t*)bias, (uint16_t*)y, part, counters, (int)M, N, (int)K, ceil_div64(N, 32 / B), (int)G, g_shift, splitk);            \
    break;
  switch (bits) {
    INC_ANYW(1) INC_ANYW(2) INC_ANYW(3) INC_ANYW(5) INC_ANYW(6) INC_ANYW(7)
    default: return INC_ERR_UNSUPPORTED;
  }
#undef INC_ANYW
  INC_LAUNCH_RETURN();
}

}  // extern "C"
