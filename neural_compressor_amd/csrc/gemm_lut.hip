// gemm_lut.hip -- K4d: fused 4-bit code-book / row-packed integer dequant + bf16/f16 MFMA GEMM.
//
// Replaces the non-optimum branch of INCWeightOnlyLinear.forward (reference neural_compressor/torch/algorithms/weight_only/
// modules.py:594-610), which recovers the dense weight (:413-443) and calls F.linear.  Covers the formats that never use the optimum
// layout: the NF4 / FP4 code books (modules.py:213-221, always use_optimum_format=False) and integer modules packed with
// use_optimum_format=False, compression_dim = 1 (modules.py:270-314): qweight [N, K / n_pack] of int8 / 16 / 32 / 64 words.
//
//   y[M,N] = x[M,K] . W^T + bias,   W[n,k] = rx( rs( (table[f(n,k)] - zp[n,g]) * scales[n,g] ) ),   g = k / group_size
//
// f(n,k) is field k of row n: byte n * row_bytes + k/2, low nibble for even k (for K % 16 == 0 every container of pack_rows gives the
// same bytes: little-endian fields, pack.hip).  `table` is 16 fp32 values filled by the caller: LUT[(f + 8) & 15] for a code book
// (the stored code is sign-extended then +8, modules.py unpack), f sign-extended for sym integers, f for asym integers.  rs rounds to
// the scale dtype (integers: inc_dequant_ints; for fp32 scales and fp16 x it rounds the exact product once, LUT_RND_EXACT16) or is
// the identity (code books multiply in fp32); rx rounds to the compute dtype.  So W is recover(dtype=x.dtype) bit for bit and y == F.linear(x, that, bias) up
// to the fp32 summation order, which is fixed (repeated calls are bit-identical).
//
// Kernel: one body for every M, 64 rows of x per workgroup (M tiles on grid.z).  A wave owns 16 output columns n (rows of qweight);
// lane (jn = lane & 15, oct = lane >> 4) loads 64 contiguous bytes of row n per 512-k super-step -- four 16-byte requests, 128 k,
// so the four oct lanes of a row read 256 contiguous bytes.  The k order inside an MFMA step is free as long as A and B agree: lane
// (jn, oct) supplies k = base + 128 oct + 32 c + 8 s + j (chunk c, word s, element j) as element j of its B fragment of MFMA step
// (c, s) (v_mfma_f32_16x16x32: lane l holds B[k = 8 (l >> 4) + j][col l & 15]), and the A lanes read x with the same map.
// Decode: a chunk of 32 k lies inside one group (group_size % 32 == 0), so per (row, group) the lane builds the 16 possible 16-bit
// weights once -- split into a low-byte table L and a high-byte table H of four dwords each -- and every nibble is then a byte select:
// v_perm_b32 picks among 8 entries, one v_bfi_b32 on bit 3 picks the half (sel16 below), two more perms interleave the bytes.
// Split-K across workgroups: fp32 partial slabs written through (sc1), one relaxed agent-scope ticket per (M tile, column strip) in
// the workspace's first 16 KiB, the last arriver sums the slabs in slice order, adds the bias and stores (the hand-off of gemm_stream.hip's
// streaming kernel).
#include "gemm_common.hpp"

namespace {

constexpr int64_t LUT_COUNTER_BYTES = 16 << 10;  // arrival counters: one uint32 per (M tile, 64-column strip)
constexpr int LUT_KSUP = 512;                    // k per super-step of a wave (4 lanes x 4 chunks x 32)

// rounding of (table - zp) * scale before the 16-bit conversion: INC_F32 (none: the fp32 product), INC_F16 / INC_BF16 (to the scale
// dtype), or LUT_RND_EXACT16: the exact product rounded ONCE to fp16 -- what inc_dequant_ints computes for fp32 scales and an fp16
// output (the compiler fuses its multiply and conversion into v_fma_mixlo_f16, a single rounding)
constexpr int LUT_RND_EXACT16 = -1;

struct LutTable {
  float v[16];  // by value in the kernel arguments: every use below has a constant index -> scalar loads
};

__device__ __forceinline__ float lut_load_scale(const void* p, int64_t i, int sdt) {
  if (sdt == INC_F32) return static_cast<const float*>(p)[i];
  const uint16_t b = static_cast<const uint16_t*>(p)[i];
  return sdt == INC_F16 ? f16_bits_to_f32(b) : bf16_bits_to_f32(b);
}

// 4 selector bytes (values 0..15) -> the 4 table bytes they name; T = 16 bytes in 4 dwords
__device__ __forceinline__ uint32_t sel16(uint32_t idx, const uint32_t (&T)[4]) {
  const uint32_t s = idx & 0x07070707u;
  const uint32_t a = __builtin_amdgcn_perm(T[1], T[0], s);  // entries 0..7
  const uint32_t b = __builtin_amdgcn_perm(T[3], T[2], s);  // entries 8..15
  const uint32_t m = ((idx >> 3) & 0x01010101u) * 0xFFu;    // 0xFF in the bytes whose index has bit 3 set
  return (b & m) | (a & ~m);
}

// the 16 weights of one (row, group): E[i] = (w[2i], w[2i+1]) as 16-bit pairs -> low-byte table L, high-byte table H
template <bool IS_BF16>
__device__ __forceinline__ void lut_build(const LutTable& tab, float s, float z, int rnd, uint32_t (&L)[4], uint32_t (&H)[4]) {
  uint32_t E[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (rnd == LUT_RND_EXACT16) {  // one rounding of the exact product (fp64 holds it: <= 5 x 24 significant bits)
      const _Float16 h0 = (_Float16)((double)(tab.v[2 * i] - z) * (double)s), h1 = (_Float16)((double)(tab.v[2 * i + 1] - z) * (double)s);
      uint16_t b0, b1;
      __builtin_memcpy(&b0, &h0, 2);
      __builtin_memcpy(&b1, &h1, 2);
      E[i] = (uint32_t)b0 | ((uint32_t)b1 << 16);
      continue;
    }
    float v0 = (tab.v[2 * i] - z) * s, v1 = (tab.v[2 * i + 1] - z) * s;
    if (rnd == INC_F16) {
      v0 = round_to<INC_F16>(v0);
      v1 = round_to<INC_F16>(v1);
    } else if (rnd == INC_BF16) {
      v0 = round_to<INC_BF16>(v0);
      v1 = round_to<INC_BF16>(v1);
    }
    E[i] = cvt_pair<IS_BF16>(v0, v1);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    L[j] = __builtin_amdgcn_perm(E[2 * j + 1], E[2 * j], 0x06040200u);
    H[j] = __builtin_amdgcn_perm(E[2 * j + 1], E[2 * j], 0x07050301u);
  }
}

// 8 nibbles (k0 .. k7 from the low end) -> 8 16-bit weights in k order, as the 4 dwords of a B fragment
__device__ __forceinline__ uint4 lut_decode(uint32_t w, const uint32_t (&L)[4], const uint32_t (&H)[4]) {
  const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;  // bytes: k0 k2 k4 k6 / k1 k3 k5 k7
  const uint32_t Ll = sel16(lo, L), Hl = sel16(lo, H), Lh = sel16(hi, L), Hh = sel16(hi, H);
  const uint32_t P = __builtin_amdgcn_perm(Hl, Ll, 0x05010400u);  // (k0, k2)
  const uint32_t Q = __builtin_amdgcn_perm(Hl, Ll, 0x07030602u);  // (k4, k6)
  const uint32_t R = __builtin_amdgcn_perm(Hh, Lh, 0x05010400u);  // (k1, k3)
  const uint32_t S = __builtin_amdgcn_perm(Hh, Lh, 0x07030602u);  // (k5, k7)
  uint4 o;
  o.x = __builtin_amdgcn_perm(R, P, 0x05040100u);  // (k0, k1)
  o.y = __builtin_amdgcn_perm(R, P, 0x07060302u);  // (k2, k3)
  o.z = __builtin_amdgcn_perm(S, Q, 0x05040100u);  // (k4, k5)
  o.w = __builtin_amdgcn_perm(S, Q, 0x07060302u);  // (k6, k7)
  return o;
}

// CPT = 32-k chunks per group table: 4 (group_size % 128 == 0 or one group), 2 (% 64), 1 (% 32).  MB = 16-row blocks of x.
template <bool IS_BF16, int CPT, int MB>
__global__ __launch_bounds__(256) void woq_gemm_lut_kernel(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ qweight, int64_t row_bytes, LutTable tab,
    const void* __restrict__ scales, int sdt, int rnd, const uint8_t* __restrict__ qzeros, int64_t zrow_bytes,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, float* __restrict__ partial, unsigned* __restrict__ counters,
    int64_t M, int64_t N, int64_t K, int64_t G, int64_t gs, int nsup, int splitk) {
  __shared__ int last_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jn = lane & 15, oct = lane >> 4;
  const int strip = (int)blockIdx.x, slice = (int)blockIdx.y, mt = (int)blockIdx.z;
  const int64_t n = (int64_t)strip * 64 + 16 * wave + jn;
  const bool n_ok = n < N;
  const int64_t nc = n_ok ? n : N - 1;  // clamped lanes recompute a valid row; their results are not stored
  const int64_t m0 = (int64_t)mt * 64;
  const int64_t ksup = (K + LUT_KSUP - 1) / LUT_KSUP;
  int64_t ss_end = (int64_t)(slice + 1) * nsup;
  if (ss_end > ksup) ss_end = ksup;
  const uint8_t* wrow = qweight + nc * row_bytes;
  const uint16_t* xrow[MB];
  bool m_ok[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    const int64_t am = m0 + 16 * b + jn;
    m_ok[b] = am < M;
    xrow[b] = x + (m_ok[b] ? am : M - 1) * K;  // rows >= M read row M - 1 and are zeroed below
  }

  f32x4 acc[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t ss = (int64_t)slice * nsup; ss < ss_end; ++ss) {
    const int64_t kl = ss * LUT_KSUP + 128 * oct;  // this lane's first k of the super-step
    uint4 w[4];
    bool k_ok[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int64_t k = kl + 32 * c;
      k_ok[c] = k < K;
      if (!k_ok[c]) k = K - 32;  // past-the-end chunks re-read the last one and are zeroed through A
      w[c] = *reinterpret_cast<const uint4*>(wrow + k / 2);
    }
    float sc[4 / CPT], zf[4 / CPT];
#pragma unroll
    for (int t = 0; t < 4 / CPT; ++t) {
      int64_t k = kl + 32 * CPT * t;
      if (k > K - 32) k = K - 32;
      const int64_t g = k / gs;
      sc[t] = lut_load_scale(scales, nc * G + g, sdt);
      zf[t] = qzeros ? (float)((qzeros[nc * zrow_bytes + (g >> 1)] >> (4 * (g & 1))) & 15) : 0.f;
    }
    uint32_t L[4], H[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c % CPT == 0) lut_build<IS_BF16>(tab, sc[c / CPT], zf[c / CPT], rnd, L, H);
      const int64_t k = k_ok[c] ? kl + 32 * c : K - 32;
      uint4 a[MB][4];
#pragma unroll
      for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          a[b][s] = *reinterpret_cast<const uint4*>(xrow[b] + k + 8 * s);
          if (!(m_ok[b] && k_ok[c])) a[b][s] = make_uint4(0u, 0u, 0u, 0u);
        }
      const uint32_t ww[4] = {w[c].x, w[c].y, w[c].z, w[c].w};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const uint4 bq = lut_decode(ww[s], L, H);
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[b] = mfma16<IS_BF16>(a[b][s], bq, acc[b]);
      }
    }
  }

  // D of 16x16x32: lane holds column jn (= output n) and rows 4 oct + r (= m) of each block
  const float bv = (bias && n_ok) ? cvt16<IS_BF16>(bias[n]) : 0.f;
  if (splitk > 1) {
    const int64_t slab = M * N;
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + 16 * b + 4 * oct + r;
        if (n_ok && m < M) __hip_atomic_store(&partial[(int64_t)slice * slab + m * N + n], acc[b][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
      }
    // publish: drain, barrier, one ticket (splitk_arrive, gemm_common.hpp)
    if (!splitk_arrive(counters + (int64_t)mt * gridDim.x + strip, splitk, &last_flag)) return;
    // last arriver: fixed-order sum over the slices (its own slab included)
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int sl = 0; sl < splitk; ++sl) {
#pragma unroll
      for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t m = m0 + 16 * b + 4 * oct + r;
          if (n_ok && m < M) acc[b][r] += __hip_atomic_load(&partial[(int64_t)sl * slab + m * N + n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
        }
    }
  }
  if (!n_ok) return;
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t m = m0 + 16 * b + 4 * oct + r;
      if (m < M) {
        const float v = acc[b][r] + bv;
        y[m * N + n] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
      }
    }
}

// split-K plan: about four workgroups per CU (256 CUs), whole super-steps per slice; no split when the (M tile, strip) pairs
// alone fill the chip or outnumber the counters
struct LutPlan {
  int splitk, nsup;
};
LutPlan lut_plan(int64_t M, int64_t N, int64_t K) {
  const int64_t ksup = ceil_div64(K, LUT_KSUP);
  const int64_t tiles = ceil_div64(N, 64) * ceil_div64(M, 64);
  int64_t sk = ceil_div64(1024, tiles);
  if (sk > ksup) sk = ksup;
  if (sk < 1 || tiles * 4 > LUT_COUNTER_BYTES) sk = 1;
  const int64_t nsup = ceil_div64(ksup, sk);
  return LutPlan{(int)ceil_div64(ksup, nsup), (int)nsup};
}

template <bool IS_BF16, int CPT>
int launch_lut(int MB, dim3 grid, hipStream_t s, const uint16_t* x, const uint8_t* qw, int64_t row_bytes, const LutTable& tab,
               const void* scales, int sdt, int rnd, const uint8_t* qz, int64_t zrow_bytes, const uint16_t* bias, uint16_t* y,
               float* part, unsigned* counters, int64_t M, int64_t N, int64_t K, int64_t G, int64_t gs, int nsup, int splitk) {
#define INC_LUT_LAUNCH(MBV)                                                                                                     \
  woq_gemm_lut_kernel<IS_BF16, CPT, MBV><<<grid, 256, 0, s>>>(x, qw, row_bytes, tab, scales, sdt, rnd, qz, zrow_bytes, bias, y, \
                                                              part, counters, M, N, K, G, gs, nsup, splitk)
  switch (MB) {
    case 1: INC_LUT_LAUNCH(1); break;
    case 2: INC_LUT_LAUNCH(2); break;
    case 3: INC_LUT_LAUNCH(3); break;
    default: INC_LUT_LAUNCH(4); break;
  }
#undef INC_LUT_LAUNCH
  INC_LAUNCH_RETURN();
}

}  // namespace

extern "C" {

// workspace layout: [0, 16 KiB) arrival counters (MUST be zero on first use, the kernel re-arms them), then splitk fp32 [M,N] slabs
int64_t inc_woq_gemm_lut_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const LutPlan p = lut_plan(M, N, K);
  return p.splitk > 1 ? LUT_COUNTER_BYTES + (int64_t)p.splitk * M * N * 4 : 0;
}

int inc_woq_gemm_lut(const void* x, int xdtype, const uint8_t* qweight, int64_t row_bytes, const float* table16, const void* scales,
                     int scale_dtype, int scale_round, const uint8_t* qzeros, int64_t zrow_bytes, const void* bias, void* y, int64_t M,
                     int64_t N, int64_t K, int64_t G, int group_size, void* workspace, int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(x && qweight && table16 && scales && y && M > 0 && N > 0 && K > 0 && G > 0 && (group_size > 0 || group_size == -1));
  INC_CHECK_ARG(!qzeros || zrow_bytes > 0);
  if (xdtype != INC_BF16 && xdtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if (scale_dtype != INC_F32 && scale_dtype != INC_F16 && scale_dtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  const int64_t gs = (group_size == -1 || group_size >= K) ? K : group_size;
  INC_CHECK_ARG(G == ceil_div64(K, gs) && (!qzeros || zrow_bytes * 2 >= G));
  if (K % 32 != 0 || (gs != K && gs % 32 != 0)) return INC_ERR_UNSUPPORTED;  // no 32-k chunk straddles a group
  if (row_bytes < K / 2 || row_bytes % 16 != 0) return INC_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(qweight) & 15)) return INC_ERR_UNSUPPORTED;
  if (ceil_div64(M, 64) > 65535 || ceil_div64(N, 64) > 0x7fffffff) return INC_ERR_UNSUPPORTED;
  const LutPlan p = lut_plan(M, N, K);
  const int64_t need = p.splitk > 1 ? LUT_COUNTER_BYTES + (int64_t)p.splitk * M * N * 4 : 0;
  if (need > 0 && (!workspace || workspace_bytes < need)) return INC_ERR_WORKSPACE;
  LutTable tab;
  for (int i = 0; i < 16; ++i) tab.v[i] = table16[i];
  const int cpt = (gs == K || gs % 128 == 0) ? 4 : (gs % 64 == 0 ? 2 : 1);
  const int MB = M >= 64 ? 4 : (int)ceil_div64(M, 16);
  const dim3 grid((unsigned)ceil_div64(N, 64), (unsigned)p.splitk, (unsigned)ceil_div64(M, 64));
  unsigned* counters = static_cast<unsigned*>(workspace);
  float* part = need > 0 ? reinterpret_cast<float*>(static_cast<char*>(workspace) + LUT_COUNTER_BYTES) : nullptr;
  const int rnd = !scale_round ? INC_F32 : (scale_dtype == INC_F32 && xdtype == INC_F16 ? LUT_RND_EXACT16 : scale_dtype);
  const auto* xx = static_cast<const uint16_t*>(x);
  const auto* bb = static_cast<const uint16_t*>(bias);
  auto* yy = static_cast<uint16_t*>(y);
  hipStream_t s = inc_s(stream);
#define INC_LUT_ARGS MB, grid, s, xx, qweight, row_bytes, tab, scales, scale_dtype, rnd, qzeros, zrow_bytes, bb, yy, part, counters, M, N, K, G, gs, p.nsup, p.splitk
  if (xdtype == INC_BF16) {
    if (cpt == 4) return launch_lut<true, 4>(INC_LUT_ARGS);
    if (cpt == 2) return launch_lut<true, 2>(INC_LUT_ARGS);
    return launch_lut<true, 1>(INC_LUT_ARGS);
  }
  if (cpt == 4) return launch_lut<false, 4>(INC_LUT_ARGS);
  if (cpt == 2) return launch_lut<false, 2>(INC_LUT_ARGS);
  return launch_lut<false, 1>(INC_LUT_ARGS);
#undef INC_LUT_ARGS
}

}  // extern "C"
