// gemm_tile.hip -- the two general kernels of the fused dequant-GEMM (inc_woq_gemm, gemm.hip): they take every width, group size and
// g_idx, and whatever the specialised kernels of the other gemm_*.hip files decline.
//   woq_gemm_tile   M > 16 : 128x128x64 workgroup tile, 2x2 waves of 64x64 (MFMA 32x32x16), x and the
//                   dequantised weights double-buffered in LDS (pitch 144 B, conflict-free b128 access),
//                   next tile prefetched into registers while the current one is multiplied.
//   woq_gemm_small  M <= 16: HBM-bound.  MFMA 16x16x32 with the 16 rows of x as the A operand; each lane
//                   loads 16 B (4 columns) of qweight per packed row, the 4 waves of a workgroup split
//                   the K range, reduce through LDS, and write one fp32 partial per K-slice which the
//                   epilogue kernel sums (+bias) and converts.
#include "gemm_common.hpp"

namespace {

constexpr int GM = 128, GN = 128, GK = 64;
constexpr int GP = GK + 8;  // LDS pitch (elements) = 144 B

template <int BITS, bool IS_BF16>
__global__ __launch_bounds__(256) void woq_gemm_tile_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight,
    const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros,
    const int32_t* __restrict__ g_idx, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    int64_t M, int64_t N, int64_t K, int64_t KW, int64_t NW, int group_size, int x_vec_ok) {
  constexpr int NP = 32 / BITS;        // k per packed word
  // 4 / 8 bits: a K-step is a whole number of words and a thread dequantises whole words.  Every other width the reference's
  // configs tune (1, 2, 3, 5, 6, 7: n_pack = 32 // bits, modules.py:231 -- 10 / 6 / 5 / 4 fields with unused high bits for 3 / 5 / 6
  // / 7) takes the ANYW form: a thread owns 32 consecutive k of one column, fetches the <= MAXW words they live in and places
  // every field by its own k (per-element group lookup, so any group_size and any g_idx).
  constexpr bool ANYW = !(BITS == 4 || BITS == 8);
  constexpr int MAXW = (31 + NP - 1) / NP + 1;  // words a run of 32 k can touch
  constexpr int WPT = ANYW ? 1 : GK / NP;         // packed rows per K-step
  constexpr int BW = ANYW ? MAXW : (WPT * GN) / 256; // words per thread per K-step (4-bit: 4, 8-bit: 8)
  constexpr int DW = ANYW ? 1 : NP / 2;           // dwords per dequantised word
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint16_t* smem = reinterpret_cast<uint16_t*>(smem_raw);
  constexpr int OPER = GM * GP;  // elements per operand stage (GM == GN)

  // XCD-aware tile order: consecutive workgroup ids land on different XCDs (id % 8), so give each
  // XCD a contiguous run of N-tiles of the same M-row-panel -> x panel and weight columns hit in L2.
  const int tiles_n = (int)((N + GN - 1) / GN);
  const int tiles_m = (int)((M + GM - 1) / GM);
  const int nwg = tiles_m * tiles_n;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
  const int64_t m0 = (int64_t)tm * GM, n0 = (int64_t)tn * GN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // staging assignments
  //   x: 1024 16-byte chunks per K-step, 4 per thread: chunk c = tid + 256*i -> row c/8, k-chunk c%8
  //   w: WPT*128 words per K-step: n = tid & 127, packed row = (tid>>7) + 2*i
  uint4 xa[4];
  uint32_t wb[BW];
  GroupQ gq[BW];
  const int bn = tid & 127;
  const int64_t ncol = n0 + bn;

  int64_t fetched_k0 = 0;  // K offset of the words held in wb (per-element g_idx lookups happen when they are dequantised)
  auto fetch = [&](int kt) {
    const int64_t k0 = (int64_t)kt * GK;
    fetched_k0 = k0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      const int64_t row = m0 + (c >> 3), k = k0 + (c & 7) * 8;
      if (row < M && x_vec_ok && k + 8 <= K) {
        xa[i] = *reinterpret_cast<const uint4*>(x + row * K + k);
      } else {
        uint16_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = (row < M && k + j < K) ? x[row * K + k + j] : (uint16_t)0;
        xa[i] = make_uint4((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16),
                           (uint32_t)e[4] | ((uint32_t)e[5] << 16), (uint32_t)e[6] | ((uint32_t)e[7] << 16));
      }
    }
    if constexpr (ANYW) {
      const int64_t kwf = (k0 + 32 * (tid >> 7)) / NP;  // first word of this thread's 32 k
#pragma unroll
      for (int i = 0; i < BW; ++i) wb[i] = (ncol < N && kwf + i < KW) ? qweight[(kwf + i) * N + ncol] : 0u;
    } else {
#pragma unroll
      for (int i = 0; i < BW; ++i) {
        const int64_t kw = k0 / NP + (tid >> 7) + 2 * i;
        if (ncol < N && kw < KW) {
          wb[i] = qweight[kw * N + ncol];
          const int64_t kk = kw * NP;
          const int64_t g = g_idx ? (int64_t)g_idx[kk] : kk / group_size;
          gq[i] = load_group<BITS>(scales, qzeros, g, ncol, N, NW);
        } else {
          wb[i] = 0;
          gq[i].s = 0.f;
          gq[i].z = 0;
        }
      }
    }
  };
  auto stash = [&](int stage) {
    uint16_t* As = smem + (stage * 2 + 0) * OPER;
    uint16_t* Bs = smem + (stage * 2 + 1) * OPER;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<uint4*>(As + (c >> 3) * GP + (c & 7) * 8) = xa[i];
    }
    if constexpr (ANYW) {
      constexpr uint32_t MASK = (1u << BITS) - 1u;
      const int kl0 = 32 * (tid >> 7);                 // first k of this thread inside the K-step
      const int64_t kbeg = fetched_k0 + kl0;
      const int64_t kwf = kbeg / NP;
      uint16_t* dst = Bs + bn * GP;
      if (ncol >= N || kbeg + 32 > K) {                // columns past N / the K tail multiply as zeros
#pragma unroll
        for (int q8 = 0; q8 < 4; ++q8) *reinterpret_cast<uint4*>(dst + kl0 + 8 * q8) = make_uint4(0u, 0u, 0u, 0u);
      }
      if (ncol < N) {
        int gprev = -1;
        GroupQ gcur;
        gcur.s = 0.f;
        gcur.z = 0;
#pragma unroll
        for (int i = 0; i < BW; ++i) {
#pragma unroll
          for (int e = 0; e < NP; ++e) {
            const int64_t k = (kwf + i) * NP + e;
            if (k >= kbeg && k < kbeg + 32 && k < K) {
              const int g = g_idx ? g_idx[k] : (int)((uint32_t)k / (uint32_t)group_size);  // (K < 2^31: inc_woq_gemm checks)
              if (g != gprev) {
                gcur = load_group<BITS>(scales, qzeros, g, ncol, N, NW);
                gprev = g;
              }
              const int q = (int)((wb[i] >> (BITS * e)) & MASK);
              const float v = (float)(int8_t)(q - gcur.z) * gcur.s;
              dst[k - fetched_k0] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
            }
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < BW; ++i) {
        const int kwl = (tid >> 7) + 2 * i;
        uint32_t d[DW];
        if (g_idx && ncol < N && fetched_k0 / NP + kwl < KW)
          dequant_word_gidx<BITS, IS_BF16>(wb[i], scales, qzeros, g_idx, fetched_k0 + (int64_t)kwl * NP, K, ncol, N, NW, d);
        else
          dequant_word<BITS, IS_BF16>(wb[i], gq[i], d);
        if constexpr (DW == 4) {
          *reinterpret_cast<uint4*>(Bs + bn * GP + kwl * NP) = make_uint4(d[0], d[1], d[2], d[3]);
        } else {
          *reinterpret_cast<uint2*>(Bs + bn * GP + kwl * NP) = make_uint2(d[0], d[1]);
        }
      }
    }
  };

  const int nk = (int)((K + GK - 1) / GK);
  fetch(0);
  stash(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) fetch(kt + 1);
    const uint16_t* As = smem + (cur * 2 + 0) * OPER + (wr * 64) * GP;
    const uint16_t* Bs = smem + (cur * 2 + 1) * OPER + (wc * 64) * GP;
#pragma unroll
    for (int kk = 0; kk < GK / 16; ++kk) {
      const int koff = kk * 16 + 8 * (lane >> 5);
      uint4 a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = *reinterpret_cast<const uint4*>(As + (m * 32 + (lane & 31)) * GP + koff);
        b[m] = *reinterpret_cast<const uint4*>(Bs + (m * 32 + (lane & 31)) * GP + koff);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = mfma32<IS_BF16>(a[m], b[n], acc[m][n]);
    }
    if (kt + 1 < nk) stash(cur ^ 1);
    __syncthreads();
  }

  // epilogue: D col = lane&31 (n), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (m)
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int64_t col = n0 + wc * 64 + n * 32 + (lane & 31);
    const float bv = (bias && col < N) ? cvt16<IS_BF16>(bias[col]) : 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M && col < N) {
          const float v = acc[m][n][r] + bv;
          y[row * N + col] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
        }
      }
    }
  }
}

constexpr int SN = 64;  // columns per workgroup strip (16 lanes x 4 columns)

template <int BITS, bool IS_BF16>
__global__ __launch_bounds__(256) void woq_gemm_small_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight,
    const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros,
    const int32_t* __restrict__ g_idx, float* __restrict__ partial, int64_t M, int64_t N, int64_t K,
    int64_t KW, int64_t NW, int group_size, int kw_per_slice) {
  constexpr int NP = 32 / BITS;
  constexpr int STEP_KW = 32 / NP;  // packed rows per MFMA K=32 step (4-bit: 4, 8-bit: 8)
  __shared__ float red[4][16][SN + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * SN;
  const int slice = blockIdx.y;
  // this wave's packed-row range inside the slice
  const int per_wave = kw_per_slice / 4;
  const int64_t kw_beg = (int64_t)slice * kw_per_slice + (int64_t)wave * per_wave;
  const int64_t kw_end = kw_beg + per_wave;

  const int jn = lane & 15, koct = lane >> 4;  // column quad index, k-octet index (0..3)
  const int64_t ncol = n0 + 4 * jn;            // first of this lane's 4 columns
  const int am = lane & 15;                    // A row (m)
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t kw = kw_beg; kw < kw_end; kw += STEP_KW) {
    // A fragment: x[m = lane&15][k = 32*step + 8*koct .. +7]
    const int64_t ka = kw * NP + 8 * koct;
    uint4 a;
    if (am < M && ka + 8 <= K) {
      const uint16_t* p = x + (int64_t)am * K + ka;
      if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        a = *reinterpret_cast<const uint4*>(p);
      } else {
        a = make_uint4((uint32_t)p[0] | ((uint32_t)p[1] << 16), (uint32_t)p[2] | ((uint32_t)p[3] << 16),
                       (uint32_t)p[4] | ((uint32_t)p[5] << 16), (uint32_t)p[6] | ((uint32_t)p[7] << 16));
      }
    } else {
      uint16_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = (am < M && ka + j < K) ? x[(int64_t)am * K + ka + j] : (uint16_t)0;
      a = make_uint4((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16),
                     (uint32_t)e[4] | ((uint32_t)e[5] << 16), (uint32_t)e[6] | ((uint32_t)e[7] << 16));
    }
    // B fragments: this lane's k-octet of 4 adjacent columns.
    uint4 b[4];
    if constexpr (BITS == 4) {
      const int64_t kwr = kw + koct;  // one packed row holds the whole octet
      uint32_t w4[4] = {0, 0, 0, 0};
      if (kwr < KW) {
        if (ncol + 4 <= N && (N % 4 == 0)) {
          const uint4 v = *reinterpret_cast<const uint4*>(qweight + kwr * N + ncol);
          w4[0] = v.x; w4[1] = v.y; w4[2] = v.z; w4[3] = v.w;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) w4[c] = (ncol + c < N) ? qweight[kwr * N + ncol + c] : 0u;
        }
      }
      const int64_t kk = kwr * NP;
      const int64_t g = (kwr < KW) ? (g_idx ? (int64_t)g_idx[kk] : kk / group_size) : 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        GroupQ gq;
        if (ncol + c < N && kwr < KW) gq = load_group<4>(scales, qzeros, g, ncol + c, N, NW);
        else { gq.s = 0.f; gq.z = 0; }
        uint32_t d[4];
        if (g_idx && ncol + c < N && kwr < KW) dequant_word_gidx<4, IS_BF16>(w4[c], scales, qzeros, g_idx, kk, K, ncol + c, N, NW, d);
        else dequant_word<4, IS_BF16>(w4[c], gq, d);
        b[c] = make_uint4(d[0], d[1], d[2], d[3]);
      }
    } else {  // 8-bit: an octet spans two packed rows
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t kwr = kw + 2 * koct + h;
          if (kwr < KW && ncol + c < N) {
            const uint32_t word = qweight[kwr * N + ncol + c];
            const int64_t kk = kwr * NP;
            const int64_t g = g_idx ? (int64_t)g_idx[kk] : kk / group_size;
            const GroupQ gq = load_group<8>(scales, qzeros, g, ncol + c, N, NW);
            uint32_t dd[2];
            if (g_idx) dequant_word_gidx<8, IS_BF16>(word, scales, qzeros, g_idx, kk, K, ncol + c, N, NW, dd);
            else dequant_word<8, IS_BF16>(word, gq, dd);
            d[2 * h] = dd[0];
            d[2 * h + 1] = dd[1];
          }
        }
        b[c] = make_uint4(d[0], d[1], d[2], d[3]);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = mfma16<IS_BF16>(a, b[c], acc[c]);
  }
  // D: col = lane&15 -> column quad jn, sub-column c; row m = 4*(lane>>4) + r
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][4 * koct + r][4 * jn + c] = acc[c][r];
  __syncthreads();
  for (int idx = tid; idx < 16 * SN; idx += 256) {
    const int m = idx / SN, c = idx - m * SN;
    if (m < M && n0 + c < N) {
      const float v = red[0][m][c] + red[1][m][c] + red[2][m][c] + red[3][m][c];
      partial[((int64_t)slice * M + m) * N + n0 + c] = v;
    }
  }
}

template <bool IS_BF16>
__global__ void splitk_reduce_kernel(const float* __restrict__ partial, const uint16_t* __restrict__ bias,
                                     uint16_t* __restrict__ y, int64_t M, int64_t N, int slices) {
  const int64_t total = M * N;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < slices; ++s) v += partial[(int64_t)s * total + i];
    if (bias) v += cvt16<IS_BF16>(bias[i % N]);
    y[i] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
  }
}

}  // namespace

// the instantiation of width `bits` (1 .. 8: woq_gemm_plan rejects every other value), found by walking B = 1 .. 8
template <int B = 1>
static int launch_tile(const WoqGemmArgs& a, const int32_t* g_idx, int bits, int group_size, int x_vec_ok) {
  if constexpr (B < 8)
    if (bits != B) return launch_tile<B + 1>(a, g_idx, bits, group_size, x_vec_ok);
  const size_t smem = (size_t)2 * 2 * GM * GP * sizeof(uint16_t);
  const unsigned grid = (unsigned)(ceil_div64(a.M, GM) * ceil_div64(a.N, GN));
  const int64_t KW = ceil_div64(a.K, 32 / B);
  static std::atomic<uint64_t> aset{0};
  if (inc_attr_needed(aset)) {
    (void)hipFuncSetAttribute((const void*)woq_gemm_tile_kernel<B, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    (void)hipFuncSetAttribute((const void*)woq_gemm_tile_kernel<B, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    inc_attr_done(aset);
  }
  if (a.bf) woq_gemm_tile_kernel<B, true><<<grid, 256, smem, a.s>>>(a.x, a.qw, a.scales, a.qz, g_idx, a.bias, a.y, a.M, a.N, a.K, KW, a.NW, group_size, x_vec_ok);
  else woq_gemm_tile_kernel<B, false><<<grid, 256, smem, a.s>>>(a.x, a.qw, a.scales, a.qz, g_idx, a.bias, a.y, a.M, a.N, a.K, KW, a.NW, group_size, x_vec_ok);
  INC_LAUNCH_RETURN();
}
int inc_launch_woq_gemm_tile(const WoqGemmArgs& a, const int32_t* g_idx, int bits, int group_size, int x_vec_ok) {
  return launch_tile(a, g_idx, bits, group_size, x_vec_ok);
}

// choose the number of K-slices for the small-M kernel: enough workgroups to cover the chip, each
// slice a multiple of 4 waves x one MFMA K=32 step
int inc_woq_gemm_small_slices(int64_t N, int64_t K, int bits, int* kw_per_slice_out) {
  const int np = 32 / bits;
  const int64_t KW = ceil_div64(K, np);
  const int step_kw = 32 / np;
  const int64_t strips = ceil_div64(N, SN);
  const int64_t unit = 4 * step_kw;              // packed rows per workgroup per MFMA round
  const int64_t units = ceil_div64(KW, unit);     // rounds available along K
  int64_t want = ceil_div64(1024, strips);        // ~1024 workgroups
  if (want < 1) want = 1;
  if (want > units) want = units;
  if (want > 64) want = 64;
  const int64_t units_per_slice = ceil_div64(units, want);
  const int slices = (int)ceil_div64(units, units_per_slice);
  *kw_per_slice_out = (int)(units_per_slice * unit);
  return slices;
}

int inc_launch_woq_gemm_small(const WoqGemmArgs& a, const int32_t* g_idx, int bits, int group_size, float* part, int slices, int kw_per_slice) {
  const int64_t KW = ceil_div64(a.K, 32 / bits);
  dim3 grid((unsigned)ceil_div64(a.N, SN), (unsigned)slices);
#define INC_SMALL(B, F) woq_gemm_small_kernel<B, F><<<grid, 256, 0, a.s>>>(a.x, a.qw, a.scales, a.qz, g_idx, part, a.M, a.N, a.K, KW, a.NW, group_size, kw_per_slice)
  if (bits == 4) { if (a.bf) INC_SMALL(4, true); else INC_SMALL(4, false); }
  else { if (a.bf) INC_SMALL(8, true); else INC_SMALL(8, false); }
#undef INC_SMALL
  int64_t rb = ceil_div64(a.M * a.N, 256);
  if (rb > 2048) rb = 2048;
  if (a.bf) splitk_reduce_kernel<true><<<(unsigned)rb, 256, 0, a.s>>>(part, a.bias, a.y, a.M, a.N, slices);
  else splitk_reduce_kernel<false><<<(unsigned)rb, 256, 0, a.s>>>(part, a.bias, a.y, a.M, a.N, slices);
  INC_LAUNCH_RETURN();
}
