// gptq_hessian_moe.hip -- K5e: GPTQ Hessian accumulation for the experts of a fused MoE module, from ROUTED tokens.
//
// Reference (relative to /root/reference/neural_compressor/torch/algorithms/weight_only/gptq.py):
//   GPTQ.add_batch      :1111-1141   H <- H*n/(n+b) + (sqrt(2/(n+b)) X)^T (sqrt(2/(n+b)) X)
// applied to every expert of one module as if it were an nn.Linear fed the rows routed to it: one routed row is the unit of the
// running mean (n = rows folded so far, b = rows of this forward), so an expert's H is what the reference computes for the un-fused
// expert up to a positive factor and fp32 rounding.
//
// One launch updates H [E, K, K] of all experts from the route buffer inc_moe_route wrote (offsets [E+1], order [S]; K4e in the
// header): workgroup (tile, e) owns one 128 x 128 tile on / above the diagonal of H[e] and walks the rows offsets[e] ..
// offsets[e+1]-1 in steps of 64 -- gathered through order[p] / top_k (gate_up Hessian) or in place (down Hessian, the input is
// already in sorted order).  The row range comes from device memory, the grid from E and K alone: no host wait.  The tile body is
// K5's 128 x 128 form (hessian_syrk_16bit_kernel: 8 x 8 blocks transposed in registers, [feature][token] LDS image, MFMA 32x32x16
// with fp32 accumulation); rows past the end of a range are zero-filled, never read.  One workgroup sums its tile's rows in
// order, so repeated calls are bit-identical; nothing is added atomically.  An expert without a row in this forward returns
// before touching H[e].  rows[e] is read by every tile of e, so it is advanced by a second, one-workgroup launch behind the first.
// fp32 inputs (the tiny test models) take the exact-fp32 MFMA 32x32x2 with the same tiling; that form is not tuned.
#include "common.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int RB = 128;          // H tile edge (features)
constexpr int RK = 64;           // rows per pipeline step
constexpr int RPITCH = RK + 8;   // LDS row pitch in elements (144 B: ds_write_b128 and the fragment ds_read_b128 are conflict free)
constexpr int RFK = 32;          // rows per step of the fp32 form
constexpr int64_t ROUTED_MAX_E = 512;

__device__ __forceinline__ void tri_decode(int idx, int nt, int& ti, int& tj) {
  // idx -> (ti, tj), tj >= ti, row-major over the upper triangle
  int t = 0, rem = idx;
  while (rem >= nt - t) { rem -= nt - t; ++t; }
  ti = t;
  tj = t + rem;
}

// the row range of expert e in this forward, clamped to the slots that exist, and the running-mean factors
struct ExpertRange {
  int off, cnt;
  float beta, alpha;
};
__device__ __forceinline__ ExpertRange expert_range(const int32_t* __restrict__ route, const int64_t* __restrict__ rows, int e, int S) {
  ExpertRange r;
  const int o0 = route[1 + e], o1 = route[2 + e];  // offsets [E+1] start at int32 index 1
  r.off = o0 < 0 ? 0 : (o0 > S ? S : o0);
  const int end = o1 < r.off ? r.off : (o1 > S ? S : o1);
  r.cnt = end - r.off;
  const int64_t c = rows[e];
  const float tot = (float)(c + (int64_t)r.cnt);
  r.beta = c > 0 ? (float)c / tot : 0.f;
  r.alpha = 2.f / tot;
  return r;
}

// source row of position p (a position of the sorted order): the token of its slot (gather) or p itself (sorted input)
template <bool GATHER>
__device__ __forceinline__ int64_t source_row(const int32_t* __restrict__ order, int p, int top_k, int64_t T) {
  if constexpr (GATHER) {
    int64_t t = order[p] / top_k;
    return t < 0 ? 0 : (t >= T ? T - 1 : t);
  } else {
    return p;
  }
}

// one thread's 8(row) x 8(feature) block, zero-filled past the end of the range; K % 8 == 0 and 16-byte aligned rows
template <bool GATHER>
__device__ __forceinline__ void load_block8x8(const uint16_t* __restrict__ x, const int32_t* __restrict__ order, int off, int cnt,
                                              int top_k, int64_t T, int64_t K, int r0, int64_t f0, uint4 (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int rr = r0 + i;
    if (rr < cnt && f0 + 8 <= K)
      r[i] = *reinterpret_cast<const uint4*>(x + source_row<GATHER>(order, off + rr, top_k, T) * K + f0);
    else
      r[i] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// transpose the 8x8 16-bit block held as r[row][4 dwords] and store 8 LDS rows [feature][8 rows]
__device__ __forceinline__ void store_block_transposed(uint16_t* lds, int f_local, int t_local, const uint4 (&r)[8]) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&r[0]);  // w[row*4 + m]
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t a = w[(2 * p) * 4 + m], b = w[(2 * p + 1) * 4 + m];
      lo[p] = (a & 0xffffu) | (b << 16);
      hi[p] = (a >> 16) | (b & 0xffff0000u);
    }
    *reinterpret_cast<uint4*>(lds + (f_local + 2 * m) * RPITCH + t_local) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *reinterpret_cast<uint4*>(lds + (f_local + 2 * m + 1) * RPITCH + t_local) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  }
}

template <bool IS_BF16>
__device__ __forceinline__ f32x16 mfma16(const uint4& a, const uint4& b, f32x16 c) {
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

// D[row][col] of a 32x32 fragment: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ void store_tile(float* __restrict__ He, int64_t K, int64_t i0, int64_t j0, int wr, int wc, int lane,
                                           const f32x16 (&acc)[2][2], float beta, float alpha) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int64_t col = j0 + wc * 64 + n * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = i0 + wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < K && col < K) {
          float* p = He + row * K + col;
          *p = beta != 0.f ? beta * (*p) + alpha * acc[m][n][r] : alpha * acc[m][n][r];  // first fold: H[e] need not be initialised
        }
      }
    }
}

template <bool IS_BF16, bool GATHER>
__global__ __launch_bounds__(256) void hessian_routed_16bit_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ route,
                                                                   const int64_t* __restrict__ rows, float* __restrict__ H, int64_t T,
                                                                   int top_k, int E, int64_t K, int nt) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[2 * 2 * RB * RPITCH];  // [stage][operand i / j][RB][RPITCH], 72 KiB
  constexpr int OPER = RB * RPITCH;
  const int e = blockIdx.y;
  const int S = (int)(T * top_k);
  const ExpertRange er = expert_range(route, rows, e, S);
  if (er.cnt <= 0) return;  // not hit in this forward: H[e] is not touched
  const int32_t* __restrict__ order = route + 2 + E;
  int ti, tj;
  tri_decode(blockIdx.x, nt, ti, tj);
  const int64_t i0 = (int64_t)ti * RB, j0 = (int64_t)tj * RB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;  // 2x2 waves, 64x64 each
  // staging role: threads 0..127 fetch the i tile, 128..255 the j tile
  const int oper = tid >> 7, tt = tid & 127;
  const int t_chunk = tt & 7, f_chunk = tt >> 3;
  const int64_t fbase = (oper == 0 ? i0 : j0) + f_chunk * 8;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int nk = (er.cnt + RK - 1) / RK;
  uint4 regs[8];
  load_block8x8<GATHER>(x, order, er.off, er.cnt, top_k, T, K, t_chunk * 8, fbase, regs);
  store_block_transposed(smem + (0 * 2 + oper) * OPER, f_chunk * 8, t_chunk * 8, regs);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_block8x8<GATHER>(x, order, er.off, er.cnt, top_k, T, K, (kt + 1) * RK + t_chunk * 8, fbase, regs);
    const uint16_t* As = smem + (cur * 2 + 0) * OPER + (wr * 64) * RPITCH;
    const uint16_t* Bs = smem + (cur * 2 + 1) * OPER + (wc * 64) * RPITCH;
#pragma unroll
    for (int kk = 0; kk < RK / 16; ++kk) {
      const int koff = kk * 16 + 8 * (lane >> 5);
      uint4 a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = *reinterpret_cast<const uint4*>(As + (m * 32 + (lane & 31)) * RPITCH + koff);
        b[m] = *reinterpret_cast<const uint4*>(Bs + (m * 32 + (lane & 31)) * RPITCH + koff);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = mfma16<IS_BF16>(a[m], b[n], acc[m][n]);
    }
    if (kt + 1 < nk) store_block_transposed(smem + ((cur ^ 1) * 2 + oper) * OPER, f_chunk * 8, t_chunk * 8, regs);
    __syncthreads();
  }
  store_tile(H + (int64_t)e * K * K, K, i0, j0, wr, wc, lane, acc, er.beta, er.alpha);
}

// fp32 inputs: exact fp32 MFMA 32x32x2 (A / B = one f32 per lane: no transpose needed)
template <bool GATHER>
__global__ __launch_bounds__(256) void hessian_routed_f32_kernel(const float* __restrict__ x, const int32_t* __restrict__ route,
                                                                 const int64_t* __restrict__ rows, float* __restrict__ H, int64_t T,
                                                                 int top_k, int E, int64_t K, int nt) {
  __shared__ float As[RFK * RB];
  __shared__ float Bs[RFK * RB];
  const int e = blockIdx.y;
  const int S = (int)(T * top_k);
  const ExpertRange er = expert_range(route, rows, e, S);
  if (er.cnt <= 0) return;
  const int32_t* __restrict__ order = route + 2 + E;
  int ti, tj;
  tri_decode(blockIdx.x, nt, ti, tj);
  const int64_t i0 = (int64_t)ti * RB, j0 = (int64_t)tj * RB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  const int nk = (er.cnt + RFK - 1) / RFK;
  for (int kt = 0; kt < nk; ++kt) {
    // stage [RFK rows][128 features] of both operands (coalesced along features)
    for (int idx = tid; idx < RFK * RB; idx += 256) {
      const int t = idx / RB, f = idx - t * RB;
      const int rr = kt * RFK + t;
      const bool in = rr < er.cnt;
      const int64_t src = in ? source_row<GATHER>(order, er.off + rr, top_k, T) : 0;
      As[idx] = (in && i0 + f < K) ? x[src * K + i0 + f] : 0.f;
      Bs[idx] = (in && j0 + f < K) ? x[src * K + j0 + f] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < RFK / 2; ++s) {
      const int k = 2 * s + (lane >> 5);
      float a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = As[k * RB + wr * 64 + m * 32 + (lane & 31)];
        b[m] = Bs[k * RB + wc * 64 + m * 32 + (lane & 31)];
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[n], acc[m][n], 0, 0, 0);
    }
    __syncthreads();
  }
  store_tile(H + (int64_t)e * K * K, K, i0, j0, wr, wc, lane, acc, er.beta, er.alpha);
}

// rows[e] += the rows of this forward; runs behind the tile kernel, which reads rows[e] in every tile of e
__global__ __launch_bounds__(512) void hessian_routed_rows_kernel(const int32_t* __restrict__ route, int64_t* __restrict__ rows, int E,
                                                                  int S) {
  const int e = threadIdx.x;
  if (e >= E) return;
  const int o0 = route[1 + e], o1 = route[2 + e];
  const int off = o0 < 0 ? 0 : (o0 > S ? S : o0);
  const int end = o1 < off ? off : (o1 > S ? S : o1);
  if (end > off) rows[e] += (int64_t)(end - off);
}

}  // namespace

extern "C" {

int inc_gptq_hessian_accum_routed(const void* a, int xdtype, int mode, const int32_t* route, int64_t T, int top_k, int64_t E, int64_t K,
                                  float* H, int64_t* rows, inc_stream_t stream) {
  INC_CHECK_ARG(a && route && H && rows && T > 0 && top_k > 0 && E > 0 && K > 0 && (mode == 0 || mode == 1));
  if (!(xdtype == INC_F32 || xdtype == INC_F16 || xdtype == INC_BF16)) return INC_ERR_UNSUPPORTED;
  if (E > ROUTED_MAX_E || T * top_k > ((int64_t)1 << 22) || (K % 32) != 0) return INC_ERR_UNSUPPORTED;  // the route kernel's limits
  if ((reinterpret_cast<uintptr_t>(a) & 15) != 0 || (reinterpret_cast<uintptr_t>(H) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(rows) & 7) != 0 || (reinterpret_cast<uintptr_t>(route) & 3) != 0)
    return INC_ERR_UNSUPPORTED;
  const int nt = (int)ceil_div64(K, RB);
  const int64_t ntiles = (int64_t)nt * (nt + 1) / 2;
  if (ntiles > 0x7fffffff) return INC_ERR_UNSUPPORTED;
  hipStream_t s = inc_s(stream);
  const dim3 grid((unsigned)ntiles, (unsigned)E);
  const int S = (int)(T * top_k);
#define INC_ROUTED16(B, G) \
  hessian_routed_16bit_kernel<B, G><<<grid, 256, 0, s>>>((const uint16_t*)a, route, rows, H, T, top_k, (int)E, K, nt)
  if (xdtype == INC_F32) {
    if (mode == 0) hessian_routed_f32_kernel<true><<<grid, 256, 0, s>>>((const float*)a, route, rows, H, T, top_k, (int)E, K, nt);
    else hessian_routed_f32_kernel<false><<<grid, 256, 0, s>>>((const float*)a, route, rows, H, T, top_k, (int)E, K, nt);
  } else if (xdtype == INC_BF16) {
    if (mode == 0) INC_ROUTED16(true, true); else INC_ROUTED16(true, false);
  } else {
    if (mode == 0) INC_ROUTED16(false, true); else INC_ROUTED16(false, false);
  }
#undef INC_ROUTED16
  hessian_routed_rows_kernel<<<1, 512, 0, s>>>(route, rows, (int)E, S);
  INC_LAUNCH_RETURN();
}

}  // extern "C"
