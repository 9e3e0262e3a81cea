// gptq_mx.hip -- K6 on the MX grid: the 128-column error-compensation chain of GPTQ with the OCP microscaling quantiser of mx.hip
// (E8M0 block bytes, RNE onto e2m1 / e4m3) in place of the integer one, and the whole column loop around it as one call.
//
// The Hessian, the inverse-Cholesky factor and the trailing (lazy) update are the integer path's, unchanged (gptq_hessian.hip,
// chol.hip / ifac.hip, gptq_lazy.hip): only the chain differs.  What it emits is inc_mx_quant's storage -- packed codes [N, Kp] (e4m3)
// or [N, Kp/2] (e2m1, element 2i in the low nibble) and E8M0 bytes [N, Kp/32] -- so MXWeightOnlyLinear / MXLinear take the two
// buffers as they are.  The specification is the comment of inc_gptq_quantize_layer_mx in include/inc_mi355x.h.
#include <algorithm>
#include <type_traits>

#include "gptq_common.hpp"
#include "mx_format.hpp"

namespace {

constexpr int Q4R = 16;  // rows per wave
constexpr int Q4W = 4;   // waves per workgroup
// compile-time loop and quad broadcast of the integer chain (gptq.hip; copied, not shared, so that object stays what it is)
template <int I, int END, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < END) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, END>(f);
  }
}
__device__ __forceinline__ float quad_bcast(float v, int src) {
  const int x = __float_as_int(v);
  int y;
  switch (src) {  // the control word must be a literal; `src` is a constant after unrolling
    case 0: y = __builtin_amdgcn_mov_dpp(x, 0x00, 0xf, 0xf, true); break;
    case 1: y = __builtin_amdgcn_mov_dpp(x, 0x55, 0xf, 0xf, true); break;
    case 2: y = __builtin_amdgcn_mov_dpp(x, 0xAA, 0xf, 0xf, true); break;
    default: y = __builtin_amdgcn_mov_dpp(x, 0xFF, 0xf, 0xf, true); break;
  }
  return __int_as_float(y);
}

// |value| of a magnitude code (the inverse of mx_encode): field f = m >> MB, fraction t = m & (2^MB - 1); (2^MB + t) * 2^(f - 1 + EMINF - 127 - MB)
// for f >= 1, t * 2^(EMINF - 127 - MB) for the subnormal codes f == 0 -- an integer times a power of two, exact in fp32
template <int FMT>
__device__ __forceinline__ float mx_code_abs(uint32_t m) {
  using F = MxFmt<FMT>;
  const uint32_t f = m >> F::MB, t = m & ((1u << F::MB) - 1u);
  const uint32_t mant = f ? t + (1u << F::MB) : t;
  const uint32_t ex = (f ? f - 1u : 0u) + (uint32_t)(F::EMINF - F::MB);
  return (float)mant * __uint_as_float(ex << 23);
}

// ---------------------------------------------------------------------------------------------
// the serial column chain for one 128-column block, MX quantiser
// ---------------------------------------------------------------------------------------------
// The work split is gptq_quant_block_q4_kernel's: a wave owns 16 rows, the four lanes of a quad share a row with the block's columns
// interleaved (lane q owns 4c + q), four waves share ONE Hinv1 tile in LDS (64 KiB, LDS-DMA), the Hinv row of step i + 1 is read from
// LDS into the alternate register set while step i computes, the steps are unrolled at compile time, contraction is off.
// The quantiser and the outputs are its own:
//   scales   a 128-column block holds four MX blocks of 32 = 8 columns per lane: amax over the lane's 8, then over the quad (two
//            shuffles); byte = clamp(expfield(amax) - EMAX, 0, 254) on the columns AS THEY ARE WHEN THE 128-BLOCK STARTS (every earlier
//            block's update applied, none of this chain's) -- the rule of the integer path's PARAMS form, always in-kernel.
//   step     v = x * 2^(127 - byte); code = mx_encode(v, sign x); q = +-|code| * 2^(byte - 127); e = (x - q) / d; wr[c] -= e * h[c]
//            -- two exact multiplications by powers of two round the rounding, no division but the one by d.
//   tail     count in {32, 64, 96}: the TAIL form of the kernel skips the 32 steps of an MX block past `count` by ONE wave-uniform
//            branch; such columns are loaded as 0 and leave as Err = 0, code 0, byte 0.  It is a form of its own because the three
//            branches cost registers (379 instead of 132: the values of every section meet at the joins) -- the tail is the LAST block
//            of a layer, no trailing update runs beside it, and the full block keeps the straight-line chain.
//   outputs  Err1 [N,128] fp32, q_out [N,K], and inc_mx_quant's storage: the codes' row piece (128 bytes, or 64 with two codes per
//            byte -- a lane's quad neighbour holds the other nibble) and the four scale bytes as one dword.  All 128 columns of the
//            block are written to wq / ws, so the last block's launch writes the padding K .. Kp - 1 itself.
#pragma clang fp contract(off)
template <int FMT, int QDT, bool TAIL>
__global__ __launch_bounds__(64 * Q4W) void gptq_mx_chain_kernel(const float* __restrict__ w, const float* __restrict__ Hinv,
                                                                 uint8_t* __restrict__ wq, uint8_t* __restrict__ ws,
                                                                 void* __restrict__ q_out, float* __restrict__ err, int64_t N,
                                                                 int64_t K, int64_t Kp, int64_t i1, int count) {
  using F = MxFmt<FMT>;
  constexpr bool FP4 = FMT == INC_MX_FP4_E2M1;
  constexpr int CB = FP4 ? QB / 2 : QB;  // code bytes of a row of the block
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* hs = reinterpret_cast<float*>(smem_raw);  // [QB][QB] Hinv1 tile, later reused as the waves' output stages
  __builtin_amdgcn_s_setprio(3);                   // the serial path goes first beside the trailing update's MFMA waves (gptq.hip)
  const int lane = threadIdx.x & 63, r = lane >> 2, q = lane & 3;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t n0 = ((int64_t)blockIdx.x * Q4W + wave) * Q4R;
  const int64_t row = n0 + r, rowc = row < N ? row : N - 1;

  if constexpr (!TAIL) {
    // Hinv1 tile -> LDS by LDS-DMA: 64 instructions of 1 KiB (two 512-byte rows each) shared out over the waves, all in flight at once
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem_raw;
    const float* hb = Hinv + i1 * K + i1;
    const uint32_t v0 = (uint32_t)(((lane >> 5) * K + 4 * (lane & 31)) * 4);
    const uint32_t step = (uint32_t)(2 * K * 4);
#pragma unroll
    for (int jj = 0; jj < 16 / Q4W; ++jj) {
      const int j = jj * Q4W + wave;
      lds_dma_4x1k(hb, lds0 + j * 4096, v0 + (4 * j) * step, v0 + (4 * j + 1) * step, v0 + (4 * j + 2) * step, v0 + (4 * j + 3) * step);
    }
  } else {
    // the tail block: a 128 x 128 window at i1 leaves the matrix, so the tile is read element by element, identity outside count x count
    for (int idx = threadIdx.x; idx < QB * QB; idx += 64 * Q4W) {
      const int rr = idx >> 7, c = idx & 127;
      hs[idx] = (rr < count && c < count) ? Hinv[(i1 + rr) * K + i1 + c] : (rr == c ? 1.f : 0.f);
    }
  }
  // this lane's 32 columns of its row: block columns 4c + q
  float wr[32], ev[32];
  uint32_t cw[8];  // the codes of columns 4c + q, one byte each
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    if constexpr (TAIL) {
      const bool in = 4 * c + q < count;  // loaded without a branch
      const float v = w[rowc * K + i1 + (in ? 4 * c + q : 0)];
      wr[c] = in ? v : 0.f;
    } else {
      wr[c] = w[rowc * K + i1 + 4 * c + q];
    }
    ev[c] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) cw[c] = 0u;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // MX block g = block columns [32g, 32g + 32): this lane's c in [8g, 8g + 8)
  float mult[4], sc[4];  // 2^(127 - byte), 2^(byte - 127)
  uint32_t sbytes = 0u;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float amax = 0.f;
#pragma unroll
    for (int c = 8 * g; c < 8 * g + 8; ++c) amax = fmaxf(amax, fabsf(wr[c]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    int byte = (int)(__float_as_uint(amax) >> 23) - F::EMAX;  // at most 255 - 2
    byte = byte < 0 ? 0 : byte;
    mult[g] = __uint_as_float((uint32_t)(254 - byte) << 23);                    // a normal number for every byte <= 253
    sc[g] = __uint_as_float(byte ? (uint32_t)byte << 23 : 0x00400000u);         // 2^-127 is subnormal
    sbytes |= (uint32_t)byte << (8 * g);
  }
  __syncthreads();

  // The row of Hinv1 needed by step i+1 is read from LDS while step i computes: two register sets used alternately
  float ha[33], hb2[33];  // [c] = hs[i][4c+q] for the live c, [32] = hs[i][i]
  auto fetch_row = [&](auto ic, float (&h)[33]) {
    constexpr int i = decltype(ic)::value;
    if constexpr (i < QB) {
#pragma unroll
      for (int c = i >> 2; c < 32; ++c) h[c] = hs[i * QB + 4 * c + q];
      h[32] = hs[i * QB + i];
    }
  };
  auto step = [&](auto ic, float (&h)[33]) {
    constexpr int i = decltype(ic)::value;
    constexpr int qo = i & 3, ci = i >> 2, g = i / 32;
    const float x = quad_bcast(wr[ci], qo);
    const uint32_t sign = __float_as_uint(x) >> 31;
    const uint32_t code = mx_encode<FMT>(x * mult[g], sign);
    const float qa = mx_code_abs<FMT>(code & (FP4 ? 0x7u : 0x7fu)) * sc[g];
    const float qv = __uint_as_float(__float_as_uint(qa) | (sign << 31));
    const float e = (x - qv) / h[32];
    const bool own = q == qo;
#pragma unroll
    for (int c = ci; c < 32; ++c) {
      const float pr = e * h[c];  // exact zero below the diagonal (Hinv is upper triangular)
      wr[c] = wr[c] - pr;
    }
    wr[ci] = own ? qv : wr[ci];
    ev[ci] = own ? e : ev[ci];
    cw[ci >> 2] = own ? (cw[ci >> 2] | (code << (8 * (ci & 3)))) : cw[ci >> 2];
    // pinned here for the reason gptq.hip records: left alone, the selects sink to the end of the chain and every step's values stay live
    asm volatile("" : "+v"(wr[ci]), "+v"(ev[ci]), "+v"(cw[ci >> 2]));
    __builtin_amdgcn_sched_barrier(0);
  };
  fetch_row(std::integral_constant<int, 0>{}, ha);
  static_for<0, 4>([&](auto gc) {
    constexpr int g = decltype(gc)::value;
    if (!TAIL || 32 * g < count) {  // wave-uniform: whole MX blocks past `count` are skipped
      static_for<16 * g, 16 * g + 16>([&](auto pc) {
        constexpr int p = decltype(pc)::value;
        fetch_row(std::integral_constant<int, 2 * p + 1>{}, hb2);
        step(std::integral_constant<int, 2 * p>{}, ha);
        fetch_row(std::integral_constant<int, 2 * p + 2>{}, ha);
        step(std::integral_constant<int, 2 * p + 1>{}, hb2);
      });
    }
  });
  __syncthreads();
  // stage the outputs through LDS (rows of 128) for coalesced stores: Err1, then Q and the packed codes -- every wave in its own 10 KiB
  float* st = reinterpret_cast<float*>(smem_raw + wave * (Q4R * QB * 5));  // [Q4R][QB] floats, then [Q4R][CB] bytes
#pragma unroll
  for (int c = 0; c < 32; ++c) st[r * QB + 4 * c + q] = ev[c];
  __syncthreads();
  for (int idx = lane; idx < Q4R * QB / 4; idx += 64) {
    const int rr = idx >> 5, c4 = (idx & 31) * 4;
    if (n0 + rr < N) *reinterpret_cast<float4*>(err + (n0 + rr) * QB + c4) = *reinterpret_cast<const float4*>(st + rr * QB + c4);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 32; ++c) st[r * QB + 4 * c + q] = wr[c] + 0.f;  // a zero leaves as +0 whatever sign later steps' e * 0 gave it
  uint8_t* cst = reinterpret_cast<uint8_t*>(st + Q4R * QB);
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const uint32_t mine = (cw[c >> 2] >> (8 * (c & 3))) & 0xffu;
    if constexpr (FP4) {
      // columns 4c + q and 4c + (q ^ 1) share byte 2c + (q >> 1): the even lane stores both nibbles
      const uint32_t other = (uint32_t)__shfl_xor((int)mine, 1, 64);
      if ((q & 1) == 0) cst[r * CB + 2 * c + (q >> 1)] = (uint8_t)(mine | (other << 4));
    } else {
      cst[r * CB + 4 * c + q] = (uint8_t)mine;
    }
  }
  __syncthreads();
  for (int idx = lane; idx < Q4R * QB; idx += 64) {
    const int rr = idx >> 7, c = idx & 127;
    if (n0 + rr < N && c < count) store_from_f32<QDT>(q_out, (n0 + rr) * K + i1 + c, st[rr * QB + c]);
  }
  const int64_t crow = FP4 ? Kp / 2 : Kp, coff = FP4 ? i1 / 2 : i1;  // bytes per row of wq, the block's first byte in it
  for (int idx = lane; idx < Q4R * CB / 16; idx += 64) {
    const int rr = idx / (CB / 16), c16 = (idx % (CB / 16)) * 16;
    if (n0 + rr < N) *reinterpret_cast<uint4*>(wq + (n0 + rr) * crow + coff + c16) = *reinterpret_cast<const uint4*>(cst + rr * CB + c16);
  }
  if (q == 0 && row < N) *reinterpret_cast<uint32_t*>(ws + row * (Kp / 32) + i1 / 32) = sbytes;
}

#pragma clang fp contract(fast)

template <int FMT>
int launch_mx_chain(const float* w, const float* Hinv, uint8_t* wq, uint8_t* ws, void* q_out, int q_dtype, float* err, int64_t N, int64_t K,
                    int64_t Kp, int64_t i1, int count, hipStream_t s) {
  const size_t smem = (size_t)QB * QB * 4;  // 64 KiB: Hinv1 tile, reused as the output stage
  static std::atomic<uint64_t> attr_set{0};
  if (inc_attr_needed(attr_set)) {
    auto lds = [&](auto... kernel) { ((void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), ...); };
    lds(gptq_mx_chain_kernel<FMT, INC_F32, false>, gptq_mx_chain_kernel<FMT, INC_F16, false>, gptq_mx_chain_kernel<FMT, INC_BF16, false>);
    lds(gptq_mx_chain_kernel<FMT, INC_F32, true>, gptq_mx_chain_kernel<FMT, INC_F16, true>, gptq_mx_chain_kernel<FMT, INC_BF16, true>);
    inc_attr_done(attr_set);
  }
  const unsigned blocks = (unsigned)ceil_div64(N, Q4R * Q4W);
  INC_DISPATCH_DTYPE(q_dtype, DT, {
    if (count == QB) gptq_mx_chain_kernel<FMT, DT, false><<<blocks, 64 * Q4W, smem, s>>>(w, Hinv, wq, ws, q_out, err, N, K, Kp, i1, count);
    else gptq_mx_chain_kernel<FMT, DT, true><<<blocks, 64 * Q4W, smem, s>>>(w, Hinv, wq, ws, q_out, err, N, K, Kp, i1, count);
  })
  INC_LAUNCH_RETURN();
}

// what both entry points require of a layer; INC_OK when the chain takes it
int mx_layer_check(const void* w, const void* Hinv, const void* wq, const void* ws, const void* q_out, const void* err, int q_dtype, int64_t N,
                   int64_t K, int64_t Kp, int fmt) {
  INC_CHECK_ARG(w && Hinv && wq && ws && q_out && err && N > 0 && K > 0 && Kp > 0);
  if (fmt != INC_MX_FP8_E4M3 && fmt != INC_MX_FP4_E2M1) return INC_ERR_UNSUPPORTED;
  if (q_dtype != INC_F32 && q_dtype != INC_F16 && q_dtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  if ((K % 32) != 0 || Kp != ceil_div64(K, QB) * QB) return INC_ERR_UNSUPPORTED;
  if (K * (int64_t)(QB + 1) * 4 >= ((int64_t)1 << 32)) return INC_ERR_UNSUPPORTED;  // 32-bit byte offsets into Hinv rows (block_range_ok)
  INC_CHECK_ARG((reinterpret_cast<uintptr_t>(wq) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0);
  return INC_OK;
}

}  // namespace

extern "C" {

int inc_gptq_quant_block_mx(const float* w, const float* Hinv, uint8_t* wq, uint8_t* ws, void* q_out, int q_dtype, float* err, int64_t N,
                            int64_t K, int64_t Kp, int64_t i1, int fmt, inc_stream_t stream) {
  const int rc = mx_layer_check(w, Hinv, wq, ws, q_out, err, q_dtype, N, K, Kp, fmt);
  if (rc != INC_OK) return rc;
  INC_CHECK_ARG(i1 >= 0 && i1 < K && (i1 % QB) == 0);
  const int count = (int)std::min<int64_t>(QB, K - i1);
  if (fmt == INC_MX_FP8_E4M3) return launch_mx_chain<INC_MX_FP8_E4M3>(w, Hinv, wq, ws, q_out, q_dtype, err, N, K, Kp, i1, count, inc_s(stream));
  return launch_mx_chain<INC_MX_FP4_E2M1>(w, Hinv, wq, ws, q_out, q_dtype, err, N, K, Kp, i1, count, inc_s(stream));
}

// The orchestration of inc_gptq_quantize_layer (gptq.hip) around the MX chain: per 128 columns the chain, then the next block's 128
// columns of the trailing update on `stream` and the rest on `aux_stream` underneath the next chain.  rest(b-1) is awaited before
// next(b), so every column receives its updates in block order from the same 128-column tiles: bit-identical to the one-stream loop.
int inc_gptq_quantize_layer_mx(float* w, const float* Hinv, uint8_t* wq, uint8_t* ws, void* q_out, int q_dtype, float* err_ws, int64_t N,
                               int64_t K, int64_t Kp, int fmt, int flags, inc_stream_t stream, inc_stream_t aux_stream) {
  const int ok = mx_layer_check(w, Hinv, wq, ws, q_out, err_ws, q_dtype, N, K, Kp, fmt);
  if (ok != INC_OK) return ok;
  hipStream_t main = inc_s(stream), side = inc_s(aux_stream);
  const bool lookahead = aux_stream != nullptr && (flags & INC_GPTQ_NO_LOOKAHEAD) == 0 && K % QB == 0 && K >= 3 * QB;
  float* errs[2] = {err_ws, err_ws + N * QB};
  hipEvent_t ready = nullptr, rest_done = nullptr;
  bool rest_pending = false;
  int rc = INC_OK;
#define INC_TRY(call)                         \
  {                                           \
    const int r_ = (call);                    \
    if (r_ != INC_OK) { rc = r_; goto done; } \
  }
  if (lookahead) {
    if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&rest_done, hipEventDisableTiming) != hipSuccess) {
      rc = INC_ERR_LAUNCH;
      goto done;
    }
    (void)hipEventRecord(ready, main);  // w / Hinv were produced on the main stream
    (void)hipStreamWaitEvent(side, ready, 0);
  }
  {
    int blk = 0;
    for (int64_t i1 = 0; i1 < K; i1 += QB, ++blk) {
      const int count = (int)std::min<int64_t>(QB, K - i1);
      const int64_t i2 = i1 + count;
      float* e = errs[lookahead ? (blk & 1) : 0];
      INC_TRY(inc_gptq_quant_block_mx(w, Hinv, wq, ws, q_out, q_dtype, e, N, K, Kp, i1, fmt, stream))
      if (!lookahead) {
        INC_TRY(inc_gptq_lazy_update(w, Hinv, e, N, K, i1, count, stream))
      } else if (i2 < K) {
        const int64_t nxt_end = std::min<int64_t>(i2 + QB, K);
        if (nxt_end < K) (void)hipEventRecord(ready, main);               // Err1 of this block is complete: rest(b) may start
        if (rest_pending) (void)hipStreamWaitEvent(main, rest_done, 0);  // rest(b-1) wrote the columns next(b) updates
        INC_TRY(inc_gptq_lazy_update_cols(w, Hinv, e, N, K, i1, count, i2, nxt_end, stream))
        if (nxt_end < K) {
          (void)hipStreamWaitEvent(side, ready, 0);
          INC_TRY(inc_gptq_lazy_update_cols(w, Hinv, e, N, K, i1, count, nxt_end, K, aux_stream))
          (void)hipEventRecord(rest_done, side);
          rest_pending = true;
        }
      }
    }
  }
  if (lookahead && rest_pending) (void)hipStreamWaitEvent(main, rest_done, 0);  // w and both Err buffers are free again
done:
#undef INC_TRY
  if (ready) (void)hipEventDestroy(ready);
  if (rest_done) (void)hipEventDestroy(rest_done);
  return rc;
}

}  // extern "C"
