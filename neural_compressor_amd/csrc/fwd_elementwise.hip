// fwd_elementwise.hip -- the three elementwise chains of a Llama block forward as one streaming kernel each, BIT-IDENTICAL to what
// eager PyTorch-ROCm computes for them (torch/algorithms/weight_only/fused_forward.py substitutes them inside the block forwards the
// GPTQ driver issues and checks the identity on the run's own tensors):
//   inc_fwd_silu_mul  act_fn(gate) * up                 2 torch kernels, one 11008-wide intermediate
//   inc_fwd_rope      apply_rotary_pos_emb(q, k, ..)    14 torch kernels (7 per tensor)
//   inc_fwd_rmsnorm   LlamaRMSNorm.forward              6 torch kernels, two of them over an fp32 copy
// Every kernel: 16 bytes per lane and access, one pass, one workgroup per chunk, non-temporal hints on the bulk tensors (the recipe
// that won the copy probe, probe.hip: tensors of a calibration forward are GBs, nothing read here is in a cache when it is needed again).
// Every rounding is the one eager makes: each torch kernel rounds its fp32 result to the tensor dtype, so the chains below round at
// the same places, and `#pragma clang fp contract(off)` keeps the compiler from fusing a multiply into a following add where eager
// has two kernels (mean * factor, then + eps).
#include "common.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// fp32 -> 16-bit as torch's c10 types convert on ROCm: BFloat16 in software (round to nearest even, EVERY NaN becomes 0x7FC0),
// Half with the hardware conversion
template <int DT>
__device__ __forceinline__ uint16_t t_round(float f) {
  if constexpr (DT == INC_BF16) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7FC0;
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
  } else {
    return f32_to_f16_bits(f);
  }
}
template <int DT>
__device__ __forceinline__ float t_f32(uint16_t b) {
  if constexpr (DT == INC_BF16) return bf16_bits_to_f32(b);
  else return f16_bits_to_f32(b);
}
template <int DT>
__device__ __forceinline__ float t_rf(float f) { return t_f32<DT>(t_round<DT>(f)); }  // round to DT, back in fp32

// The same roundings, eight values (one 16-byte piece) at a time.  bf16 goes through the hardware conversion, two values per
// v_cvt_pk_bf16_f32 (round to nearest even, denormals kept) instead of ~6 integer instructions per value; what the hardware does NOT do
// is torch's NaN rule (it keeps a NaN's sign and payload bits), so a piece that holds a NaN -- one unordered compare per pair tells --
// is redone with t_round.  fp16 is the hardware conversion either way.
template <int DT>
__device__ __forceinline__ u32x4 round8(const float (&f)[8]) {
  u32x4 v;
  if constexpr (DT == INC_BF16) {
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = cvt_pair<true>(f[2 * i], f[2 * i + 1]);
      nan |= __builtin_isunordered(f[2 * i], f[2 * i + 1]);
    }
    if (__builtin_expect(nan, 0)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = static_cast<uint32_t>(t_round<DT>(f[2 * i])) | (static_cast<uint32_t>(t_round<DT>(f[2 * i + 1])) << 16);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = static_cast<uint32_t>(t_round<DT>(f[2 * i])) | (static_cast<uint32_t>(t_round<DT>(f[2 * i + 1])) << 16);
  }
  return v;
}
// round to DT and back to fp32, in place: an INTERMEDIATE of a chain.  A NaN stays a NaN here (every value that gets here is the result
// of an fp32 operation, so its NaN is quiet and the quiet bit survives the conversion) and its payload never reaches memory: whatever
// is computed from it is a NaN again, and the chain's last rounding (round8) writes torch's 0x7FC0 for it.
template <int DT>
__device__ __forceinline__ void rf8(float (&f)[8]) {
  if constexpr (DT == INC_BF16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t r = cvt_pair<true>(f[2 * i], f[2 * i + 1]);
      f[2 * i] = __uint_as_float(r << 16);
      f[2 * i + 1] = __uint_as_float(r & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = t_rf<DT>(f[i]);
  }
}

template <int DT>
__device__ __forceinline__ void unpack8(const u32x4 v, float (&e)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[2 * i] = t_f32<DT>(static_cast<uint16_t>(v[i] & 0xffffu));
    e[2 * i + 1] = t_f32<DT>(static_cast<uint16_t>(v[i] >> 16));
  }
}
__device__ __forceinline__ u32x4 ld_nt(const void* p, int64_t i16) { return __builtin_nontemporal_load(static_cast<const u32x4*>(p) + i16); }
__device__ __forceinline__ void st_nt(void* p, int64_t i16, u32x4 v) { __builtin_nontemporal_store(v, static_cast<u32x4*>(p) + i16); }

// ---- SiLU * up ------------------------------------------------------------------------------------------------------------------
// torch: silu kernel  s = DT(g / (1 + exp(-g))) in fp32 (ActivationSiluKernel.cu), then mul kernel  out = DT(float(s) * float(u))
template <int DT>
__device__ __forceinline__ uint16_t silu_mul_one(float g, float u) {
#pragma clang fp contract(off)
  const float s = t_rf<DT>(g / (1.0f + expf(-g)));
  return t_round<DT>(s * u);
}

template <int DT>
__global__ __launch_bounds__(256) void fwd_silu_mul_kernel(const void* __restrict__ gate, const void* __restrict__ up, void* __restrict__ out, int64_t n) {
  const int64_t n8 = n >> 3;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n8) {
#pragma clang fp contract(off)
    float g[8], u[8];
    unpack8<DT>(ld_nt(gate, i), g);
    unpack8<DT>(ld_nt(up, i), u);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = g[e] / (1.0f + expf(-g[e]));
    rf8<DT>(g);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = g[e] * u[e];
    st_nt(out, i, round8<DT>(g));
  } else {
    const int64_t e = n8 * 8 + (i - n8);  // the n % 8 tail, one element per lane
    if (e < n) {
      const uint16_t* g = static_cast<const uint16_t*>(gate);
      const uint16_t* u = static_cast<const uint16_t*>(up);
      static_cast<uint16_t*>(out)[e] = silu_mul_one<DT>(t_f32<DT>(g[e]), t_f32<DT>(u[e]));
    }
  }
}

// ---- rotary embedding of q and k ------------------------------------------------------------------------------------------------
// torch (per tensor x of [B, H, T, D], cos / sin [Bc, 1, T, D]):  x * cos,  -x2,  cat(-x2, x1),  rot * sin,  add -- each kernel
// rounds to DT.  x * cos and rot * sin are exact in fp32 before that rounding (two 8- or 11-bit significands), -x2 is exact.
struct RopeStrides {
  int64_t q[3], k[3], qo[3], ko[3];  // element strides of the b, h, t dimensions; the d stride is 1
};

// one head of one token: the 16-byte pieces at d and d + D/2 and the four cos / sin pieces (unpacked) that go with them.
// `sign2` is 0x80008000, handed in as a kernel ARGUMENT: eager negates x2 in a kernel of its own, so a NaN there has its sign flipped
// before the multiply, and an fp16 result carries that sign to memory.  A negation the compiler can see is one it may move -- to sin, or
// to the product (it did both: `v_pk_mul_f32 .. neg_lo:[0,1]`, `v_sub_f16`) -- which is the same number for everything but a NaN.  An
// exclusive-or of the 16-bit patterns with a value it does not know stays where eager has it.  (bf16 writes 0x7FC0 for every NaN: no need.)
template <int DT>
__device__ __forceinline__ void rope_pieces(const u32x4 v_lo, const u32x4 v_hi, const float (&c_lo)[8], const float (&c_hi)[8],
                                            const float (&s_lo)[8], const float (&s_hi)[8], const uint32_t sign2, u32x4& o_lo, u32x4& o_hi) {
#pragma clang fp contract(off)
  float lo[8], hi[8], a[8], b[8];
  unpack8<DT>(v_lo, lo);
  unpack8<DT>(v_hi, hi);
  if constexpr (DT == INC_BF16) {
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = -hi[e];
  } else {
    u32x4 n_hi;
#pragma unroll
    for (int i = 0; i < 4; ++i) n_hi[i] = v_hi[i] ^ sign2;
    unpack8<DT>(n_hi, b);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    a[e] = lo[e] * c_lo[e];
    b[e] = b[e] * s_lo[e];
  }
  rf8<DT>(a);
  rf8<DT>(b);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = a[e] + b[e];
  o_lo = round8<DT>(a);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    a[e] = hi[e] * c_hi[e];
    b[e] = lo[e] * s_hi[e];
  }
  rf8<DT>(a);
  rf8<DT>(b);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = a[e] + b[e];
  o_hi = round8<DT>(a);
}

// The walker: one WAVE per token (b, t).  A lane owns one 16-byte piece of d (with its partner at d + D/2): it decodes its offsets once,
// loads its four cos / sin pieces once and keeps them unpacked in registers, then walks the heads -- the q heads, then the k heads, each
// tensor with its own strides.  D / 16 lanes cover a head, so the wave takes HPI = 64 / (D / 16) consecutive heads per iteration (8 for
// D = 128: 2 KiB contiguous in the model's [B, T, H * D] layout) and strides by HPI heads; U iterations' loads are issued before the
// first of them is used (2 U loads of 16 bytes in flight per lane).  D / 16 must be a power of two up to 64.
constexpr int ROPE_WALK_U = 4;
constexpr uint32_t ROPE_SIGN2 = 0x80008000u;  // the sign bits of two 16-bit values (see rope_pieces)

template <int DT>
__device__ __forceinline__ void rope_walk(const char* __restrict__ src, char* __restrict__ dst, const int64_t in_base, const int64_t out_base,
                                          const int64_t in_hs, const int64_t out_hs, const uint32_t H, const uint32_t hsub, const uint32_t hpi,
                                          const int64_t half, const float (&c_lo)[8], const float (&c_hi)[8], const float (&s_lo)[8],
                                          const float (&s_hi)[8], const uint32_t sign2) {
  for (uint32_t h0 = 0; h0 < H; h0 += hpi * ROPE_WALK_U) {  // (uniform over the wave)
    u32x4 v_lo[ROPE_WALK_U], v_hi[ROPE_WALK_U];
#pragma unroll
    for (int u = 0; u < ROPE_WALK_U; ++u) {
      const uint32_t h = h0 + u * hpi + hsub;
      if (h < H) {
        const int64_t off = in_base + (int64_t)h * in_hs;  // elements; a multiple of 8
        v_lo[u] = ld_nt(src, off >> 3);
        v_hi[u] = ld_nt(src, (off + half) >> 3);
      }
    }
#pragma unroll
    for (int u = 0; u < ROPE_WALK_U; ++u) {
      const uint32_t h = h0 + u * hpi + hsub;
      if (h < H) {
        u32x4 o_lo, o_hi;
        rope_pieces<DT>(v_lo[u], v_hi[u], c_lo, c_hi, s_lo, s_hi, sign2, o_lo, o_hi);
        const int64_t off = out_base + (int64_t)h * out_hs;
        st_nt(dst, off >> 3, o_lo);
        st_nt(dst, (off + half) >> 3, o_hi);
      }
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void fwd_rope_walk_kernel(const void* __restrict__ q, const void* __restrict__ k, const void* __restrict__ cosp,
                                                            const void* __restrict__ sinp, void* __restrict__ q_out, void* __restrict__ k_out,
                                                            uint32_t tokens, uint32_t Hq, uint32_t Hk, uint32_t T, uint32_t D, uint32_t d16_log2,
                                                            uint32_t cs_batch, uint32_t sign2, RopeStrides st) {
  const uint32_t token = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));  // the same for the whole wave
  if (token >= tokens) return;
  const uint32_t b = token / T, t = token - b * T;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t dc = lane & ((1u << d16_log2) - 1u), hsub = lane >> d16_log2, hpi = 64u >> d16_log2;
  const int64_t half = D >> 1;
  const int64_t cs_off = ((int64_t)(cs_batch == 1 ? 0 : b) * T + t) * D + dc * 8;

  float c_lo[8], c_hi[8], s_lo[8], s_hi[8];
  unpack8<DT>(static_cast<const u32x4*>(cosp)[cs_off >> 3], c_lo);
  unpack8<DT>(static_cast<const u32x4*>(cosp)[(cs_off + half) >> 3], c_hi);
  unpack8<DT>(static_cast<const u32x4*>(sinp)[cs_off >> 3], s_lo);
  unpack8<DT>(static_cast<const u32x4*>(sinp)[(cs_off + half) >> 3], s_hi);

  rope_walk<DT>(static_cast<const char*>(q), static_cast<char*>(q_out), (int64_t)b * st.q[0] + (int64_t)t * st.q[2] + dc * 8,
                (int64_t)b * st.qo[0] + (int64_t)t * st.qo[2] + dc * 8, st.q[1], st.qo[1], Hq, hsub, hpi, half, c_lo, c_hi, s_lo, s_hi, sign2);
  rope_walk<DT>(static_cast<const char*>(k), static_cast<char*>(k_out), (int64_t)b * st.k[0] + (int64_t)t * st.k[2] + dc * 8,
                (int64_t)b * st.ko[0] + (int64_t)t * st.ko[2] + dc * 8, st.k[1], st.ko[1], Hk, hsub, hpi, half, c_lo, c_hi, s_lo, s_hi, sign2);
}

// the item-per-lane form: every (b, t, head, piece) is a lane of its own.  Kept for head sizes the walker does not take (D / 16 no power
// of two, or above 64)
template <int DT>
__global__ __launch_bounds__(256) void fwd_rope_kernel(const void* __restrict__ q, const void* __restrict__ k, const void* __restrict__ cosp,
                                                       const void* __restrict__ sinp, void* __restrict__ q_out, void* __restrict__ k_out,
                                                       uint32_t total, uint32_t Hq, uint32_t Hk, uint32_t T, uint32_t D, uint32_t cs_batch,
                                                       uint32_t sign2, RopeStrides st) {
#pragma clang fp contract(off)
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= total) return;
  // memory order of the model's layout ([B, T, H * D] projections): d fastest, then head (q heads, then k heads), then t, then b
  const uint32_t d16 = D >> 4, H = Hq + Hk;
  const uint32_t dc = idx % d16;
  uint32_t r = idx / d16;
  const uint32_t hh = r % H;
  r /= H;
  const uint32_t t = r % T, b = r / T;
  const bool is_k = hh >= Hq;
  const uint32_t h = is_k ? hh - Hq : hh;
  const int64_t* si = is_k ? st.k : st.q;
  const int64_t* so = is_k ? st.ko : st.qo;
  const char* src = static_cast<const char*>(is_k ? k : q);
  char* dst = static_cast<char*>(is_k ? k_out : q_out);
  const int64_t in_off = (int64_t)b * si[0] + (int64_t)h * si[1] + (int64_t)t * si[2] + dc * 8;   // elements; multiples of 8
  const int64_t out_off = (int64_t)b * so[0] + (int64_t)h * so[1] + (int64_t)t * so[2] + dc * 8;
  const int64_t cs_off = ((int64_t)(cs_batch == 1 ? 0 : b) * T + t) * D + dc * 8;
  const int64_t half = D >> 1;

  float c_lo[8], c_hi[8], s_lo[8], s_hi[8];
  const u32x4 v_lo = ld_nt(src, in_off >> 3), v_hi = ld_nt(src, (in_off + half) >> 3);
  unpack8<DT>(static_cast<const u32x4*>(cosp)[cs_off >> 3], c_lo);
  unpack8<DT>(static_cast<const u32x4*>(cosp)[(cs_off + half) >> 3], c_hi);
  unpack8<DT>(static_cast<const u32x4*>(sinp)[cs_off >> 3], s_lo);
  unpack8<DT>(static_cast<const u32x4*>(sinp)[(cs_off + half) >> 3], s_hi);
  u32x4 o_lo, o_hi;
  rope_pieces<DT>(v_lo, v_hi, c_lo, c_hi, s_lo, s_hi, sign2, o_lo, o_hi);
  st_nt(dst, out_off >> 3, o_lo);
  st_nt(dst, (out_off + half) >> 3, o_hi);
}

// ---- RMSNorm --------------------------------------------------------------------------------------------------------------------
// torch: x32 = float(x); x32.pow(2); .mean(-1) ; + eps ; rsqrt (in double, see below) ; x32 * that ; .to(DT) ; weight * that.  Everything but the mean is
// elementwise; the mean's summation order is the one of at::native::reduce_kernel (ATen/native/cuda/Reduce.cuh) for an fp32
// [rows, cols] input reduced over its contiguous dimension with vt0 = 4, input_vec_size = 4, 512 threads and wave64, rows >= 8:
//   * 256 <= cols <= 8128 (WAVES = 1): block (64, 8), one wave per row.  Lane L adds the float4 vectors L, L + 64, L + 128, .. of the
//     row into four accumulators (one per vector component, starting from 0), then ((a0 + a1) + a2) + a3, then the wave adds lane
//     L + o to lane L for o = 1, 2, 4, .. 32 (the ROCm order of block_x_reduce), lane 0 holds the sum.
//   * 8129 <= cols < 131072 (WAVES = 8): block (64, 8), eight waves per row.  Lane L of wave w adds the vectors L + 64 w + 512 j; the
//     waves reduce as above and their eight sums s_w combine through shared memory as ((s0+s4) + (s2+s6)) + ((s1+s5) + (s3+s7)).
//   then MeanOps' projection: sum * factor with factor = float(rows) / float(rows * cols).
// Here HALF a wave plays one torch wave: lane p of it holds the vectors of torch lanes 2p and 2p + 1 (16 bytes of the 16-bit row), so
// the first step of torch's wave reduction (offset 1) is an add inside the lane and offsets 2 .. 32 are shuffles by 1 .. 16.  The row
// stays in registers (J 16-byte pieces per lane) between the sum and the scaling.
template <int DT, int WAVES, int J>
__global__ __launch_bounds__(WAVES == 1 ? 256 : 512) void fwd_rmsnorm_kernel(const void* __restrict__ x, const void* __restrict__ w, void* __restrict__ out,
                                                                              int64_t rows, int cols, float eps, float factor) {
#pragma clang fp contract(off)
  constexpr int HALVES = (WAVES == 1 ? 256 : 512) / 32, ROWS_PER_BLOCK = HALVES / WAVES;
  __shared__ float part[ROWS_PER_BLOCK][8];
  const int p = threadIdx.x & 31, hw = threadIdx.x >> 5;
  const int rb = hw / WAVES, tw = hw % WAVES;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + rb;
  const bool live = row < rows;
  const int pieces = cols >> 3;                       // 16-byte pieces of a row
  const int64_t base = (live ? row : 0) * (int64_t)pieces;
  const int first = p + 32 * tw;

  u32x4 v[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int u = first + 32 * WAVES * j;
    if (live && u < pieces) v[j] = ld_nt(x, base + u);
  }
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int u = first + 32 * WAVES * j;
    if (live && u < pieces) {
      float e[8];
      unpack8<DT>(v[j], e);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = a[i] + e[i] * e[i];          // e * e is exact in fp32 (or overflows to inf in every order)
        b[i] = b[i] + e[4 + i] * e[4 + i];
      }
    }
  }
  float s = (((a[0] + a[1]) + a[2]) + a[3]) + (((b[0] + b[1]) + b[2]) + b[3]);  // torch lanes 2p and 2p + 1, then offset 1
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) s = s + __shfl_down(s, o, 32);               // torch offsets 2 .. 32
  if constexpr (WAVES == 1) {
    s = __shfl(s, 0, 32);
  } else {
    if (p == 0) part[rb][tw] = s;
    __syncthreads();
    const float* q = part[rb];
    s = ((q[0] + q[4]) + (q[2] + q[6])) + ((q[1] + q[5]) + (q[3] + q[7]));
  }
  if (!live) return;
  const float mean = s * factor;
  // torch's rsqrt kernel calls ::rsqrt(a) on a float, and HIP declares rsqrt for double only (the float one is rsqrtf): the value goes
  // through the DOUBLE routine and is rounded back, which is not always what the 1-ulp v_rsq_f32 gives
  const float rs = static_cast<float>(::rsqrt(static_cast<double>(mean + eps)));
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int u = first + 32 * WAVES * j;
    if (u < pieces) {
      float e[8], g[8];
      unpack8<DT>(v[j], e);
      unpack8<DT>(static_cast<const u32x4*>(w)[u], g);
#pragma unroll
      for (int i = 0; i < 8; ++i) e[i] = e[i] * rs;
      rf8<DT>(e);
#pragma unroll
      for (int i = 0; i < 8; ++i) e[i] = g[i] * e[i];
      st_nt(out, base + u, round8<DT>(e));
    }
  }
}

template <int DT, int WAVES, int J>
void rmsnorm_launch(const void* x, const void* w, void* out, int64_t rows, int cols, float eps, float factor, hipStream_t s) {
  constexpr int THREADS = WAVES == 1 ? 256 : 512, ROWS_PER_BLOCK = THREADS / 32 / WAVES;
  fwd_rmsnorm_kernel<DT, WAVES, J><<<(unsigned)ceil_div64(rows, ROWS_PER_BLOCK), THREADS, 0, s>>>(x, w, out, rows, cols, eps, factor);
}

// ---- the rounding helper on its own (inc_probe_round16): out[i] = DT(in[i]) through round8, the n % 8 tail through t_round -----------
template <int DT>
__global__ __launch_bounds__(256) void probe_round16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int64_t n) {
  const int64_t n8 = n >> 3;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n8) {
    const u32x4 a = static_cast<const u32x4*>(static_cast<const void*>(in))[2 * i], b = static_cast<const u32x4*>(static_cast<const void*>(in))[2 * i + 1];
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[e] = __uint_as_float(a[e]);
      f[4 + e] = __uint_as_float(b[e]);
    }
    static_cast<u32x4*>(static_cast<void*>(out))[i] = round8<DT>(f);
  } else {
    const int64_t e = n8 * 8 + (i - n8);
    if (e < n) out[e] = t_round<DT>(in[e]);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int inc_fwd_silu_mul(const void* gate, const void* up, void* out, int64_t n, int dtype, inc_stream_t stream) {
  INC_CHECK_ARG(gate && up && out && n > 0);
  if (dtype != INC_BF16 && dtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if (!aligned16(gate) || !aligned16(up) || !aligned16(out)) return INC_ERR_UNSUPPORTED;
  const int64_t blocks = ceil_div64((n >> 3) + (n & 7), 256);
  if (blocks > 0x7fffffff) return INC_ERR_UNSUPPORTED;
  if (dtype == INC_BF16) fwd_silu_mul_kernel<INC_BF16><<<(unsigned)blocks, 256, 0, inc_s(stream)>>>(gate, up, out, n);
  else fwd_silu_mul_kernel<INC_F16><<<(unsigned)blocks, 256, 0, inc_s(stream)>>>(gate, up, out, n);
  INC_LAUNCH_RETURN();
}

int inc_fwd_rope(const void* q, const void* k, const void* cos, const void* sin, void* q_out, void* k_out, int64_t B, int64_t Hq,
                 int64_t Hk, int64_t T, int64_t D, const int64_t* strides, int64_t cs_batch, int dtype, inc_stream_t stream) {
  INC_CHECK_ARG(q && k && cos && sin && q_out && k_out && strides && B > 0 && Hq > 0 && Hk > 0 && T > 0 && D > 0);
  INC_CHECK_ARG(cs_batch == 1 || cs_batch == B);
  if (dtype != INC_BF16 && dtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if (D % 16 != 0) return INC_ERR_UNSUPPORTED;
  RopeStrides st;
  for (int i = 0; i < 3; ++i) {
    st.q[i] = strides[i];
    st.k[i] = strides[3 + i];
    st.qo[i] = strides[6 + i];
    st.ko[i] = strides[9 + i];
  }
  for (int i = 0; i < 12; ++i)
    if (strides[i] < 0 || strides[i] % 8 != 0) return INC_ERR_UNSUPPORTED;  // every 16-byte piece stays aligned
  if (!aligned16(q) || !aligned16(k) || !aligned16(cos) || !aligned16(sin) || !aligned16(q_out) || !aligned16(k_out)) return INC_ERR_UNSUPPORTED;
  if (B >= (1ll << 31) || T >= (1ll << 31) || Hq + Hk >= (1ll << 31)) return INC_ERR_UNSUPPORTED;
  const double items = (double)B * (double)T * (double)(Hq + Hk) * (double)(D / 16);
  if (items >= 2147483648.0 - 256.0) return INC_ERR_UNSUPPORTED;  // the kernel decodes a 32-bit item index
  const uint32_t d16 = (uint32_t)(D / 16);
  if ((d16 & (d16 - 1u)) == 0 && d16 <= 64u) {  // the walker: one wave per token (B * T < 2^31 by the item count above)
    const uint32_t tokens = (uint32_t)(B * T), lg = (uint32_t)__builtin_ctz(d16);
    const unsigned wblocks = (tokens + 3u) / 4u;
    if (dtype == INC_BF16)
      fwd_rope_walk_kernel<INC_BF16><<<wblocks, 256, 0, inc_s(stream)>>>(q, k, cos, sin, q_out, k_out, tokens, (uint32_t)Hq, (uint32_t)Hk, (uint32_t)T, (uint32_t)D, lg, (uint32_t)cs_batch, ROPE_SIGN2, st);
    else
      fwd_rope_walk_kernel<INC_F16><<<wblocks, 256, 0, inc_s(stream)>>>(q, k, cos, sin, q_out, k_out, tokens, (uint32_t)Hq, (uint32_t)Hk, (uint32_t)T, (uint32_t)D, lg, (uint32_t)cs_batch, ROPE_SIGN2, st);
    INC_LAUNCH_RETURN();
  }
  const uint32_t total = (uint32_t)(B * T * (Hq + Hk) * (D / 16));
  const unsigned blocks = (total + 255u) / 256u;
  if (dtype == INC_BF16)
    fwd_rope_kernel<INC_BF16><<<blocks, 256, 0, inc_s(stream)>>>(q, k, cos, sin, q_out, k_out, total, (uint32_t)Hq, (uint32_t)Hk, (uint32_t)T, (uint32_t)D, (uint32_t)cs_batch, ROPE_SIGN2, st);
  else
    fwd_rope_kernel<INC_F16><<<blocks, 256, 0, inc_s(stream)>>>(q, k, cos, sin, q_out, k_out, total, (uint32_t)Hq, (uint32_t)Hk, (uint32_t)T, (uint32_t)D, (uint32_t)cs_batch, ROPE_SIGN2, st);
  INC_LAUNCH_RETURN();
}

int inc_probe_round16(const float* in, uint16_t* out, int64_t n, int dtype, inc_stream_t stream) {
  INC_CHECK_ARG(in && out && n > 0);
  if (dtype != INC_BF16 && dtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if (!aligned16(in) || !aligned16(out)) return INC_ERR_UNSUPPORTED;
  const int64_t blocks = ceil_div64((n >> 3) + (n & 7), 256);
  if (blocks > 0x7fffffff) return INC_ERR_UNSUPPORTED;
  if (dtype == INC_BF16) probe_round16_kernel<INC_BF16><<<(unsigned)blocks, 256, 0, inc_s(stream)>>>(in, out, n);
  else probe_round16_kernel<INC_F16><<<(unsigned)blocks, 256, 0, inc_s(stream)>>>(in, out, n);
  INC_LAUNCH_RETURN();
}

int inc_fwd_rmsnorm(const void* x, const void* w, void* out, int64_t rows, int64_t cols, float eps, int dtype, inc_stream_t stream) {
  INC_CHECK_ARG(x && w && out && rows > 0 && cols > 0);
  if (dtype != INC_BF16 && dtype != INC_F16) return INC_ERR_UNSUPPORTED;
  // the launch configurations of torch's reduction whose order the kernel reproduces (see above); fewer than 8 rows, narrower or
  // wider rows reduce in another order
  if (rows < 8 || cols % 8 != 0 || cols < 256 || cols > 16384 || rows >= (1ll << 40)) return INC_ERR_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(w) || !aligned16(out)) return INC_ERR_UNSUPPORTED;
  if (ceil_div64(rows, 2) > 0x7fffffff) return INC_ERR_UNSUPPORTED;
  const float factor = static_cast<float>(rows) / static_cast<float>(rows * cols);  // mean_kernel_impl: float(outputs) / numel
  const int c = (int)cols;
  hipStream_t s = inc_s(stream);
#define INC_RMS(W, JJ)                                                                        \
  do {                                                                                        \
    if (dtype == INC_BF16) rmsnorm_launch<INC_BF16, W, JJ>(x, w, out, rows, c, eps, factor, s); \
    else rmsnorm_launch<INC_F16, W, JJ>(x, w, out, rows, c, eps, factor, s);                    \
  } while (0)
  if (cols <= 8128) {  // one torch wave per row: J pieces of 16 bytes per lane of the half wave, 256 elements per J
    if (cols <= 2048) INC_RMS(1, 8);
    else if (cols <= 4096) INC_RMS(1, 16);
    else if (cols <= 6144) INC_RMS(1, 24);
    else INC_RMS(1, 32);
  } else {             // eight torch waves per row, 2048 elements per J
    INC_RMS(8, 8);
  }
#undef INC_RMS
  INC_LAUNCH_RETURN();
}

}  // extern "C"
