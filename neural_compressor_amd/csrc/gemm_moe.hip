// gemm_moe.hip -- K4e: weight-only INT4 fused MoE experts (route, grouped dequant-GEMM, combine).
//
// Replaces transformers' MixtralExperts.forward (also the Qwen2-MoE / Qwen3-MoE / OLMoE experts, which share it): a host loop over
// the experts that were hit (found with nonzero(), a host wait), two F.linear per expert and an index_add_.  Here one forward is four
// launches and no host synchronisation:
//
//   inc_moe_route      top_k_index [T,k] -> per-expert offsets, the slots sorted by expert (ascending flat slot t*k+s inside an expert:
//                      a fixed order, so results are deterministic), the inverse map and a table of 64-row tiles
//   inc_woq_moe_gemm   mode 0 (gate_up): h[p, j] = rx( silu(x[tok(p)] . Wg[e, j]) * (x[tok(p)] . Wu[e, j]) ),  j < I
//                      mode 1 (down):    y[p, n] = w[slot(p)] * (h[p] . Wd[e, n])                      (fp32)
//                      mode 2 (plain):   y[p, n] = x[tok(p)] . W[e, n]                                   (fp32, for tests)
//   inc_moe_combine    out[t] = rx( sum_s y[pos(t, s)] ), s = 0 .. k-1 in order, fp32
//
// p is a position in the sorted slot order, e the expert of its tile, rx the rounding to x's dtype.  W is each expert's slice of the
// optimum layout stacked on a leading expert axis (qweight [E, K/8, N] int32, scales [E, G, N] fp16, qzeros [E, G, N/8] int32) and is
// dequantised exactly as inc_woq_dequant does (the fp8-converter form of gemm_common.hpp), so the weight an expert decodes is
// recover(x.dtype) bit for bit.
//
// GEMM kernel: workgroup = (256-column strip, 64-row tile, K slice); wave w owns columns 64 w .. 64 w + 63 of the strip, lane (jn, oct)
// loads one 16-byte word group (8 k of 4 adjacent columns) per 32-k step -- four B fragments of v_mfma_f32_16x16x32 (the
// woq_gemv_w4_body pattern) -- and gate_up streams the gate and the up column of the same j, so the SiLU product is formed in registers.
// A rows are gathered through the slot list (gate_up) or read in place (down).  Tiles with no work and blocks of 16 rows past a tile's
// end skip their loads and MFMAs (wave-uniform branches).  When (tile, strip) pairs alone leave the chip idle the K range is split over
// workgroups: fp32 partial slabs written through (sc1), one relaxed agent-scope ticket per (tile, strip), the last arriver sums the
// slabs in slice order (the hand-off of gemm_lut.hip), so repeated calls are bit-identical and the counters re-arm themselves.
#include "gemm_common.hpp"
#include "moe_common.hpp"  // the route buffer's layout, the routing-weight load

namespace {

constexpr int MOE_BN = 256;          // output columns per workgroup (4 waves x 64)
constexpr int MOE_ROUTE_WAVES = 16;  // route kernel: 1024 threads
// split-K arrival counters: a fixed region at the start of the workspace (a split runs only while (tile slot, strip) pairs are fewer
// than 512), so one workspace serves every call shape and both GEMMs -- the partials of one call never land on another's counters
constexpr int64_t MOE_COUNTER_BYTES = 4 << 10;

__device__ __forceinline__ int moe_bucket(const void* idx, int idx8, int64_t i, int E) {
  const int64_t e = idx8 ? static_cast<const int64_t*>(idx)[i] : (int64_t) static_cast<const int32_t*>(idx)[i];
  return (e < 0 || e >= E) ? E : (int)e;  // out-of-range ids (e.g. a "no expert" sentinel) go to bucket E: no tile, no contribution
}

// One workgroup.  Wave w owns the slots [w seg, (w + 1) seg): it counts them per expert, a scan turns the counts into offsets (and
// per-wave starting points inside each expert), then every wave walks its slots again in order and places them: a stable counting sort.
__global__ __launch_bounds__(1024) void moe_route_kernel(const void* __restrict__ idx, int idx8, int S, int E, int* __restrict__ route) {
  __shared__ int cnt[MOE_ROUTE_WAVES][MOE_MAX_E + 1];
  __shared__ int sa[1024], sb[1024];
  __shared__ int offs[MOE_MAX_E + 1];
  const RouteLayout L = moe_route_layout(S, E);
  int* const offsets = route + L.offsets;
  int* const order = route + L.order;
  int* const pos = route + L.pos;
  int* const tiles = route + L.tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < MOE_ROUTE_WAVES * (MOE_MAX_E + 1); i += 1024) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int seg = (S + MOE_ROUTE_WAVES - 1) / MOE_ROUTE_WAVES;
  const int beg = wave * seg < S ? wave * seg : S;
  const int end = beg + seg < S ? beg + seg : S;
  for (int i = beg + lane; i < end; i += 64) atomicAdd(&cnt[wave][moe_bucket(idx, idx8, i, E)], 1);
  __syncthreads();
  int tot = 0;
  if (tid <= E) {
    for (int w = 0; w < MOE_ROUTE_WAVES; ++w) {
      const int c = cnt[w][tid];
      cnt[w][tid] = tot;  // this wave's first rank inside the bucket
      tot += c;
    }
  }
  const int a0 = tid <= E ? tot : 0, b0 = tid < E ? (tot + MOE_BM - 1) / MOE_BM : 0;
  sa[tid] = a0;
  sb[tid] = b0;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // inclusive scans of the bucket sizes and of the tile counts
    const int va = tid >= d ? sa[tid - d] : 0, vb = tid >= d ? sb[tid - d] : 0;
    __syncthreads();
    sa[tid] += va;
    sb[tid] += vb;
    __syncthreads();
  }
  if (tid <= E) {
    offs[tid] = sa[tid] - a0;
    offsets[tid] = sa[tid] - a0;  // offsets[E] = number of slots with a valid expert
  }
  if (tid < E) {
    const int t0 = sb[tid] - b0, p0 = sa[tid] - a0;
    for (int j = 0; j < b0; ++j) {
      tiles[2 * (t0 + j)] = tid;
      tiles[2 * (t0 + j) + 1] = p0 + MOE_BM * j;
    }
  }
  if (tid == 0) route[0] = sb[1023];
  __syncthreads();
  for (int base = beg; base < end; base += 64) {
    const int i = base + lane;
    const bool act = i < end;
    const int e = act ? moe_bucket(idx, idx8, i, E) : -1;
    unsigned long long pending = __ballot(act);
    while (pending) {
      const int leader = __builtin_ctzll(pending);
      const int e0 = __shfl(e, leader);
      const unsigned long long m = __ballot(act && e == e0);
      int b = 0;
      if (lane == leader) b = atomicAdd(&cnt[wave][e0], __popcll(m));
      b = __shfl(b, leader);
      if (act && e == e0) {
        const int p = offs[e0] + b + __popcll(m & ((1ull << lane) - 1ull));
        order[p] = i;
        pos[i] = p;
      }
      pending &= ~m;
    }
  }
}

// MODE 0 gate_up (N = 2I, output h [S, I] of x's dtype), 1 down (output fp32 [S, N] x routing weight), 2 plain (fp32 [S, N]).
// G4: the 128 k of four consecutive steps lie in one group (group_size >= 128 or one group per row): group parameters once per chunk.
template <bool IS_BF16, int MODE, bool G4>
__global__ __launch_bounds__(256) void woq_moe_gemm_kernel(
    const uint16_t* __restrict__ a, const int* __restrict__ route, const uint32_t* __restrict__ qweight,
    const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros, const void* __restrict__ rw, int wdt,
    void* __restrict__ out, float* __restrict__ partial, unsigned* __restrict__ counters, int S, int top_k, int E, int64_t N,
    int64_t K, int G, int g_shift, int splitk, int nsteps) {
  __shared__ int last_flag;
  constexpr int NS = MODE == 0 ? 2 : 1;  // weight streams: gate and up columns of the same j
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jn = lane & 15, oct = lane >> 4;
  const int strip = (int)blockIdx.x, tile = (int)blockIdx.y, slice = (int)blockIdx.z;
  if (tile >= route[0]) return;  // more tile slots than tiles: nothing to do (the whole workgroup, before any counter)
  const RouteLayout L = moe_route_layout(S, E);
  const int e = route[L.tiles + 2 * tile], p0 = route[L.tiles + 2 * tile + 1];
  const int pe = route[L.offsets + e + 1];
  const int rows = pe - p0 < MOE_BM ? pe - p0 : MOE_BM;
  const int* const order = route + L.order;
  const int64_t Nout = MODE == 0 ? N / 2 : N;
  const int64_t ncol0 = (int64_t)strip * MOE_BN + 64 * wave + 4 * jn;
  const bool n_ok = ncol0 < Nout;
  const int64_t ncol = n_ok ? ncol0 : Nout - 4;  // clamped lanes recompute valid columns; their results are not stored
  const int64_t coff[2] = {ncol, Nout + ncol};
  const int64_t NW = N / 8;
  const uint32_t* const qw = qweight + (int64_t)e * (K / 8) * N;
  const uint16_t* const sc = scales + (int64_t)e * G * N;
  const uint32_t* const qz = qzeros + (int64_t)e * G * NW;
  const uint16_t* arow[4];
  bool a_ok[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int r = 16 * b + jn;
    a_ok[b] = r < rows;
    const int p = a_ok[b] ? p0 + r : p0;
    arow[b] = MODE == 1 ? a + (int64_t)p * K : a + (int64_t)(order[p] / top_k) * K;
  }
  const float inv_u = fp8_unit_inverse();
  const int steps = (int)(K / 32);
  const int st_beg = slice * nsteps;
  const int st_end = st_beg + nsteps < steps ? st_beg + nsteps : steps;

  f32x4 acc[NS][4][4];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[s][b][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int NG = G4 ? 1 : 4;
  for (int st0 = st_beg; st0 < st_end; st0 += 4) {
    uint4 w[NS][4], av[4][4];
    uint2 sr[NS][NG];
    uint32_t zr[NS][NG];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int st = st0 + u < st_end ? st0 + u : st_end - 1;  // past-the-end steps re-read the last one and are skipped below
#pragma unroll
      for (int s = 0; s < NS; ++s) w[s][u] = *reinterpret_cast<const uint4*>(qw + ((int64_t)st * 4 + oct) * N + coff[s]);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        av[b][u] = make_uint4(0u, 0u, 0u, 0u);
        if (16 * b < rows) {
          const uint4 v = *reinterpret_cast<const uint4*>(arow[b] + (int64_t)st * 32 + 8 * oct);
          if (a_ok[b]) av[b][u] = v;
        }
      }
    }
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
      const int st = st0 + gi < st_end ? st0 + gi : st_end - 1;
      const int64_t g = g_shift >= 0 ? (((int64_t)st * 32) >> g_shift) : 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        sr[s][gi] = *reinterpret_cast<const uint2*>(sc + g * N + coff[s]);
        zr[s][gi] = qz[g * NW + (coff[s] >> 3)];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (st0 + u >= st_end) break;
      const int gi = G4 ? 0 : u;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int zsh = 4 * (int)(coff[s] & 7);  // coff % 4 == 0: the 4 zero nibbles sit at bits zsh .. zsh+15
        const uint32_t sw[2] = {sr[s][gi].x, sr[s][gi].y};
        const uint32_t ww[4] = {w[s][u].x, w[s][u].y, w[s][u].z, w[s][u].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float scl = f16_bits_to_f32((uint16_t)(sw[c >> 1] >> (16 * (c & 1))));
          uint32_t zz = ((zr[s][gi] >> (zsh + 4 * c)) & 15u) + 1u;
          zz = zz > 15u ? 0u : zz;
          const uint4 bq = dequant8<IS_BF16>(ww[c], scl * inv_u, -(float)zz * scl);
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (16 * b < rows) acc[s][b][c] = mfma16<IS_BF16>(av[b][u], bq, acc[s][b][c]);
        }
      }
    }
  }

  // D of 16x16x32: lane holds column 4 jn + c (accumulator c) and rows 16 b + 4 oct + r
  if (splitk > 1) {
    const int64_t slab = (int64_t)S * N;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * b + 4 * oct + r;
          if (n_ok && row < rows) {
            float* dst = partial + (int64_t)slice * slab + (int64_t)(p0 + row) * N + coff[s];
#pragma unroll
            for (int c = 0; c < 4; ++c) __hip_atomic_store(dst + c, acc[s][b][c][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
          }
        }
    // publish: drain, barrier, one ticket (splitk_arrive, gemm_common.hpp)
    if (!splitk_arrive(counters + (int64_t)tile * gridDim.x + strip, splitk, &last_flag)) return;
    // last arriver: fixed-order sum over the slices (its own slab included)
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[s][b][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int sl = 0; sl < splitk; ++sl) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * b + 4 * oct + r;
            if (n_ok && row < rows) {
              const float* src = partial + (int64_t)sl * slab + (int64_t)(p0 + row) * N + coff[s];
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[s][b][c][r] += __hip_atomic_load(src + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
            }
          }
    }
  }
  if (!n_ok) return;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * b + 4 * oct + r;
      if (row >= rows) continue;
      const int64_t p = p0 + row;
      if constexpr (MODE == 0) {
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float g = acc[0][b][c][r], u = acc[1][b][c][r];
          v[c] = silu_mul_f32(g, u);
        }
        uint2 o;
        o.x = pack2<IS_BF16>(v[0], v[1]);
        o.y = pack2<IS_BF16>(v[2], v[3]);
        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + p * Nout + ncol) = o;
      } else {
        const float wt = MODE == 1 ? moe_load_weight(rw, order[p], wdt) : 1.f;
        float4 o;
        o.x = acc[0][b][0][r] * wt;
        o.y = acc[0][b][1][r] * wt;
        o.z = acc[0][b][2][r] * wt;
        o.w = acc[0][b][3][r] * wt;
        *reinterpret_cast<float4*>(static_cast<float*>(out) + p * N + ncol) = o;
      }
    }
}

template <bool IS_BF16>
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, const int* __restrict__ route, uint16_t* __restrict__ out,
                                                          int T, int top_k, int E, int64_t H) {
  const int S = T * top_k;
  const RouteLayout L = moe_route_layout(S, E);
  const int nvalid = route[L.offsets + E];
  const int* const pos = route + L.pos;
  const int64_t H4 = H / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)T * H4) return;
  const int64_t t = i / H4, c = 4 * (i % H4);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < top_k; ++s) {
    const int p = pos[t * top_k + s];
    if (p < nvalid) {
      const float4 v = *reinterpret_cast<const float4*>(y + (int64_t)p * H + c);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  uint2 o;
  o.x = pack2<IS_BF16>(acc.x, acc.y);
  o.y = pack2<IS_BF16>(acc.z, acc.w);
  *reinterpret_cast<uint2*>(out + t * H + c) = o;
}

// split-K plan: about two workgroups per CU counting every tile slot; whole 4-step chunks per slice, at least one chunk; no split once
// the (tile slot, strip) pairs alone reach 512
struct MoePlan {
  int strips, tiles_max, splitk, nsteps;
};
MoePlan moe_plan(int mode, int64_t S, int64_t E, int64_t N, int64_t K) {
  MoePlan p;
  const int64_t Nout = mode == 0 ? N / 2 : N;
  p.strips = (int)ceil_div64(Nout, MOE_BN);
  p.tiles_max = (int)moe_tiles_max(S, E);
  const int64_t steps = K / 32, units = (int64_t)p.strips * p.tiles_max;
  int64_t sk = units >= 512 ? 1 : ceil_div64(512, units);
  const int64_t cap = ceil_div64(steps, 4);
  if (sk > cap) sk = cap;
  if (sk < 1) sk = 1;
  int64_t ns = ceil_div64(steps, sk);
  ns = ceil_div64(ns, 4) * 4;
  p.nsteps = (int)ns;
  p.splitk = (int)ceil_div64(steps, ns);
  return p;
}
int64_t moe_ws_bytes(const MoePlan& p, int64_t S, int64_t N) {
  if (p.splitk <= 1) return 0;
  return MOE_COUNTER_BYTES + (int64_t)p.splitk * S * N * 4;
}

template <bool IS_BF16, int MODE>
int launch_moe(bool g4, dim3 grid, hipStream_t s, const uint16_t* a, const int* route, const uint32_t* qw, const uint16_t* sc,
               const uint32_t* qz, const void* rw, int wdt, void* out, float* part, unsigned* counters, int S, int top_k, int E, int64_t N,
               int64_t K, int G, int g_shift, int splitk, int nsteps) {
  if (g4)
    woq_moe_gemm_kernel<IS_BF16, MODE, true><<<grid, 256, 0, s>>>(a, route, qw, sc, qz, rw, wdt, out, part, counters, S, top_k, E, N, K, G,
                                                                  g_shift, splitk, nsteps);
  else
    woq_moe_gemm_kernel<IS_BF16, MODE, false><<<grid, 256, 0, s>>>(a, route, qw, sc, qz, rw, wdt, out, part, counters, S, top_k, E, N, K, G,
                                                                   g_shift, splitk, nsteps);
  INC_LAUNCH_RETURN();
}

}  // namespace

extern "C" {

int64_t inc_moe_route_bytes(int64_t T, int top_k, int64_t E) {
  if (T <= 0 || top_k <= 0 || E <= 0) return 0;
  return moe_route_layout(T * top_k, E).total * 4;
}

int inc_moe_route(const void* top_k_index, int index_bytes, int64_t T, int top_k, int64_t E, int32_t* route, int64_t route_bytes,
                  inc_stream_t stream) {
  INC_CHECK_ARG(top_k_index && route && T > 0 && top_k > 0 && E > 0 && (index_bytes == 4 || index_bytes == 8));
  if (E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  if (route_bytes < inc_moe_route_bytes(T, top_k, E)) return INC_ERR_WORKSPACE;
  moe_route_kernel<<<1, 1024, 0, inc_s(stream)>>>(top_k_index, index_bytes == 8, (int)(T * top_k), (int)E, route);
  INC_LAUNCH_RETURN();
}

int64_t inc_woq_moe_gemm_workspace_bytes(int mode, int64_t T, int top_k, int64_t E, int64_t N, int64_t K) {
  if (mode < 0 || mode > 2 || T <= 0 || top_k <= 0 || E <= 0 || N <= 0 || K < 32) return 0;
  // shapes inc_woq_moe_gemm rejects before it plans need no workspace (mode 0 with N = 1 has no column, so no strip to plan over)
  if (N % 8 != 0 || K % 32 != 0) return 0;
  const int64_t S = T * top_k;
  return moe_ws_bytes(moe_plan(mode, S, E, N, K), S, N);
}

int inc_woq_moe_gemm(int mode, const void* a, int xdtype, const int32_t* route, const int32_t* qweight, const uint16_t* scales,
                     const int32_t* qzeros, const void* routing_weights, int wdtype, void* out, int64_t T, int top_k, int64_t E, int64_t N,
                     int64_t K, int64_t G, int group_size, void* workspace, int64_t workspace_bytes, inc_stream_t stream) {
  INC_CHECK_ARG(mode >= 0 && mode <= 2);
  INC_CHECK_ARG(a && route && qweight && scales && qzeros && out && T > 0 && top_k > 0 && E > 0 && N > 0 && K > 0 && G > 0);
  INC_CHECK_ARG(group_size > 0 || group_size == -1);
  INC_CHECK_ARG(mode != 1 || routing_weights);
  if (xdtype != INC_BF16 && xdtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if (mode == 1 && wdtype != INC_F32 && wdtype != INC_F16 && wdtype != INC_BF16) return INC_ERR_UNSUPPORTED;
  if (E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  const int64_t gs = (group_size == -1 || group_size >= K) ? K : group_size;
  INC_CHECK_ARG(G == ceil_div64(K, gs));
  if (K % 32 != 0 || N % 8 != 0) return INC_ERR_UNSUPPORTED;
  int g_shift = -1;
  if (gs != K) {
    if (gs < 32 || (gs & (gs - 1)) != 0 || K % gs != 0) return INC_ERR_UNSUPPORTED;  // groups: powers of two >= 32 that divide K
    g_shift = 0;
    while ((int64_t(1) << g_shift) < gs) ++g_shift;
  }
  if ((reinterpret_cast<uintptr_t>(a) & 15) || (reinterpret_cast<uintptr_t>(qweight) & 15) || (reinterpret_cast<uintptr_t>(scales) & 7) ||
      (reinterpret_cast<uintptr_t>(out) & 15))
    return INC_ERR_UNSUPPORTED;
  const int64_t S = T * top_k;
  const MoePlan p = moe_plan(mode, S, E, N, K);
  const int64_t need = moe_ws_bytes(p, S, N);
  if (need > 0 && (!workspace || workspace_bytes < need)) return INC_ERR_WORKSPACE;
  unsigned* counters = static_cast<unsigned*>(workspace);
  float* part = need > 0 ? reinterpret_cast<float*>(static_cast<char*>(workspace) + MOE_COUNTER_BYTES) : nullptr;
  const dim3 grid((unsigned)p.strips, (unsigned)p.tiles_max, (unsigned)p.splitk);
  const bool g4 = gs == K || gs >= 128;
  const auto* aa = static_cast<const uint16_t*>(a);
  const auto* qw = reinterpret_cast<const uint32_t*>(qweight);
  const auto* qz = reinterpret_cast<const uint32_t*>(qzeros);
  hipStream_t s = inc_s(stream);
#define INC_MOE_ARGS g4, grid, s, aa, route, qw, scales, qz, routing_weights, wdtype, out, part, counters, (int)S, top_k, (int)E, N, K, (int)G, \
                     g_shift, p.splitk, p.nsteps
  if (xdtype == INC_BF16) {
    if (mode == 0) return launch_moe<true, 0>(INC_MOE_ARGS);
    if (mode == 1) return launch_moe<true, 1>(INC_MOE_ARGS);
    return launch_moe<true, 2>(INC_MOE_ARGS);
  }
  if (mode == 0) return launch_moe<false, 0>(INC_MOE_ARGS);
  if (mode == 1) return launch_moe<false, 1>(INC_MOE_ARGS);
  return launch_moe<false, 2>(INC_MOE_ARGS);
#undef INC_MOE_ARGS
}

int inc_moe_combine(const float* y, const int32_t* route, void* out, int xdtype, int64_t T, int top_k, int64_t E, int64_t H,
                    inc_stream_t stream) {
  INC_CHECK_ARG(y && route && out && T > 0 && top_k > 0 && E > 0 && H > 0);
  if (xdtype != INC_BF16 && xdtype != INC_F16) return INC_ERR_UNSUPPORTED;
  if (H % 4 != 0 || E > MOE_MAX_E || T * top_k > MOE_MAX_SLOTS) return INC_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(y) & 15) || (reinterpret_cast<uintptr_t>(out) & 7)) return INC_ERR_UNSUPPORTED;
  const int64_t n = T * (H / 4);
  const unsigned blocks = (unsigned)ceil_div64(n, 256);
  auto* o = static_cast<uint16_t*>(out);
  if (xdtype == INC_BF16)
    moe_combine_kernel<true><<<blocks, 256, 0, inc_s(stream)>>>(y, route, o, (int)T, top_k, (int)E, H);
  else
    moe_combine_kernel<false><<<blocks, 256, 0, inc_s(stream)>>>(y, route, o, (int)T, top_k, (int)E, H);
  INC_LAUNCH_RETURN();
}

}  // extern "C"
