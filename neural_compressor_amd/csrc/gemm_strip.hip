// gemm_strip.hip -- the mid-M strip kernel (64 < M <= STRIP_MAX_M) of the fused dequant-GEMM (inc_woq_gemm, gemm.hip): 64 rows x 128 columns per workgroup,
// the K range divided over its eight waves.  Its successor for M > 128 without K-slices is gemm_strip8.hip.
#include "gemm_common.hpp"

namespace {

// The 256 x 256 tile needs split-K over 8-16 fp32 slabs to put such a problem on 256 CUs (M = 512, 4096^2: 32 tiles, 134 MB of
// slab traffic, 62 us; M = 128: 30 us).  This kernel extends the streaming kernel instead: a workgroup owns 64 rows x 128
// columns for the WHOLE of K (or 1/splitk of it when rows x columns alone leave CUs idle), its eight waves take an eighth of
// the K-steps each, and a wave's packed-weight loads ARE its MFMA B fragments (a lane's uint4 = 8 consecutive k of 4 adjacent
// columns), dequantised in registers and fed to four 16x16x32 MFMAs each; the waves' accumulators meet in LDS at the end (64 x 64
// outputs per pass).  Split-K (only when needed, <= 4 slices) hands over like the streaming kernel: write-through partials, one
// relaxed ticket, the last arriver sums in slice order -> deterministic.
constexpr int STRIP_WAVES = 8;                                          // waves per workgroup: eighths of the K range
constexpr int STRIP_RING = 3;                                           // operand slots (K-steps in flight) per wave
constexpr int STRIP_SMEM_BYTES = STRIP_WAVES * STRIP_RING * 6 * 1024;   // 144 KiB: the operand rings; the epilogue reuses them
static_assert(STRIP_SMEM_BYTES >= STRIP_WAVES * 64 * 68 * 4, "the reduction buffer (WAVES x 64 x 68 fp32) aliases the rings");
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// ABL (harness build only, timing-only, WRONG results): bit 0 no x requests, bit 1 no W requests, bit 2 no MFMA / dequantisation
template <bool IS_BF16, int WAVES, int RING, int ABL = 0>
__global__ __launch_bounds__(64 * WAVES) void woq_gemm_w4_strip_kernel(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counters, int M, int64_t N, int64_t K, int64_t NW, int g_shift, int splitk) {
  constexpr int MB = 4, NB = 2;  // 16-row blocks and 64-column groups of a wave: the operand requests below are written out for these
  constexpr int ROWS = 16 * MB, COLS = 64 * NB, NT = 64 * WAVES;
  extern __shared__ __attribute__((aligned(16))) char strip_smem[];
  float* const red = reinterpret_cast<float*>(strip_smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jn = lane & 15, oct = lane >> 4;
  const float inv_u = fp8_unit_inverse();
  // XCD-aware tile order: workgroup L (dispatch order: x fastest, then y) runs on XCD L % 8.  The tiles are renumbered so that an
  // XCD owns a CONTIGUOUS range of (row strip, column strip) pairs, row strip major: the 32 column strips of one 64-row strip
  // share that strip's x rows (512 KiB at K = 4096) out of ONE XCD's L2 instead of every XCD streaming the whole of x (4 MiB at
  // M = 512, the size of an L2) from the Infinity Cache.
  int bx = (int)blockIdx.x, by = (int)blockIdx.y;
  {
    const int nx = (int)gridDim.x, nt = nx * (int)gridDim.y, L = by * nx + bx;
    const int t = xcd_remap(L, nt);
    by = t / nx;
    bx = t - by * nx;
  }
  const int64_t n0 = (int64_t)bx * COLS;
  const int m0 = by * ROWS;
  const int slice = blockIdx.z;

  int64_t ncol[NB];
  int zsh[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    ncol[nb] = n0 + 64 * nb + 4 * jn;
    if (ncol[nb] > N - 4) ncol[nb] = N - 4;  // clamped lanes recompute valid columns; their results are not stored
    zsh[nb] = 4 * (int)(ncol[nb] & 7);
  }
  // this wave's K-steps (32 k each): an even share of the slice-and-wave grid
  const int steps_total = (int)(K / 32);
  const int Q = WAVES * splitk, q = slice * WAVES + wave;
  const int lo = (int)((int64_t)steps_total * q / Q), hi = (int)((int64_t)steps_total * (q + 1) / Q);

  // Operand pipeline.  hipcc sinks plain loads to their first use, and a wave then pays the full memory latency in every step
  // (measured: 1.4 us per step); pinned register prefetch one step ahead is all the register file allows next to 128
  // accumulators at two waves per SIMD, and was still latency-bound (a third of the wave time issuing).  So the fragments travel
  // through LDS without touching a register: every wave owns a ring of RING slots of 6 KiB; a step's four x fragments and two
  // weight fragments arrive by six LDS-DMA requests (lane-linear image = the fragment layout), RING steps ahead of the MFMAs, and
  // are picked up with six conflict-free ds_read_b128.  The raw group parameters (4 small requests per step) stay register
  // loads in the same in-order queue: one step = 10 requests.
  struct Step {  // x and weight fragments of one K-step
    uint4 a[4];
    uint4 w[2];
  };
  struct Par {  // raw scales / zero-point words of the step's group
    u32x2 s[2];
    uint32_t z[2];
  };
  constexpr int SLOT = 6 * 1024;
  const uint32_t ring0 = (uint32_t)(uintptr_t)strip_smem + (uint32_t)wave * (RING * SLOT);
  uint32_t xoff[4], woff[2], soff[2], zoff[2];
  // x fragments: FOUR ADJACENT LANES fetch the 64 contiguous bytes (32 k) of one row -- the memory pipeline coalesces adjacent
  // lanes only; with the MFMA operand's own lane order (adjacent lanes = adjacent rows, 8 KiB apart) every lane is its own
  // 16-byte request and the workgroup gets ~11 bytes per clock (measured).  Lane l lands at byte 16 l of the slot and carries row
  // l >> 2, 16-byte chunk (l & 3) ^ (row >> 2): the XOR makes the pick-up below (lane (jn, oct) reads row jn, chunk oct)
  // conflict-free.
  const int xr = lane >> 2, xc = (lane & 3) ^ (xr >> 2);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    int am = m0 + 16 * b + xr;
    if (am > M - 1) am = M - 1;  // rows past M are computed from a valid row and never stored
    xoff[b] = (uint32_t)(((int64_t)am * K + 8 * xc) * 2);
  }
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    woff[nb] = (uint32_t)(((int64_t)oct * N + ncol[nb]) * 4);
    soff[nb] = (uint32_t)(ncol[nb] * 2);
    zoff[nb] = (uint32_t)((ncol[nb] >> 3) * 4);
  }
  auto issue = [&](int slot, Par& p, int st) {
    st = st > hi - 1 ? hi - 1 : st;  // the prefetch past the end re-reads the last step
    const int64_t g = g_shift >= 0 ? (((int64_t)st * 32) >> g_shift) : 0;
    const uint16_t* xb = x + (int64_t)st * 32;
    const uint32_t* wb = qweight + (int64_t)st * 4 * N;
    const uint16_t* sb = scales + g * N;
    const uint32_t* zb = qzeros + g * NW;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(ring0 + (uint32_t)slot * SLOT);
    uint32_t keep;
    if constexpr (ABL & 3) {  // timing-only: the same ten-request step with some requests left out (vmcnt bookkeeping is by count, so
                              // every omitted request is replaced by a 4-byte load of the parameter words)
      asm volatile("s_mov_b32 %0, m0" : "=&s"(keep));
#define INC_STRIP_REQ(COND, OFF, BASE, LDSOFF)                                                                                  \
  if constexpr (COND) asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(OFF), "s"(BASE), "s"(dst), "i"(LDSOFF) : "memory", "scc"); \
  else asm volatile("global_load_dword %0, %1, %2" : "=&v"(p.z[0]) : "v"(zoff[0]), "s"(zb) : "memory");
      INC_STRIP_REQ((ABL & 1) == 0, xoff[0], xb, 0x0)
      INC_STRIP_REQ((ABL & 1) == 0, xoff[1], xb, 0x400)
      INC_STRIP_REQ((ABL & 1) == 0, xoff[2], xb, 0x800)
      INC_STRIP_REQ((ABL & 1) == 0, xoff[3], xb, 0xc00)
      INC_STRIP_REQ((ABL & 2) == 0, woff[0], wb, 0x1000)
      INC_STRIP_REQ((ABL & 2) == 0, woff[1], wb, 0x1400)
#undef INC_STRIP_REQ
      asm volatile("global_load_dwordx2 %0, %4, %6\n\tglobal_load_dwordx2 %1, %5, %6\n\tglobal_load_dword %2, %7, %9\n\tglobal_load_dword %3, %8, %9\n\ts_mov_b32 m0, %10"
                   : "=&v"(p.s[0]), "=&v"(p.s[1]), "=&v"(p.z[0]), "=&v"(p.z[1])
                   : "v"(soff[0]), "v"(soff[1]), "s"(sb), "v"(zoff[0]), "v"(zoff[1]), "s"(zb), "s"(keep)
                   : "memory");
      return;
    }
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_nop 4\n\t"
        "s_mov_b32 m0, %19\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %5, %15\n\t"
        "s_add_u32 m0, %19, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %6, %15\n\t"
        "s_add_u32 m0, %19, 0x800\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %7, %15\n\t"
        "s_add_u32 m0, %19, 0xc00\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %8, %15\n\t"
        "s_add_u32 m0, %19, 0x1000\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %9, %16\n\t"
        "s_add_u32 m0, %19, 0x1400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %10, %16\n\t"
        "global_load_dwordx2 %1, %11, %17\n\t"
        "global_load_dwordx2 %2, %12, %17\n\t"
        "global_load_dword %3, %13, %18\n\t"
        "global_load_dword %4, %14, %18\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&v"(p.s[0]), "=&v"(p.s[1]), "=&v"(p.z[0]), "=&v"(p.z[1])
        : "v"(xoff[0]), "v"(xoff[1]), "v"(xoff[2]), "v"(xoff[3]), "v"(woff[0]), "v"(woff[1]), "v"(soff[0]), "v"(soff[1]), "v"(zoff[0]),
          "v"(zoff[1]), "s"(xb), "s"(wb), "s"(sb), "s"(zb), "s"(dst)
        : "memory", "scc");
  };
  // the oldest of RING steps in flight has landed in its slot / its parameter registers (the younger ones stay in flight)
  auto landed = [&](Par& p) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(p.s[0]), "+v"(p.s[1]), "+v"(p.z[0]), "+v"(p.z[1]) : "i"(10 * (RING - 1)) : "memory");
  };
  auto fetch_issue = [&](Step& t, int slot) {
    const char* base = strip_smem + wave * (RING * SLOT) + slot * SLOT;
    const int apos = (4 * jn + (oct ^ (jn >> 2))) * 16;  // where row jn, chunk oct of an x fragment landed
#pragma unroll
    for (int b = 0; b < 4; ++b) t.a[b] = *reinterpret_cast<const uint4*>(base + b * 1024 + apos);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) t.w[nb] = *reinterpret_cast<const uint4*>(base + 4096 + nb * 1024 + lane * 16);
  };
  auto fetch = [&](Step& t, int slot) {
    fetch_issue(t, slot);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot is free for the next DMA once these have returned
  };

  f32x4 acc[MB][4 * NB];
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int c = 0; c < 4 * NB; ++c) acc[b][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // scale / zero point of this lane's 8 columns, refreshed when the K-step enters a new group (every 2^(g_shift-5) steps)
  float scu[4 * NB], nzs[4 * NB];
  const int gmask = g_shift < 0 ? 0x7fffffff : ((1 << (g_shift - 5)) - 1);
  auto refresh = [&](const Par& p, int st) {
    if (st == lo || (st & gmask) == 0) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float sc = f16_bits_to_f32((uint16_t)(p.s[nb][c >> 1] >> (16 * (c & 1))));
          uint32_t zz = ((p.z[nb] >> (zsh[nb] + 4 * c)) & 15u) + 1u;  // modules.py:407-410 (stored zp - 1; wraps above 15)
          zz = zz > 15u ? 0u : zz;
          scu[4 * nb + c] = sc * inv_u;
          nzs[4 * nb + c] = -(float)zz * sc;
        }
    }
  };
  auto compute = [&](const Step& t) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const uint32_t ww[4] = {t.w[nb].x, t.w[nb].y, t.w[nb].z, t.w[nb].w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint4 bq = dequant8<IS_BF16>(ww[c], scu[4 * nb + c], nzs[4 * nb + c]);
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[b][4 * nb + c] = mfma16<IS_BF16>(t.a[b], bq, acc[b][4 * nb + c]);
      }
    }
  };

  static_assert(RING >= 2 && 10 * (RING - 1) < 64, "vmcnt counts 63 requests at most");
  // ABL bit 3 (harness A/B, CORRECT results): the LDS reads of step s + 1 are requested before the MFMAs of step s (two fragment
  // sets) instead of each step waiting for its own reads in front of its MFMAs; bit 4: s_setprio 1 around a step's dequantise + MFMA
  if constexpr ((ABL & 8) != 0) {
    if (lo < hi) {
      Par p[RING];
      Step t[2];
#pragma unroll
      for (int r = 0; r < RING; ++r) issue(r, p[r], lo + r);
      landed(p[0]);
      fetch_issue(t[0], 0);
      for (int st = lo; st < hi; st += 2 * RING) {  // two rounds of the ring per iteration: the fragment set index stays a constant
#pragma unroll
        for (int rr = 0; rr < 2 * RING; ++rr) {
          constexpr int dummy = 0;
          (void)dummy;
          const int r = rr % RING;
          if (st + rr < hi) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // t[rr & 1] has arrived: slot r is free
            refresh(p[r], st + rr);
            issue(r, p[r], st + rr + RING);
            if (st + rr + 1 < hi) {
              landed(p[(r + 1) % RING]);
              fetch_issue(t[(rr + 1) & 1], (r + 1) % RING);
            }
            if constexpr ((ABL & 16) != 0) __builtin_amdgcn_s_setprio(1);
            compute(t[rr & 1]);
            if constexpr ((ABL & 16) != 0) __builtin_amdgcn_s_setprio(0);
          }
        }
      }
    }
  } else if (lo < hi) {
    Par p[RING];  // (indexed by unrolled constants only: registers)
    Step t;
#pragma unroll
    for (int r = 0; r < RING; ++r) issue(r, p[r], lo + r);
    for (int st = lo; st < hi; st += RING) {
#pragma unroll
      for (int r = 0; r < RING; ++r) {
        if (st + r < hi) {
          landed(p[r]);
          fetch(t, r);
          refresh(p[r], st + r);
          issue(r, p[r], st + r + RING);
          if constexpr ((ABL & 16) != 0) __builtin_amdgcn_s_setprio(1);
          if constexpr ((ABL & 4) == 0) compute(t);
          if constexpr ((ABL & 16) != 0) __builtin_amdgcn_s_setprio(0);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped prefetches past the end
  __syncthreads();                                   // every wave's ring is dead: the reduction buffer takes their place

  // ---- the waves' accumulators meet in LDS, 64 rows x 64 columns per pass ---------------------------------------------
  // D of an MFMA: column = lane & 15 -> tile column 4*jn + c, row = 4*oct + r.  Every thread sums and stores FOUR adjacent columns at a
  // time: 16-byte LDS reads, 16-byte write-through partial stores or one 8-byte store of four outputs (round 6: the single-float form of
  // this epilogue was about a third of a mid-M launch, tools/midm_lab)
  const int64_t slab = (int64_t)M * N;
  constexpr int RP = 68;  // row pitch of the reduction buffer in floats
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (nb > 0) __syncthreads();  // the previous pass has been read
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // the lane's 4 adjacent columns of one row: one 16-byte store (row pitch 68 floats = 17 x 16 B)
        *reinterpret_cast<float4*>(red + (wave * 64 + 16 * b + 4 * oct + r) * RP + 4 * jn) =
            make_float4(acc[b][4 * nb + 0][r], acc[b][4 * nb + 1][r], acc[b][4 * nb + 2][r], acc[b][4 * nb + 3][r]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < (64 * 16 + NT - 1) / NT; ++i) {
      const int idx = tid + NT * i, rr = idx >> 4, c4 = (idx & 15) * 4;
      if (idx >= 64 * 16) continue;
      float4 v = *reinterpret_cast<const float4*>(red + rr * RP + c4);
#pragma unroll
      for (int wv = 1; wv < WAVES; ++wv) {  // fixed order
        const float4 u = *reinterpret_cast<const float4*>(red + (wv * 64 + rr) * RP + c4);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
      }
      const int m = m0 + rr;
      const int64_t n = n0 + 64 * nb + c4;
      if (m < M && n < N) {  // N % 4 == 0 on this path: the four columns exist together
        if (splitk > 1) splitk_store16_sc1(partial + (int64_t)slice * slab + (int64_t)m * N + n, f32x4{v.x, v.y, v.z, v.w});
        else store_out4<IS_BF16>(y + (int64_t)m * N + n, v, bias ? bias + n : nullptr);
      }
    }
  }
  if (splitk <= 1) return;
  // publish: drain, barrier, one ticket (splitk_arrive, gemm_common.hpp)
  if (!splitk_arrive(counters + (by * gridDim.x + bx), splitk, red)) return;
  // last arriver: fixed-order sum over the slices (sc1 16-byte loads: the partials were written through); 4 column quads x up to 4
  // slices of a thread are in flight together
  constexpr int QUADS = ROWS * COLS / 4 / NT;
  static_assert(ROWS * COLS / 4 % NT == 0 && QUADS % 4 == 0, "whole batches of four quads per thread");
  for (int i0 = 0; i0 < QUADS; i0 += 4) {
    f32x4 pv[4][4];
    int64_t off[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + NT * (i0 + i), rr = idx / (COLS / 4), c4 = (idx % (COLS / 4)) * 4;
      const int m = m0 + rr;
      const int64_t n = n0 + c4;
      ok[i] = m < M && n < N;
      off[i] = ok[i] ? (int64_t)m * N + n : 0;
    }
    const float* sb[4];
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {  // slab bases are wave-uniform (SGPR pairs); slices past splitk re-read the last one and are not added
      const uint64_t a = (uint64_t)(uintptr_t)(partial + (int64_t)(sl < splitk ? sl : splitk - 1) * slab);
      sb[sl] = reinterpret_cast<const float*>((uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) |
                                                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a)));
    }
    splitk_load16x16_sc1(pv, sb[0], sb[1], sb[2], sb[3], (uint32_t)(off[0] * 4), (uint32_t)(off[1] * 4), (uint32_t)(off[2] * 4), (uint32_t)(off[3] * 4));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v = pv[0][i];
#pragma unroll
      for (int sl = 1; sl < 4; ++sl)
        if (sl < splitk) v += pv[sl][i];
      if (ok[i]) {
        const int64_t n = n0 + ((tid + NT * (i0 + i)) % (COLS / 4)) * 4;
        store_out4<IS_BF16>(y + off[i], make_float4(v[0], v[1], v[2], v[3]), bias ? bias + n : nullptr);
      }
    }
  }
}

}  // namespace

// K-slices of the strip kernel for (M, N, K): split-K only to fill the chip (one workgroup = two waves per SIMD per CU)
int inc_woq_gemm_strip_splitk(int64_t M, int64_t N, int64_t K) {
  const int64_t wgs = ceil_div64(M, 64) * ceil_div64(N, 128);
  int sk = 1;
  if (wgs < 192) {
    sk = (int)(256 / wgs);
    if (sk > 4) sk = 4;                                                   // the last arriver sums <= 4 slabs
    while (sk > 1 && (K / 32) / (STRIP_WAVES * sk) < 4) --sk;            // >= 4 steps per wave
  }
  return sk;
}

// `part` / `counters`: the split-K slabs and the per-tile arrival counters (zero on first use, re-armed by the kernel); unused at splitk == 1
int inc_launch_woq_gemm_strip(const WoqGemmArgs& a, float* part, unsigned* counters, int splitk, int dbg) {
  static std::atomic<uint64_t> strip_attr_set{0};
  if (inc_attr_needed(strip_attr_set)) {
    (void)hipFuncSetAttribute((const void*)woq_gemm_w4_strip_kernel<true, STRIP_WAVES, STRIP_RING>, hipFuncAttributeMaxDynamicSharedMemorySize, STRIP_SMEM_BYTES);
    (void)hipFuncSetAttribute((const void*)woq_gemm_w4_strip_kernel<false, STRIP_WAVES, STRIP_RING>, hipFuncAttributeMaxDynamicSharedMemorySize, STRIP_SMEM_BYTES);
    inc_attr_done(strip_attr_set);
  }
  dim3 grid((unsigned)ceil_div64(a.N, 128), (unsigned)ceil_div64(a.M, 64), (unsigned)splitk);
#define INC_STRIP(BF, W, R, A)                                                                                                        \
  woq_gemm_w4_strip_kernel<BF, W, R, A><<<grid, 64 * W, W * R * 6 * 1024, a.s>>>(a.x, a.qw, a.scales, a.qz, a.bias, a.y, part, counters, (int)a.M, a.N, a.K, a.NW, a.g_shift, splitk)
#ifdef INC_KBENCH  // harness: the bf16 kernel with W waves, a ring of R slots and ablation A
#define INC_STRIP_H(W, R, A)                                                                                                          \
  { (void)hipFuncSetAttribute((const void*)woq_gemm_w4_strip_kernel<true, W, R, A>, hipFuncAttributeMaxDynamicSharedMemorySize, W * R * 6 * 1024); INC_STRIP(true, W, R, A); }
#define INC_STRIP_ABL(A) INC_STRIP_H(STRIP_WAVES, STRIP_RING, A)
  if (a.bf && dbg >= 85 && dbg <= 89) {  // timing-only ablations of the strip step
    if (dbg == 85) INC_STRIP_ABL(1) else if (dbg == 86) INC_STRIP_ABL(2) else if (dbg == 87) INC_STRIP_ABL(3) else if (dbg == 88) INC_STRIP_ABL(4) else INC_STRIP_ABL(7)
    INC_LAUNCH_RETURN();
  }
  if (a.bf && dbg >= 100 && dbg <= 102) {  // A/B with CORRECT results: 100 LDS reads one step ahead, 101 s_setprio around the compute, 102 both
    if (dbg == 100) INC_STRIP_ABL(8) else if (dbg == 101) INC_STRIP_ABL(16) else INC_STRIP_ABL(24)
    INC_LAUNCH_RETURN();
  }
  if (a.bf && dbg == 84) {  // A/B: four waves (one per SIMD) with a six-deep ring
    INC_STRIP_H(4, 6, 0)
    INC_LAUNCH_RETURN();
  }
#undef INC_STRIP_ABL
#undef INC_STRIP_H
#endif
  if (a.bf) INC_STRIP(true, STRIP_WAVES, STRIP_RING, 0);
  else INC_STRIP(false, STRIP_WAVES, STRIP_RING, 0);
#undef INC_STRIP
  INC_LAUNCH_RETURN();
}
