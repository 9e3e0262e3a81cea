// kbench_gptq_tile_lab.inc -- harness-only generations of the 256 x 256 transpose-read syrk tile (included by csrc/gptq_hessian.hip under
// INC_KBENCH).  The PRODUCT tile (csrc/gptq_hessian.hip, hessian_syrk_tr_tile) is the ABL = 176 form of this template written out
// without the switches; everything else lives here: ABL bits 0 / 1 are timing-only ablations with WRONG results (no LDS-DMA / no
// fragment reads and no MFMA), bits 2 / 3 correct A/B partners (requests spread over the step / row fragments two rows ahead), bit 4
// static priority for waves 4-7, bit 5 one rolling fragment pipeline per step, bit 7 a step's eight LDS-DMA pieces from one asm block;
// (TOK, NST) other than (64, 2) are the stage-shape A/B partners.  tools/kbench hessian / hpf select them by flag: the table and the two
// launch hooks at the end of this file, one per Hessian entry point.  `slab`: as in the product tile.
constexpr int TR_LAB_ABL = 176;
template <bool IS_BF16, int TOK, int NST, int ABL = TR_LAB_ABL>
__device__ __forceinline__ void hessian_syrk_tr_tile_lab(const uint16_t* __restrict__ x, int64_t T, int64_t K, int64_t ldx,
                                                     float* __restrict__ H, float beta, float alpha, int nt, int block, int nblocks,
                                                     float* __restrict__ slab = nullptr) {
  static_assert((NST & (NST - 1)) == 0 && NST >= 2 && NST <= 4 && TOK % 32 == 0, "stage ring");
  constexpr int D = NST - 1;        // steps the DMA runs ahead
  constexpr int RPW = TOK / 8;      // DMA requests (token rows) per wave and step
  constexpr int STAGE = TOK * TR_PITCH;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  int ti, tj;
  xcd_supertile_decode(block, nblocks, nt, ti, tj);
  const int64_t i0 = (int64_t)ti * H2, j0 = (int64_t)tj * H2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem_raw;

  // DMA source: this lane's 16-byte chunk (8 features) of the i panel (lanes 0..31) or the j panel (lanes 32..63)
  int64_t f = (lane < 32 ? i0 : j0) + 8 * (lane & 31);
  if (f > K - 8) f = K - 8;  // K % 8 == 0 on this path: a chunk past K only feeds rows / columns that are never stored
  const uint32_t voff = (uint32_t)(f * 2);
  const int nk = (int)((T + TOK - 1) / TOK);
  auto issue_one = [&](int kt, int i) {
    const int stage = kt & (NST - 1);
    const int r = wave * RPW + i;
    int64_t t = (int64_t)kt * TOK + r;
    if (t > T - 1) t = T - 1;  // rows past T are zeroed in LDS before they are multiplied (below)
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE + r * TR_PITCH);
    if constexpr ((ABL & 1) == 0) lds_dma_1k(x + t * ldx, dst, voff);
  };
  // ABL bit 7: a step whose TOK token rows all exist (every step but a ragged last one) issues its pieces from ONE asm block -- the
  // row stride sits in per-lane offsets computed once per tile, so a piece is an M0 update and the request instead of ~25 instructions
  // (a clamped 64-bit row address, M0 save / restore, wait states).  Same requests in the same order: bit-identical H.
  constexpr bool FAST_ISSUE = (ABL & 128) != 0 && RPW == 8;  // (written for eight rows per wave: the 64-token stages)
  uint32_t voffr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) voffr[i] = voff + (uint32_t)((int64_t)i * ldx * 2);
  auto issue = [&](int kt) {
    if constexpr (FAST_ISSUE && (ABL & 1) == 0) {
      if ((int64_t)(kt + 1) * TOK <= T) {
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (kt & (NST - 1)) * STAGE + wave * RPW * TR_PITCH);
        lds_dma_8x1k<TR_PITCH>(x + ((int64_t)kt * TOK + wave * RPW) * ldx, dst, voffr[0], voffr[1], voffr[2], voffr[3], voffr[4], voffr[5],
                               voffr[6], voffr[7]);
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) issue_one(kt, i);
  };
  // ABL bit 2 (harness A/B, CORRECT results): the step's RPW requests are not issued back to back at the top of the step but one
  // behind every (8 * TOK / 32 / RPW)-th row of four MFMAs -- a piece costs its wave 60-185 issue cycles (profiles/NOTES.md)
  constexpr bool SPREAD = (ABL & 4) != 0;
  constexpr int SLOTS = 8 * (TOK / 32), SLOT_EVERY = SLOTS / RPW > 0 ? SLOTS / RPW : 1;
  // step `next` has landed when at most the steps after it (up to `last_issued`) are still in this wave's queue
  auto wait_landed = [&](int next, int last_issued) {
    const int younger = last_issued - next;
    if (D >= 3 && younger >= 2) wait_vmcnt<2 * RPW>();
    else if (D >= 2 && younger >= 1) wait_vmcnt<RPW>();
    else wait_vmcnt<0>();
  };

  f32x4_t acc[8][4];  // [i fragment of 16 rows][j fragment of 16 columns]
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // fragment read address: lane (a + 4b) of 16-lane group g -> token row 4g + b (second read: 16 + 4g + b), feature block 4a
  const int s16 = lane & 15, fa = s16 & 3, fb = s16 >> 2, fg = lane >> 4;
  const uint32_t rbase = (uint32_t)((4 * fg + fb) * TR_PITCH + (wm * 128 + 4 * fa) * 2);        // + mt * 32
  const uint32_t cbase = (uint32_t)((4 * fg + fb) * TR_PITCH + 512 + (wn * 64 + 4 * fa) * 2);  // + nt * 32
  typedef __attribute__((address_space(3))) s16x4_t* lds_ptr_t;
  auto frag = [&](uint32_t byte_off) {
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr_t)(uintptr_t)(byte_off));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr_t)(uintptr_t)(byte_off + 16 * TR_PITCH));
    uint4 v;
    __builtin_memcpy(&v, &lo, 8);
    __builtin_memcpy(reinterpret_cast<char*>(&v) + 8, &hi, 8);
    return v;
  };

  // ABL bit 4: static priority for the second-dispatched half of the workgroup (the younger wave of every SIMD loses each
  // arbitration to the older one, MI355X_MICROARCH.md "Two waves per SIMD")
  if constexpr ((ABL & 16) != 0) {
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  }
  const int pro = nk < D ? nk : D;
  for (int d = 0; d < pro; ++d) issue(d);
  wait_landed(0, pro - 1);
  __builtin_amdgcn_s_barrier();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & (NST - 1);
    const bool more = kt + D < nk;
    if (!SPREAD && more) issue(kt + D);  // its stage was last read in step kt - 1 (barrier passed)
    if (kt == nk - 1 && (T % TOK) != 0) {
      // token tail: zero the rows past T of this (last) stage; its DMA has landed (counted wait + barrier of the previous step)
      const int first = (int)(T - (int64_t)kt * TOK);
      for (int idx = tid; idx < (TOK - first) * 64; idx += 512) {
        const int r = first + idx / 64, c = idx % 64;
        *reinterpret_cast<uint4*>(smem_raw + cur * STAGE + r * TR_PITCH + c * 16) = make_uint4(0u, 0u, 0u, 0u);
      }
      __syncthreads();
    }
    // ABL bit 5: ONE rolling pipeline over the step's 8 * TOK / 32 MFMA rows -- the row fragment of row r + 2 and (at row 4 of a
    // 32-token sub-step) the column fragments of the NEXT sub-step are requested before row r's MFMAs, so only the step's first six
    // fragment reads are exposed (round 4: all twelve of every sub-step in front of its first MFMA)
    if constexpr ((ABL & 32) != 0) {
      constexpr int NKK = TOK / 32, ROWS = 8 * NKK;
      const uint32_t st0 = lds0 + cur * STAGE;
      uint4 bq[2][4], aq[3];
#pragma unroll
      for (int n = 0; n < 4; ++n) bq[0][n] = frag(st0 + cbase + n * 32);
      aq[0] = frag(st0 + rbase);
      aq[1] = frag(st0 + rbase + 32);
#pragma unroll
      for (int row = 0; row < ROWS; ++row) {
        const int kk = row / 8, m = row % 8;
        if (row + 2 < ROWS) aq[(row + 2) % 3] = frag(st0 + ((row + 2) / 8) * 32 * TR_PITCH + rbase + ((row + 2) % 8) * 32);
        if (m == 4 && kk + 1 < NKK) {
#pragma unroll
          for (int n = 0; n < 4; ++n) bq[(kk + 1) & 1][n] = frag(st0 + (kk + 1) * 32 * TR_PITCH + cbase + n * 32);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          if constexpr (IS_BF16) {
            bf16x8 fa8, fb8;
            __builtin_memcpy(&fa8, &aq[row % 3], 16);
            __builtin_memcpy(&fb8, &bq[kk & 1][n], 16);
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa8, fb8, acc[m][n], 0, 0, 0);
          } else {
            f16x8 fa8, fb8;
            __builtin_memcpy(&fa8, &aq[row % 3], 16);
            __builtin_memcpy(&fb8, &bq[kk & 1][n], 16);
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa8, fb8, acc[m][n], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < ((ABL & (2 | 32)) ? 0 : TOK / 32); ++kk) {
      const uint32_t st = lds0 + cur * STAGE + kk * 32 * TR_PITCH;
      uint4 a[8], b[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) b[n] = frag(st + cbase + n * 32);
      // ABL bit 3 (harness A/B, CORRECT results): the row fragments are requested two MFMA rows ahead of their use instead of all
      // eight in front of the first MFMA (a wave then covers its own ds_read latency with its own MFMAs)
      constexpr bool ROLL = (ABL & 8) != 0;
#pragma unroll
      for (int m = 0; m < (ROLL ? 2 : 8); ++m) a[m] = frag(st + rbase + m * 32);
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        if constexpr (ROLL) {
          if (m + 2 < 8) a[m + 2] = frag(st + rbase + (m + 2) * 32);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          if constexpr (IS_BF16) {
            bf16x8 fa8, fb8;
            __builtin_memcpy(&fa8, &a[m], 16);
            __builtin_memcpy(&fb8, &b[n], 16);
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa8, fb8, acc[m][n], 0, 0, 0);
          } else {
            f16x8 fa8, fb8;
            __builtin_memcpy(&fa8, &a[m], 16);
            __builtin_memcpy(&fb8, &b[n], 16);
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa8, fb8, acc[m][n], 0, 0, 0);
          }
        }
        if constexpr (SPREAD) {
          const int slot = kk * 8 + m;
          if (slot % SLOT_EVERY == SLOT_EVERY - 1 && slot / SLOT_EVERY < RPW) {
            __builtin_amdgcn_sched_barrier(0);
            if (more) issue_one(kt + D, slot / SLOT_EVERY);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    // every fragment read of this step has returned (the compiler sinks the last MFMAs below the barrier, so this is not
    // implied by program order) and step kt + 1 has landed (younger steps stay in flight)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int last_issued = kt + D < nk ? kt + D : nk - 1;
    wait_landed(kt + 1, last_issued > kt + 1 ? last_issued : kt + 1);
    __builtin_amdgcn_s_barrier();
  }

  // epilogue: D[row i][col j] of a 16x16 fragment: col = lane & 15, row = 4 * (lane >> 4) + r
  if (slab) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          slab[(wm * 128 + m * 16 + 4 * (lane >> 4) + r) * H2 + wn * 64 + n * 16 + (lane & 15)] = acc[m][n][r];
    return;
  }
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int64_t col = j0 + wn * 64 + n * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = i0 + wm * 128 + m * 16 + 4 * (lane >> 4) + r;
        if (row < K && col < K) {
          float* p = H + row * K + col;
          *p = beta * (*p) + alpha * acc[m][n][r];
        }
      }
    }
}

template <bool IS_BF16, int TOK = TR_TOK, int NST = TR_NST, int ABL = TR_LAB_ABL>
__global__ __launch_bounds__(512) void hessian_syrk_tr_256_lab_kernel(const uint16_t* __restrict__ x, int64_t T, int64_t K, int64_t ldx,
                                                                  float* __restrict__ H, float beta, float alpha, int nt) {
  hessian_syrk_tr_tile_lab<IS_BF16, TOK, NST, ABL>(x, T, K, ldx, H, beta, alpha, nt, (int)blockIdx.x, (int)gridDim.x);
}

// the batched launch over the harness generations of the tile
template <bool IS_BF16, int TOK = TR_TOK, int NST = TR_NST, int ABL = TR_LAB_ABL>
__global__ __launch_bounds__(512) void hessian_syrk_tr_256_multi_lab_kernel(HessianBatch args, int64_t T) {
  hessian_batch_workgroup(args, T, TOK, [](auto... a) __attribute__((always_inline)) { hessian_syrk_tr_tile_lab<IS_BF16, TOK, NST, ABL>(a...); });
}

// ---- harness launches: flag -> form of the tile (bf16 only) ---------------------------------------------------------------------
struct TileLabForm { int flag, tok, nst, abl; bool batched; };  // batched: also instantiated for the batched launch
constexpr TileLabForm TILE_LAB_FORMS[] = {
    {LAB_HESSIAN_STAGES_4X32, 32, 4, TR_LAB_ABL, true},
    {LAB_HESSIAN_NO_DMA, 64, 2, 1, false},          // timing only
    {LAB_HESSIAN_NO_MFMA, 64, 2, 2, false},         // timing only
    {LAB_HESSIAN_NO_DMA_NO_MFMA, 64, 2, 3, false},  // timing only
    {LAB_HESSIAN_SPREAD, 64, 2, 4, false},
    {LAB_HESSIAN_SPREAD_4X32, 32, 4, 4, false},     // three steps in flight
    {LAB_HESSIAN_SPREAD_ROLL, 64, 2, 4 | 8, false},
    {LAB_HESSIAN_ROLL, 64, 2, 8, true},
    {LAB_HESSIAN_PRIO, 64, 2, 16, true},
    {LAB_HESSIAN_SPREAD_ROLL_PRIO, 64, 2, 4 | 8 | 16, false},
    {LAB_HESSIAN_ROLL_PRIO, 64, 2, 8 | 16, true},
    {LAB_HESSIAN_PIPELINE, 64, 2, 32, true},
    {LAB_HESSIAN_PIPELINE_PRIO, 64, 2, 32 | 16, true},
    {LAB_HESSIAN_ROUND4, 64, 2, 0, true},           // A/B partner of every switch
    {LAB_HESSIAN_PRODUCT_FORM, 64, 2, TR_LAB_ABL, true},
};
// `launch(index)`, the table index of `flag` as a compile-time constant; false when the flag selects no form here.  BATCHED: only the
// forms with `batched` set are offered, so only those multi_lab_kernel instantiations exist.
template <bool BATCHED, int I = 0, class Launch>
bool tile_lab_dispatch(int flag, Launch launch) {
  if constexpr (I < (int)(sizeof(TILE_LAB_FORMS) / sizeof(TILE_LAB_FORMS[0]))) {
    if constexpr (!BATCHED || TILE_LAB_FORMS[I].batched)
      if (flag == TILE_LAB_FORMS[I].flag) return launch(std::integral_constant<int, I>{}), true;
    return tile_lab_dispatch<BATCHED, I + 1>(flag, launch);
  }
  return false;
}

// a harness launch of 512-thread workgroups: the LDS attribute is set at every launch
template <class Kernel, class... Args>
void lab_launch(Kernel kernel, int grid, size_t smem, hipStream_t s, Args... args) {
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  kernel<<<grid, 512, smem, s>>>(args...);
}

// The hook of inc_gptq_hessian_accum on the 256 x 256 route.  Returns whether it launched.
bool hessian_lab_launch(const uint16_t* xp, int xdtype, int64_t T, int64_t K, int64_t ldx, float* H, float beta, float alpha, int nt2,
                        int ntiles2, hipStream_t s) {
  const int flag = inc_small_tiles_flag(-1);
  if (flag == LAB_HESSIAN_REG_TRANSPOSE) {
    hessian_256_dispatch(xdtype, T, [&](auto bf16, auto tail) {
      lab_launch(hessian_syrk_16bit_256_kernel<bf16.value, tail.value>, ntiles2, H2_SMEM, s, xp, T, K, ldx, H, beta, alpha, nt2);
    });
    return true;
  }
  if (xdtype != INC_BF16) return false;
  return tile_lab_dispatch<false>(flag, [&](auto i) {
    constexpr TileLabForm F = TILE_LAB_FORMS[i.value];
    lab_launch(hessian_syrk_tr_256_lab_kernel<true, F.tok, F.nst, F.abl>, ntiles2, (size_t)TR_NST * TR_STAGE, s, xp, T, K, ldx, H, beta, alpha, nt2);
  });
}

// The hook of inc_gptq_hessian_accum_multi, after the batch is filled.  Returns whether it launched; LAB_HESSIAN_NO_TAIL_SPLIT only
// undoes the split and leaves the launch to the product.
bool hessian_batch_lab_launch(HessianBatch& a, int xdtype, int64_t T, int cus, hipStream_t s) {
  const int flag = inc_small_tiles_flag(-1), tiles = a.first[a.n];
  const size_t smem3 = (size_t)TR_NST * TR_STAGE;
  auto unsplit = [&] { a.full = tiles; a.nseg = 1; a.slab = nullptr; };
  auto grid = [&] { return a.full + (tiles - a.full) * a.nseg; };
  if (flag == LAB_HESSIAN_NO_TAIL_SPLIT) { unsplit(); return false; }
  if (flag == LAB_HESSIAN_REG_TRANSPOSE) {
    unsplit();
    hessian_256_dispatch(xdtype, T, [&](auto bf16, auto tail) {
      lab_launch(hessian_syrk_16bit_256_multi_kernel<bf16.value, tail.value>, tiles, H2_SMEM, s, a, T);
    });
    return true;
  }
  if (flag == LAB_HESSIAN_ROUND_LAUNCHES) {  // the product kernel, one launch per round of one-tile-per-CU
    const int chunk = (cus <= 0 || (cus % 8) != 0) ? 256 : cus;
    for (int b0 = 0; b0 < grid(); b0 += chunk) {
      a.block0 = b0;
      const int g = std::min(grid() - b0, chunk);
      if (xdtype == INC_BF16) lab_launch(hessian_syrk_tr_256_multi_kernel<true>, g, smem3, s, a, T);
      else lab_launch(hessian_syrk_tr_256_multi_kernel<false>, g, smem3, s, a, T);
    }
    hessian_tail_finalize(a, s);
    return true;
  }
  if (xdtype != INC_BF16) return false;
  return tile_lab_dispatch<true>(flag, [&](auto i) {
    constexpr TileLabForm F = TILE_LAB_FORMS[i.value];
    if (F.tok != TR_TOK) unsplit();  // the split's token ranges are whole 64-token steps
    lab_launch(hessian_syrk_tr_256_multi_lab_kernel<true, F.tok, F.nst, F.abl>, grid(), smem3, s, a, T);
    hessian_tail_finalize(a, s);
  });
}
