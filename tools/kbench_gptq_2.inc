// kbench_gptq_2.inc -- HARNESS ONLY (included by csrc/gptq.hip under INC_KBENCH, inside its anonymous namespace):
// the second generation of the lazy update and the hook through which the harness flags reach it and the split-product experiment.
// ---------------------------------------------------------------------------------------------
// lazy update, second generation: W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:] with Err1 held in registers
// ---------------------------------------------------------------------------------------------
// 256 threads = 4 waves, each wave owns 32 rows of a 128-row panel and keeps its whole 32 x 128 slice of
// Err1 as MFMA A-operands in 64 VGPRs for the lifetime of the workgroup.  The workgroup walks over the
// 128-column tiles assigned to it (tile = chunk, chunk + nchunks, ...): the [128 k][128 col] fp32 tile of
// Hinv arrives by LDS-DMA into one of two 64 KiB LDS buffers while the previous tile is being multiplied
// (exact fp32 v_mfma_f32_32x32x2_f32: 256 per wave per tile), the W tile is fetched into registers at the
// start of the tile and written back as W - acc at its end (same "sum, then subtract" order as before).
template <bool UNUSED>
__global__ __launch_bounds__(256) void gptq_lazy_update_v2_kernel(float* __restrict__ w, const float* __restrict__ Hinv,
                                                                  const float* __restrict__ err, int64_t N, int64_t K,
                                                                  int64_t i1, int64_t i2, int nchunks, int ncol_tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chunk = blockIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * L2T + wave * 32;  // first row of this wave

  // Err1 slice -> registers: a[s] = Err1[r0 + (lane&31)][2s + (lane>>5)]
  float a[64];
  {
    int64_t row = r0 + (lane & 31);
    if (row > N - 1) row = N - 1;
    const float* ep = err + row * QB + (lane >> 5);
#pragma unroll
    for (int s = 0; s < 64; ++s) a[s] = ep[2 * s];
  }
  // DMA source offsets (bytes from Hinv + i1*K + c0): instruction j of this wave moves tile rows
  // (wave*16 + j)*2 + (lane>>5), 16-byte chunk lane&31
  const uint32_t rowoff = (uint32_t)(((wave * 32 + (lane >> 5)) * K) * 4);
  const float* const hbase = Hinv + i1 * K;
  auto dma_tile = [&](int ct, int buf) {
    const int64_t c0 = i2 + (int64_t)ct * L2T;
    int64_t col = c0 + 4 * (lane & 31);
    if (col > K - 4) col = K - 4;  // partial last tile: clamped columns are never stored
    const uint32_t v = rowoff + (uint32_t)(col * 4);
    const uint32_t step = (uint32_t)(2 * K * 4);
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + buf * (L2T * L2T * 4) + wave * 16384);
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4)
      lds_dma_4x1k(hbase, dst + q4 * 4096, v + (4 * q4) * step, v + (4 * q4 + 1) * step, v + (4 * q4 + 2) * step,
                   v + (4 * q4 + 3) * step);
  };

  int ct = chunk;
  if (ct >= ncol_tiles) return;
  dma_tile(ct, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0;
  for (; ct < ncol_tiles; ct += nchunks, cur ^= 1) {
    const int64_t c0 = i2 + (int64_t)ct * L2T;
    if (ct + nchunks < ncol_tiles) dma_tile(ct + nchunks, cur ^ 1);
    // W tile -> registers (D layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5))
    float wt[4][16];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      int64_t col = c0 + nf * 32 + (lane & 31);
      if (col > K - 1) col = K - 1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int64_t row = r0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row > N - 1) row = N - 1;
        wt[nf][r] = w[row * K + col];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nf][r] = 0.f;
    const float* hs = reinterpret_cast<const float*>(smem_raw + cur * (L2T * L2T * 4)) + (lane >> 5) * L2T + (lane & 31);
    // B operands are read from LDS one batch (8 k-steps x 4 column fragments) AHEAD of the MFMAs that use them:
    // with one wave per SIMD nothing else hides the LDS latency (hipcc alone reads each pair just in time)
    float bA[32], bB[32];
    auto load_batch = [&](int g, float (&b)[32]) {
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) b[s8 * 4 + nf] = hs[(2 * (8 * g + s8)) * L2T + nf * 32];
    };
    auto mma_batch = [&](int g, const float (&b)[32]) {
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          acc[nf] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[8 * g + s8], b[s8 * 4 + nf], acc[nf], 0, 0, 0);
    };
    load_batch(0, bA);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      load_batch(2 * p + 1, bB);
      __builtin_amdgcn_sched_barrier(0);
      mma_batch(2 * p, bA);
      if (p < 3) load_batch(2 * p + 2, bA);
      __builtin_amdgcn_sched_barrier(0);
      mma_batch(2 * p + 1, bB);
    }
    if (r0 + 32 <= N && c0 + L2T <= K) {  // wave-uniform: interior tile, unguarded stores
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        float* wp = w + (r0 + 4 * (lane >> 5)) * K + c0 + nf * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) wp[((r & 3) + 8 * (r >> 2)) * K] = wt[nf][r] - acc[nf][r];
      }
    } else {
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const int64_t col = c0 + nf * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = r0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (row < N && col < K) w[row * K + col] = wt[nf][r] - acc[nf][r];
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// The hook of lazy_update_range (csrc/gptq.hip).  Returns whether it launched.
bool launch_lazy_update_x3(float* w, const float* err, int64_t N, int64_t K, int64_t i1, int64_t c_begin, int64_t c_end, hipStream_t s);  // kbench_gptq_3.inc
bool lazy_update_lab_launch(float* w, const float* Hinv, const float* err, int64_t N, int64_t K, int64_t i1, int64_t c_begin, int64_t c_end,
                            bool exclusive, hipStream_t s) {
  const int flag = inc_small_tiles_flag(-1);
  // (the experiment covers the look-ahead loop's column-range calls only)
  if (flag == LAB_LAZY_X3 && !exclusive) return launch_lazy_update_x3(w, err, N, K, i1, c_begin, c_end, s);
  if (flag != LAB_LAZY_V2) return false;
  const int ncol_tiles = (int)ceil_div64(c_end - c_begin, L2T);
  const int row_tiles = (int)ceil_div64(N, L2T);
  const int nchunks = std::min((int)ceil_div64(512, row_tiles), ncol_tiles);  // ~512 workgroups when the trailing matrix is wide enough
  const size_t smem2 = (size_t)2 * L2T * L2T * 4;  // 128 KiB
  (void)hipFuncSetAttribute((const void*)gptq_lazy_update_v2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem2);
  gptq_lazy_update_v2_kernel<true><<<dim3((unsigned)nchunks, (unsigned)row_tiles), 256, smem2, s>>>(w, Hinv, err, N, K, i1, c_begin, nchunks,
                                                                                                 ncol_tiles);
  return true;
}
