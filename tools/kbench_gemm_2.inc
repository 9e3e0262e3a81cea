// harness-only code of gemm_tile256.hip, which includes it in place (tools/libinc_mi355x_kbench.so, -DINC_KBENCH; NOT part of libinc_mi355x.so):
// the launcher of the producer / consumer specialisation of the 3A2B tile (one scale per column and K-step: group_size >= 64)
int inc_launch_woq_gemm_pc(const WoqGemmArgs& a, int y_vec_ok, float* part, int steps, int splits, int dbg) {
  const size_t smem = (size_t)3 * T_ASTAGE + 2 * T_BSTAGE;  // 160 KiB: the whole LDS of a CU
  static std::atomic<uint64_t> pc_attr_set{0};
  if (inc_attr_needed(pc_attr_set)) {
    (void)hipFuncSetAttribute((const void*)woq_gemm_w4_pc_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    (void)hipFuncSetAttribute((const void*)woq_gemm_w4_pc_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    inc_attr_done(pc_attr_set);
  }
  const unsigned grid = (unsigned)(ceil_div64(a.M, TM) * ceil_div64(a.N, TN));
  // woq_gemm_plan: y_vec_ok bit 0: 8-byte stores possible; bit 1: 16-byte stores possible (full tiles then leave through LDS)
  dim3 g2(grid, (unsigned)splits);
#define INC_PC(B, A) woq_gemm_w4_pc_kernel<B, A><<<g2, PC_THREADS, smem, a.s>>>(a.x, a.qw, a.scales, a.qz, a.bias, a.y, a.M, a.N, a.K, a.NW, a.g_shift, y_vec_ok, part, steps)
  if (!a.bf) INC_PC(false, 0);
  // timing-only ablations of the producer / consumer step (tools/kbench pcablate)
#define INC_PC_ABL(A) { INC_ALLOW_PC(A); INC_PC(true, A); }
#define INC_ALLOW_PC(A) (void)hipFuncSetAttribute((const void*)woq_gemm_w4_pc_kernel<true, A>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)
  else if (dbg == 51) INC_PC_ABL(1)
  else if (dbg == 52) INC_PC_ABL(3)
  else if (dbg == 53) INC_PC_ABL(4)
  else if (dbg == 54) INC_PC_ABL(8)
  else if (dbg == 55) INC_PC_ABL(12)
  else if (dbg == 56) INC_PC_ABL(15)
  else if (dbg == 57) INC_PC_ABL(16)
  else if (dbg == 58) INC_PC_ABL(31)
  else if (dbg == 59) INC_PC_ABL(95)
  else if (dbg == 60) INC_PC_ABL(32)
  else if (dbg == 61) INC_PC_ABL(64)
  else if (dbg == 62) INC_PC_ABL(48)       // producers alone (consumers neither read nor multiply)
  else if (dbg == 63) INC_PC_ABL(49)
  else if (dbg == 64) INC_PC_ABL(51)
  else if (dbg == 65) INC_PC_ABL(52)
  else if (dbg == 66) INC_PC_ABL(56)
  else if (dbg == 67) INC_PC_ABL(60)
  else if (dbg == 68) INC_PC_ABL(63)
  else if (dbg == 69) INC_PC_ABL(128)      // no epilogue stores
  else if (dbg == 70) INC_PC_ABL(256)      // consumers at raised priority
  else if (dbg == 71) INC_PC_ABL(512)      // producers at raised priority
  else if (dbg == 72) INC_PC_ABL(128 + 63) // nothing but prologue + barriers
  else if (dbg == 73) INC_PC_ABL(1024)     // correct results: v_pk_fma_f32 in the dequantisation (the first generation)
  else if (dbg == 74) INC_PC_ABL(2048)     // correct results: single v_cvt_f32_fp8 conversions
#undef INC_PC_ABL
#undef INC_ALLOW_PC
  else INC_PC(true, 0);
#undef INC_PC
  if (part) return inc_launch_slab_reduce(a, part, splits);
  INC_LAUNCH_RETURN();
}
