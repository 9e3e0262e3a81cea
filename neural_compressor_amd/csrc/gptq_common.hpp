// gptq_common.hpp -- what the GPTQ calibration translation units share: the column loop's block constants and guards (gptq.hip,
// gptq_lazy.hip) and the names of the harness flags of the GPTQ kernel families (those two, gptq_hessian.hip, chol.hip, tools/kbench).
#pragma once
#include <hip/hip_runtime.h>

constexpr int QB = 128;   // columns per block of the column loop
constexpr int L2T = 128;  // rows / columns of a lazy-update tile

// third / fourth generation of the lazy update over the columns [c_begin, c_end) of the trailing matrix: gptq_lazy.hip
void inc_launch_lazy_update_v3(float* w, const float* Hinv, const float* err, int64_t N, int64_t K, int64_t i1, int64_t c_begin,
                               int64_t c_end, bool exclusive, hipStream_t s);

// A full 128-column block whose kernels may use 32-bit byte offsets into Hinv / W rows (K * (QB + 1) * 4 < 2^32) and 16-byte
// accesses (K % 4).  The quantisation chain starts on the 128-column grid; the trailing update only needs an aligned first row.
static inline bool block_range_ok(int64_t K, int count) { return count == QB && (K % 4) == 0 && K * (int64_t)(QB + 1) * 4 < ((int64_t)1 << 32); }
static inline bool chain_block_ok(int64_t K, int64_t i1, int count) { return (i1 % QB) == 0 && block_range_ok(K, count); }
static inline bool lazy_block_ok(int64_t K, int64_t i1, int count) { return (i1 % 4) == 0 && block_range_ok(K, count); }

// groups of one (scale, zero) per 128-column block that the quad-per-row chain kernel handles: 1 / 2 / 4, or 0 (none).
// `allow_ungrouped`: per-row tables (group_size <= 0) and groups of whole blocks count as one group per block.
static inline int groups_per_block(int group_size, bool allow_ungrouped) {
  if (allow_ungrouped ? (group_size <= 0 || (group_size % QB) == 0) : group_size == QB) return 1;
  return group_size == 64 ? 2 : group_size == 32 ? 4 : 0;
}

// Harness flags of the GPTQ kernel families (inc_small_tiles_flag, common.hpp): what tools/kbench sets to reach another generation of
// a kernel or a timing-only ablation.  They mean something in the harness build only; the product reads the constant 0.
enum IncGptqLabFlag {
  LAB_HESSIAN_ROUND_LAUNCHES = 43,   // batched Hessian launch: one launch per round of one-tile-per-CU
  LAB_HESSIAN_NO_TAIL_SPLIT = 44,    // batched Hessian launch: every tile of the last round is one workgroup
  // generations of the 256 x 256 Hessian tile
  LAB_HESSIAN_REG_TRANSPOSE = 45,    // operands transposed in registers (first generation)
  LAB_HESSIAN_STAGES_4X32 = 46,      // four 32-token stages
  LAB_HESSIAN_NO_DMA = 47,           // timing only, WRONG results: no LDS-DMA
  LAB_HESSIAN_NO_MFMA = 48,          // timing only: no fragment reads, no MFMA
  LAB_HESSIAN_NO_DMA_NO_MFMA = 49,   // timing only: barriers + epilogue
  LAB_HESSIAN_SPREAD = 50,           // DMA requests spread over the step's MFMA rows
  LAB_HESSIAN_SPREAD_4X32 = 51,      // that with four 32-token stages
  LAB_HESSIAN_SPREAD_ROLL = 52,      // spread + row fragments two rows ahead
  LAB_HESSIAN_ROLL = 53,             // row fragments two rows ahead
  LAB_HESSIAN_PRIO = 54,             // static priority for waves 4-7
  LAB_HESSIAN_SPREAD_ROLL_PRIO = 55,
  LAB_HESSIAN_ROLL_PRIO = 56,
  LAB_HESSIAN_PIPELINE = 57,         // one rolling fragment pipeline per step
  LAB_HESSIAN_PIPELINE_PRIO = 58,
  LAB_HESSIAN_ROUND4 = 59,           // the round-4 form of the tile (no switch set)
  LAB_HESSIAN_PRODUCT_FORM = 60,     // the template's instantiation of the product tile
  // lazy (trailing) update of the column loop
  LAB_LAZY_V2 = 86,                  // second generation
  LAB_LAZY_NO_MFMA = 87,             // timing only, third generation: no MFMAs
  LAB_LAZY_NO_LOADS = 88,            // timing only: no loads / LDS-DMA
  LAB_LAZY_NO_STORES = 90,           // timing only: no stores
  LAB_LAZY_X3 = 106,                 // split (bf16 x 3) products: an experiment
  LAB_LAZY_V3_ONLY = 107,            // third generation everywhere (no strip form)
  LAB_LAZY_STRIP_CAP_4 = 108,        // short strips everywhere, at most 4 tiles
  LAB_LAZY_STRIP_CAP_16 = 109,       // short strips everywhere, at most 16 tiles
  LAB_LAZY_SHORT_STRIPS = 110,       // short strips everywhere (never one round of long ones)
  LAB_CHOL_DIAG_V1 = 201,            // inverse Cholesky factor: first generation of the diagonal-block kernel
};
