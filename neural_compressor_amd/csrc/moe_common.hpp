// moe_common.hpp -- what the routed MoE kernels share: the layout of the route buffer inc_moe_route writes (gemm_moe.hip) and the
// routing-weight load.  Readers: the INT4 grouped GEMM and combine (gemm_moe.hip) and the MX / FP8 grouped GEMM (gemm_strip_moe.hip).
#pragma once
#include "common.hpp"

constexpr int MOE_BM = 64;  // rows (slots) per tile
constexpr int MOE_MAX_E = 512;
constexpr int64_t MOE_MAX_SLOTS = 1 << 22;

// int32 offsets inside the route buffer
struct RouteLayout {
  int64_t offsets, order, pos, tiles, total;
};
__host__ __device__ inline int64_t moe_tiles_max(int64_t S, int64_t E) { return (S + MOE_BM - 1) / MOE_BM + (E < S ? E : S); }
__host__ __device__ inline RouteLayout moe_route_layout(int64_t S, int64_t E) {
  RouteLayout L;
  L.offsets = 1;  // [0] = number of tiles
  L.order = L.offsets + E + 1;
  L.pos = L.order + S;
  L.tiles = L.pos + S;
  L.total = L.tiles + 2 * moe_tiles_max(S, E);
  return L;
}

__device__ __forceinline__ float moe_load_weight(const void* p, int64_t i, int dt) {
  if (dt == INC_F32) return static_cast<const float*>(p)[i];
  const uint16_t b = static_cast<const uint16_t*>(p)[i];
  return dt == INC_F16 ? f16_bits_to_f32(b) : bf16_bits_to_f32(b);
}
