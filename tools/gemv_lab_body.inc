// generated from csrc/gemm_stream.hip (then part of gemm.hip; profiles/NOTES.md round 6): woq_gemv_w4_body with timing-only ablation hooks (GL_ABL)
template <bool IS_BF16, bool G128, int VSTEPS, int MB, bool NT = false>
__device__ __forceinline__ void woq_gemv_w4_body(
    const uint16_t* __restrict__ x, const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
    const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
    float* __restrict__ partial, unsigned* __restrict__ counter, int M, int64_t N, int64_t K, int64_t NW,
    int g_shift, int splitk, int strip, int slice) {
  constexpr int VS = VSTEPS;  // shadows the file-level maximum inside this kernel
  constexpr int ROWS = 16 * MB;
  constexpr int NOUT = ROWS * 64 / 256;  // outputs per thread of the strip
  __shared__ float red[4 * ROWS * 65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_u = fp8_unit_inverse();
  const int jn = lane & 15, oct = lane >> 4;
  const int64_t n0 = (int64_t)strip * 64;
  int64_t ncol = n0 + 4 * jn;
  if (ncol > N - 4) ncol = N - 4;  // clamped lanes recompute valid columns; their results are not stored
  const int steps_total = (int)(K / 32);
  const int step0 = (slice * 4 + wave) * VS;

  // ---- issue every load of this wave up front ---------------------------------------------------
  uint4 w[VS], a[MB][VS];
#pragma unroll
  for (int s = 0; s < VS; ++s) {
    int st = step0 + s;
    if (st > steps_total - 1) st = steps_total - 1;  // past-the-end steps re-read the last one and are zeroed via A
    if constexpr (NT) {
      typedef uint32_t nt_u32x4 __attribute__((ext_vector_type(4)));
      const nt_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u32x4*>(qweight + ((int64_t)st * 4 + oct) * N + ncol));
      w[s] = make_uint4(v.x, v.y, v.z, v.w);
    } else {
      w[s] = *reinterpret_cast<const uint4*>(qweight + ((int64_t)((GL_ABL & 4) ? 0 : st) * 4 + oct) * N + ncol);
    }
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const int am = 16 * b + jn < M ? 16 * b + jn : M - 1;  // A row (clamped; rows >= M are zeroed below)
      a[b][s] = *reinterpret_cast<const uint4*>(x + (int64_t)am * K + (int64_t)st * 32 + 8 * oct);
    }
  }
  // group parameters: G128 -> one group per 4 steps (step0 is a multiple of 4)
  constexpr int NG = G128 ? (VS + 3) / 4 : VS;
  uint2 sraw[NG];
  uint32_t zraw[NG];
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    int st = step0 + (G128 ? 4 * i : i);
    if (st > steps_total - 1) st = steps_total - 1;
    const int64_t g = g_shift >= 0 ? (((int64_t)st * 32) >> g_shift) : 0;
    sraw[i] = *reinterpret_cast<const uint2*>(scales + g * N + ncol);
    zraw[i] = qzeros[g * NW + (ncol >> 3)];
  }
  const int zsh = 4 * (int)(ncol & 7);  // ncol % 4 == 0: the 4 zero nibbles sit at bits zsh .. zsh+15
  // this thread's outputs of the strip: idx = tid + 256*i -> row idx>>6, column idx&63; bias fetched now
  uint16_t braw[NOUT];
  const uint16_t* const bsrc = bias ? bias : scales;  // always a valid address: the loads stay unconditional
  bool out_ok[NOUT];
  int64_t out_off[NOUT];
#pragma unroll
  for (int i = 0; i < NOUT; ++i) {
    const int idx = tid + 256 * i, m = idx >> 6, c = idx & 63;
    out_ok[i] = m < M && n0 + c < N;
    out_off[i] = out_ok[i] ? (int64_t)m * N + n0 + c : 0;
    braw[i] = bsrc[out_ok[i] ? n0 + c : 0];
  }
  __builtin_amdgcn_sched_barrier(0);  // everything above is in flight before the first use below

  f32x4 acc[MB][4];
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[b][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < VS; ++s) {
    const int gi = G128 ? (s >> 2) : s;
    const bool in_k = step0 + s < steps_total;
    uint4 av[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const bool live = in_k && (16 * b + jn < M);
      av[b] = a[b][s];
      av[b].x = live ? av[b].x : 0u; av[b].y = live ? av[b].y : 0u; av[b].z = live ? av[b].z : 0u; av[b].w = live ? av[b].w : 0u;
    }
    const uint32_t sw[2] = {sraw[gi].x, sraw[gi].y};
    const uint32_t ww[4] = {w[s].x, w[s].y, w[s].z, w[s].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float sc = f16_bits_to_f32((uint16_t)(sw[c >> 1] >> (16 * (c & 1))));
      uint32_t zz = ((zraw[gi] >> (zsh + 4 * c)) & 15u) + 1u;
      zz = zz > 15u ? 0u : zz;
      if constexpr ((GL_ABL & 1) == 0) {
        const uint4 bq = dequant8<IS_BF16, GL_FORM>(ww[c], sc * inv_u, -(float)zz * sc);
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[b][c] = mfma16<IS_BF16>(av[b], bq, acc[b][c]);
      } else {
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[b][c][0] += __uint_as_float((ww[c] & 0xffu) | 0x3f800000u) * sc + __uint_as_float(av[b].x | 0x3f800000u);
      }
    }
  }
  // ---- reduce the 4 waves: D col = lane&15 -> column 4*jn + c, row m = 16*b + 4*oct + r ------------------
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * ROWS + 16 * b + 4 * oct + r) * 65 + 4 * jn + c] = acc[b][c][r];
  __syncthreads();
  float sum[NOUT];
#pragma unroll
  for (int i = 0; i < NOUT; ++i) {
    const int idx = tid + 256 * i, m = idx >> 6, c = idx & 63;
    sum[i] = red[(0 * ROWS + m) * 65 + c] + red[(1 * ROWS + m) * 65 + c] + red[(2 * ROWS + m) * 65 + c] + red[(3 * ROWS + m) * 65 + c];
  }
  if (splitk > 1 && (GL_ABL & 2) == 0) {
    const int64_t slab = (int64_t)M * N;
#pragma unroll
    for (int i = 0; i < NOUT; ++i)
      if (out_ok[i]) __hip_atomic_store(&partial[(int64_t)slice * slab + out_off[i]], sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
    // publish: every wave drains its write-through stores, then one relaxed agent-scope ticket from lane 0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = ticket == (unsigned)(splitk - 1);
      if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next call
      red[0] = last ? 1.f : 0.f;
    }
    __syncthreads();
    if (red[0] == 0.f) return;
    // last arriver: fixed-order sum over the slices, up to 32 partial loads of this thread in flight at a time
#pragma unroll
    for (int i = 0; i < NOUT; ++i) sum[i] = 0.f;
    constexpr int SB = 32 / NOUT;  // slices per batch (8 for M <= 16: one L2 round trip for up to 8 slices)
    for (int sl0 = 0; sl0 < splitk; sl0 += SB) {
      float pv[SB][NOUT];
#pragma unroll
      for (int d = 0; d < SB; ++d) {
        const int sl = sl0 + d < splitk ? sl0 + d : splitk - 1;
#pragma unroll
        for (int i = 0; i < NOUT; ++i) pv[d][i] = __hip_atomic_load(&partial[(int64_t)sl * slab + out_off[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1
      }
#pragma unroll
      for (int d = 0; d < SB; ++d)
#pragma unroll
        for (int i = 0; i < NOUT; ++i) sum[i] += (sl0 + d < splitk) ? pv[d][i] : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < NOUT; ++i)
    if (out_ok[i]) {
      const float v = sum[i] + (bias ? cvt16<IS_BF16>(braw[i]) : 0.f);
      y[out_off[i]] = IS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
    }
}

