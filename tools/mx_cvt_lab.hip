// mx_cvt_lab.hip -- pins v_cvt_scalef32_pk_bf16_fp4 / v_cvt_scalef32_pk_bf16_fp8 on the device: which codes a selector converts and
// what comes out for every code and scale.  Stand-alone (`make -C tools mx_cvt_lab && tools/mx_cvt_lab`); the output is kept in
// profiles/mx/mx_cvt_lab.log, the findings in DESIGN section 8b.  gemm_mx_wo.hip is written against this log.
//
// One launch per instruction: thread (code, selector, scale index) converts one source word with the scale as_float(byte << 23), for
// the scale bytes 0, 1, 16, 126, 127, 128, 240, 254.  Two source words per thread:
//   position  every nibble / byte holds a DIFFERENT code (fp4: nibble i = code (c + i) & 15; fp8: byte i = code (c + 37 i) & 255), so
//             the two results name the positions the selector reads (at scale byte 127, where every value is exact);
//   value     the code in every position: both results must be value(code) * 2^(byte - 127) bit for bit wherever that is a normal
//             bf16 number (every such product is exact in bf16: 1 or 3 mantissa bits against 7, the exponent range of fp32).
// Below the normal range and for the e4m3 NaN codes 0x7f / 0xff the lab prints what the instruction returns.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

static const int SCALE_BYTES[8] = {0, 1, 16, 126, 127, 128, 240, 254};

__device__ __forceinline__ uint32_t bits_of(bf16x2 v) {
  uint32_t r;
  __builtin_memcpy(&r, &v, 4);
  return r;
}

// out[2 * t] = the position word's result, out[2 * t + 1] = the value word's; t = (code * NSEL + sel) * 8 + scale index
template <bool FP4>
__global__ void convert_all(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ val, const int* __restrict__ sbytes,
                            uint32_t* __restrict__ out) {
  constexpr int NSEL = FP4 ? 4 : 2;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (FP4 ? 16 : 256) * NSEL * 8) return;
  const int code = t / (NSEL * 8), sel = (t / 8) % NSEL;
  const float scale = __uint_as_float((uint32_t)sbytes[t % 8] << 23);
  const uint32_t p = pos[code], v = val[code];
  uint32_t rp = 0, rv = 0;
  if constexpr (FP4) {
    if (sel == 0) { rp = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, scale, 0)); rv = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 0)); }
    if (sel == 1) { rp = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, scale, 1)); rv = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 1)); }
    if (sel == 2) { rp = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, scale, 2)); rv = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 2)); }
    if (sel == 3) { rp = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, scale, 3)); rv = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 3)); }
  } else {
    if (sel == 0) { rp = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(p, scale, false)); rv = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, scale, false)); }
    if (sel == 1) { rp = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(p, scale, true)); rv = bits_of(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, scale, true)); }
  }
  out[2 * t] = rp;
  out[2 * t + 1] = rv;
}

static double value_of(int code, bool fp4) {
  const int sign = fp4 ? 8 : 0x80, mb = fp4 ? 1 : 3, emin = fp4 ? 0 : -6, bias = fp4 ? 1 : 7;
  const int mag = code & (sign - 1), e = mag >> mb, m = mag & ((1 << mb) - 1);
  const double v = e == 0 ? ldexp((double)m, emin - mb) : ldexp(1.0 + (double)m / (1 << mb), e - bias);
  return code & sign ? -v : v;
}

static double bf16_value(uint32_t h) {
  const uint32_t u = (h & 0xffffu) << 16;
  float f;
  memcpy(&f, &u, 4);
  return (double)f;
}

// the code whose value at scale byte 127 is the bf16 `h` (sign of zero included), -1 for none
static int code_of_result(uint32_t h, bool fp4) {
  for (int c = 0; c < (fp4 ? 16 : 256); ++c) {
    if (!fp4 && (c & 0x7f) == 0x7f) continue;
    const double v = value_of(c, fp4);
    if (bf16_value(h) == v && (bool)(h & 0x8000u) == (bool)signbit(v)) return c;
  }
  return -1;
}

template <bool FP4>
static int run(const char* name) {
  constexpr int NC = FP4 ? 16 : 256, NSEL = FP4 ? 4 : 2, NPOS = FP4 ? 8 : 4, TOTAL = NC * NSEL * 8;
  static uint32_t pos[NC], val[NC], out[2 * TOTAL];
  for (int c = 0; c < NC; ++c) {
    pos[c] = val[c] = 0;
    for (int i = 0; i < NPOS; ++i) {
      int pc = FP4 ? (c + i) & 15 : (c + 37 * i) & 255;
      if (!FP4 && (pc & 0x7f) == 0x7f) pc ^= 1;  // no NaN code in a position word
      pos[c] |= (uint32_t)pc << ((FP4 ? 4 : 8) * i);
      val[c] |= (uint32_t)c << ((FP4 ? 4 : 8) * i);
    }
  }
  uint32_t *dp, *dv, *dout;
  int* ds;
  hipMalloc(&dp, sizeof pos); hipMalloc(&dv, sizeof val); hipMalloc(&dout, sizeof out); hipMalloc(&ds, sizeof SCALE_BYTES);
  hipMemcpy(dp, pos, sizeof pos, hipMemcpyHostToDevice);
  hipMemcpy(dv, val, sizeof val, hipMemcpyHostToDevice);
  hipMemcpy(ds, SCALE_BYTES, sizeof SCALE_BYTES, hipMemcpyHostToDevice);
  hipMemset(dout, 0xff, sizeof out);
  convert_all<FP4><<<(TOTAL + 255) / 256, 256>>>(dp, dv, ds, dout);
  if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); return -1; }
  hipMemcpy(out, dout, sizeof out, hipMemcpyDeviceToHost);

  int failures = 0;
  // ---- positions: at scale byte 127 (index 4) the results name their source positions --------------------------------------------
  for (int sel = 0; sel < NSEL; ++sel) {
    int lo_pos = -2, hi_pos = -2;  // -2 unset, -1 inconsistent
    for (int c = 0; c < NC; ++c) {
      const uint32_t r = out[2 * ((c * NSEL + sel) * 8 + 4)];
      const int got[2] = {code_of_result(r & 0xffffu, FP4), code_of_result(r >> 16, FP4)};
      for (int h = 0; h < 2; ++h) {
        int where = -1;
        for (int i = 0; i < NPOS; ++i)
          if ((int)((pos[c] >> ((FP4 ? 4 : 8) * i)) & (FP4 ? 15 : 255)) == got[h]) where = i;
        int& slot = h ? hi_pos : lo_pos;
        slot = slot == -2 ? where : (slot == where ? slot : -1);
      }
    }
    const bool ok = lo_pos == 2 * sel && hi_pos == 2 * sel + 1;
    printf("%s selector %d: result.lo converts %s %d, result.hi %s %d  %s\n", name, sel, FP4 ? "nibble" : "byte", lo_pos,
           FP4 ? "nibble" : "byte", hi_pos, ok ? "ok (positions 2 sel, 2 sel + 1)" : "DIFFERS from (2 sel, 2 sel + 1)");
    failures += !ok;
  }
  // ---- values: every code x selector x scale byte ----------------------------------------------------------------------------------
  for (int si = 0; si < 8; ++si) {
    const int sb = SCALE_BYTES[si];
    int normal = 0, normal_bad = 0, zero = 0, zero_bad = 0, below = 0, below_exact = 0, below_rounded = 0, below_flushed = 0, below_other = 0;
    int above = 0, above_inf = 0, above_other = 0;
    const double bf16_max = ldexp(2.0 - ldexp(1.0, -7), 127);
    for (int c = 0; c < NC; ++c) {
      if (!FP4 && (c & 0x7f) == 0x7f) continue;
      const double want = ldexp(value_of(c, FP4), sb - 127);
      for (int sel = 0; sel < NSEL; ++sel) {
        const uint32_t r = out[2 * ((c * NSEL + sel) * 8 + si) + 1];
        for (int h = 0; h < 2; ++h) {
          const uint32_t b = h ? r >> 16 : r & 0xffffu;
          const bool same = bf16_value(b) == want && (bool)(b & 0x8000u) == (bool)signbit(want);
          if (want == 0) { ++zero; zero_bad += !same; }
          else if (fabs(want) > bf16_max) { ++above; const bool inf = (b & 0x7fffu) == 0x7f80u; above_inf += inf; above_other += !inf; }
          else if (fabs(want) >= ldexp(1.0, -126)) { ++normal; normal_bad += !same; }
          else {  // a bf16 subnormal is a multiple of 2^-133
            ++below;
            const bool fl = (b & 0x7fffu) == 0, rne = bf16_value(b) == ldexp(nearbyint(ldexp(want, 133)), -133);
            below_exact += same; below_flushed += !same && fl; below_rounded += !same && !fl && rne; below_other += !same && !fl && !rne;
          }
        }
      }
    }
    printf("%s scale byte %3d: normal results %5d, %d differ; zero codes %4d, %d differ; below 2^-126: %4d (exact %d, rounded to the nearest "
           "subnormal %d, flushed to zero %d, other %d); above bf16's range: %4d (+-inf %d, other %d)  %s\n", name, sb, normal, normal_bad,
           zero, zero_bad, below, below_exact, below_rounded, below_flushed, below_other, above, above_inf, above_other,
           normal_bad || zero_bad ? "DIFFERS" : "ok");
    failures += normal_bad != 0 || zero_bad != 0;
  }
  if (!FP4) {
    for (const int c : {0x7f, 0xff})
      for (const int si : {2, 4, 7})
        printf("%s code 0x%02x, scale byte %3d: result 0x%04x\n", name, c, SCALE_BYTES[si], out[2 * ((c * NSEL) * 8 + si) + 1] & 0xffffu);
  }
  hipFree(dp); hipFree(dv); hipFree(dout); hipFree(ds);
  return failures;
}

int main() {
  const int f4 = run<true>("fp4 (v_cvt_scalef32_pk_bf16_fp4)");
  const int f8 = run<false>("fp8 (v_cvt_scalef32_pk_bf16_fp8)");
  if (f4 < 0 || f8 < 0) return 2;
  printf("%s\n", f4 + f8 ? "MX CVT LAB: FINDINGS CONTRADICT WHAT gemm_mx_wo.hip ASSUMES" : "MX CVT LAB: both conversions are exact and take positions (2 sel, 2 sel + 1)");
  return f4 + f8 ? 1 : 0;
}
