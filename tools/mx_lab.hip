// mx_lab.hip -- pins the operand maps of v_mfma_scale_f32_32x32x64_f8f6f4 / _16x16x128_ on the device with exact integer data.
// Stand-alone (`make -C tools mx_lab && tools/mx_lab`); the output is kept in profiles/mx/mx_lab.log, the findings in DESIGN section 8b.
//
// One wave runs ONE instruction on registers the host packed under a stated hypothesis; the host compares all results with the
// exact product  C[i][j] = sum_blocks 2^(SA[i][b] + SB[j][b] - 254) * sum_{k in b} A[i][k] * B[k][j].  Element values are in
// {0, +-1, +-2, +-3} (exact in e4m3 and e2m1), scale bytes 125 .. 129 from (3 * row + 7 * block) % 5 for A and
// (2 * col + 3 * block + 1) % 5 for B (both depend on the block), A and B from different asymmetric formulas (a symmetric
// B hides a transposed write).  Every sum is a small multiple of 2^-4: exact in fp32 in any summation order.
// Hypothesis H (what gemm_mx.hip relies on):
//   lane l holds row (A) / column (B) l % R; g = l / R is its lane group (R = 32: 2 groups, R = 16: 4 groups);
//   fp4: the lane holds the 32 elements of block g, k = 32 g + j in nibble j of the FIRST 4 dwords (element 2i = low nibble of byte
//        i); dwords 4 .. 7 are not read (the lab fills them with ones);
//   fp8: the lane holds 16 bytes of TWO halves of the K step: dword d, byte b is k = (R = 32 ? 32 : 64) * (d >> 2) + 16 g + 4 (d & 3) + b
//        -- the layout of two back-to-back 8-bit MFMAs of half the K -- so a 32-element block is spread over two lane groups;
//   scales: lane group g supplies the scale of block g (k = 32 g .. 32 g + 31) of its row, in the byte of its scale register that
//        opsel (0 .. 3) names (the lab puts wrong values in the other three bytes).
// H0, the first guess for fp8 (a lane's 8 dwords are the 32 consecutive bytes of block g), also runs and must FAIL.
// A mixed fp4 x fp8 product also runs with the fp4 nibbles swapped (hypothesis N'), which must FAIL: it shows the data tells the two
// nibble orders apart.  A same-format product cannot see the element order inside a lane, and no product can see a relabelling of
// the blocks applied to A, B and both scales alike: H is established up to those, which is all a kernel can depend on.
// Last case (for gemm_fp8.hip): the UNSCALED opcode v_mfma_f32_*_f8f6f4 against the scaled one with every scale byte
// 127, fp8 x fp8 on the same data, both shapes -- they must agree bit for bit and with the exact product.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <int R, int CB, int BL, int OA, int OB>
__global__ void one_mfma(const int* __restrict__ a, const int* __restrict__ b, const int* __restrict__ sa, const int* __restrict__ sb,
                         float* __restrict__ c) {
  const int l = threadIdx.x;
  i32x8 av, bv;
  for (int d = 0; d < 8; ++d) { av[d] = a[l * 8 + d]; bv[d] = b[l * 8 + d]; }
  if constexpr (R == 32) {
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, CB, BL, OA, sa[l], OB, sb[l]);
    for (int r = 0; r < 16; ++r) c[l * 16 + r] = acc[r];
  } else {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, CB, BL, OA, sa[l], OB, sb[l]);
    for (int r = 0; r < 4; ++r) c[l * 16 + r] = acc[r];
  }
}

// the same instruction through the builtin with LITERAL zero scale operands, which the compiler emits as the unscaled opcode
// v_mfma_f32_*_f8f6f4 (no scale register): gemm_fp8.hip relies on it meaning "both scales 1.0" -- a RUNTIME scale byte of 0 is 2^-127
template <int R>
__global__ void one_mfma_unscaled(const int* __restrict__ a, const int* __restrict__ b, const int*, const int*, float* __restrict__ c) {
  const int l = threadIdx.x;
  i32x8 av, bv;
  for (int d = 0; d < 8; ++d) { av[d] = a[l * 8 + d]; bv[d] = b[l * 8 + d]; }
  if constexpr (R == 32) {
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 0, 0, 0, 0, 0, 0);
    for (int r = 0; r < 16; ++r) c[l * 16 + r] = acc[r];
  } else {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 0, 0, 0, 0, 0, 0);
    for (int r = 0; r < 4; ++r) c[l * 16 + r] = acc[r];
  }
}

typedef void (*kern_t)(const int*, const int*, const int*, const int*, float*);
struct Variant { int R, cb, bl, oa, ob; kern_t k; };
#define V(R, CB, BL, OA, OB) {R, CB, BL, OA, OB, one_mfma<R, CB, BL, OA, OB>}
static const Variant variants[] = {
    V(32, 0, 0, 0, 0), V(32, 4, 4, 0, 0), V(32, 4, 0, 0, 0), V(32, 0, 4, 0, 0), V(32, 0, 0, 0, 3), V(32, 0, 0, 1, 2), V(32, 0, 0, 2, 1),
    V(32, 0, 0, 3, 0), V(32, 4, 0, 2, 2), V(16, 0, 0, 0, 0), V(16, 4, 0, 0, 0), V(16, 4, 4, 2, 1), V(16, 0, 4, 1, 3)};

static int code_of(int v, int fmt) {
  static const int c8[4] = {0x00, 0x38, 0x40, 0x44}, c4[4] = {0, 2, 4, 5};
  const int m = v < 0 ? -v : v;
  return fmt == 0 ? (c8[m] | (v < 0 ? 0x80 : 0)) : (c4[m] | (v < 0 ? 8 : 0));
}

struct Problem {
  int R, KD;                   // rows = cols = R, K = KD
  int A[32][128], B[128][32];  // values
  int SA[32][4], SB[32][4];    // scale bytes per (row / column, block)
};

static bool contiguous_fp8 = false;  // pack fp8 under H0
static void pack(const Problem& p, bool isA, int fmt, int opsel, bool swap_nibbles, int* regs, int* sc) {
  for (int l = 0; l < 64; ++l) {
    const int row = l % p.R, blk = l / p.R;
    uint32_t w[8];
    for (int d = 0; d < 8; ++d) w[d] = fmt == 0 ? 0u : (d < 4 ? 0u : 0xffffffffu);
    for (int j = 0; j < 32; ++j) {
      const int d = j >> 2, b = j & 3;
      const int k = (fmt == 0 && !contiguous_fp8) ? (p.R == 32 ? 32 : 64) * (d >> 2) + 16 * blk + 4 * (d & 3) + b : 32 * blk + j;
      const uint32_t cde = (uint32_t)code_of(isA ? p.A[row][k] : p.B[k][row], fmt);
      if (fmt == 0) w[j >> 2] |= cde << (8 * (j & 3));
      else w[j >> 3] |= cde << (4 * ((swap_nibbles ? (j ^ 1) : j) & 7));
    }
    memcpy(regs + l * 8, w, 32);
    const int s = isA ? p.SA[row][blk] : p.SB[row][blk];
    uint32_t sv = 0;
    for (int byte = 0; byte < 4; ++byte) sv |= (uint32_t)(byte == opsel ? s : (s ^ 0x15) + byte) << (8 * byte);
    sc[l] = (int)sv;
  }
}

static double expect(const Problem& p, int i, int j) {
  double s = 0;
  for (int b = 0; b < p.KD / 32; ++b) {
    int dot = 0;
    for (int k = 32 * b; k < 32 * b + 32; ++k) dot += p.A[i][k] * p.B[k][j];
    s += ldexp((double)dot, p.SA[i][b] + p.SB[j][b] - 254);
  }
  return s;
}

static int *dA, *dB, *dSA, *dSB;
static float* dC;

static int run(const Problem& p, const Variant& v, bool swapA, bool swapB, float* out) {
  int ra[512], rb[512], sa[64], sb[64];
  pack(p, true, v.cb, v.oa, swapA, ra, sa);
  pack(p, false, v.bl, v.ob, swapB, rb, sb);
  hipMemcpy(dA, ra, sizeof ra, hipMemcpyHostToDevice);
  hipMemcpy(dB, rb, sizeof rb, hipMemcpyHostToDevice);
  hipMemcpy(dSA, sa, sizeof sa, hipMemcpyHostToDevice);
  hipMemcpy(dSB, sb, sizeof sb, hipMemcpyHostToDevice);
  hipMemset(dC, 0xff, 1024 * 4);
  v.k<<<1, 64>>>(dA, dB, dSA, dSB, dC);
  if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return -1; }
  hipMemcpy(out, dC, 1024 * 4, hipMemcpyDeviceToHost);
  return 0;
}

// C/D map: 32x32: col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); 16x16: col = l & 15, row = 4 * (l >> 4) + r
static int mismatches(const Problem& p, const float* out) {
  int bad = 0;
  const int nr = p.R == 32 ? 16 : 4;
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < nr; ++r) {
      const int j = l % p.R, i = p.R == 32 ? (r & 3) + 8 * (r >> 2) + 4 * (l >> 5) : 4 * (l >> 4) + r;
      if ((double)out[l * 16 + r] != expect(p, i, j)) ++bad;
    }
  return bad;
}

static void fill(Problem& p, int R) {
  memset(&p, 0, sizeof p);
  p.R = R;
  p.KD = R == 32 ? 64 : 128;
  for (int i = 0; i < R; ++i)
    for (int k = 0; k < p.KD; ++k) {
      p.A[i][k] = (i * 7 + k * 3 + (i * k) % 5) % 7 - 3;
      p.B[k][i] = (k * 5 + i * 11 + (k ^ i) % 3) % 7 - 3;
    }
  for (int i = 0; i < R; ++i)
    for (int b = 0; b < p.KD / 32; ++b) {
      p.SA[i][b] = 125 + (3 * i + 7 * b) % 5;
      p.SB[i][b] = 125 + (2 * i + 3 * b + 1) % 5;
    }
}

int main() {
  hipMalloc(&dA, 2048); hipMalloc(&dB, 2048); hipMalloc(&dSA, 256); hipMalloc(&dSB, 256); hipMalloc(&dC, 4096);
  static float out[1024];
  static Problem p;
  int failures = 0;
  const char* fn[5] = {"fp8", "?", "?", "?", "fp4"};
  for (const Variant& v : variants) {
    fill(p, v.R);
    if (run(p, v, false, false, out)) return 2;
    const int bad = mismatches(p, out);
    printf("%dx%dx%d  A=%s B=%s opsel_a=%d opsel_b=%d  hypothesis H: %4d / %d results differ  %s\n", v.R, v.R, p.KD, fn[v.cb], fn[v.bl],
           v.oa, v.ob, bad, v.R * v.R, bad ? "FAIL" : "ok");
    failures += bad != 0;
    if (v.cb == 0 && v.bl == 0 && v.oa == 0 && v.ob == 0) {
      contiguous_fp8 = true;
      if (run(p, v, false, false, out)) return 2;
      contiguous_fp8 = false;
      const int alt = mismatches(p, out);
      printf("        same with 32 consecutive bytes per lane (H0):    %4d / %d differ  %s\n", alt, v.R * v.R,
             alt ? "ok (H0 refuted)" : "FAIL (data cannot tell)");
      failures += alt == 0;
    }
    if (v.cb != v.bl) {  // the nibble order matters only against the other format's byte order
      if (run(p, v, v.cb == 4, v.bl == 4, out)) return 2;
      const int alt = mismatches(p, out);
      printf("        same with the fp4 nibbles swapped (N'):          %4d / %d differ  %s\n", alt, v.R * v.R,
             alt ? "ok (N' refuted)" : "FAIL (data cannot tell)");
      failures += alt == 0;
    }
  }
  // scale bytes 0 and 254: one product 1 * 1 at (0, 0, k = 0), every other element zero
  const struct { int sa, sb; double want; } ext[] = {{0, 254, 1.0}, {254, 127, ldexp(1.0, 127)}, {0, 127, ldexp(1.0, -127)},
                                                     {1, 126, ldexp(1.0, -127)}, {0, 0, 0.0}, {254, 0, 1.0}};
  for (const auto& e : ext) {
    fill(p, 32);
    memset(p.A, 0, sizeof p.A);
    memset(p.B, 0, sizeof p.B);
    p.A[0][0] = 1;
    p.B[0][0] = 1;
    for (int i = 0; i < 32; ++i)
      for (int b = 0; b < 2; ++b) { p.SA[i][b] = e.sa; p.SB[i][b] = e.sb; }
    if (run(p, variants[0], false, false, out)) return 2;
    uint32_t bits;
    memcpy(&bits, &out[0], 4);
    const bool ok = (double)out[0] == e.want;
    printf("scale bytes A=%3d B=%3d, 1 * 1: C[0][0] = %.9g (0x%08x), 2^(A + B - 254) = %.9g  %s\n", e.sa, e.sb, (double)out[0], bits,
           e.want, ok ? "ok" : "DIFFERS");
    failures += !ok;
  }
  // unscaled opcode against the scaled one with every scale byte 127, fp8 x fp8, on the asymmetric data above, both shapes
  for (const int R : {32, 16}) {
    static float scaled[1024], unscaled[1024];
    fill(p, R);
    for (int i = 0; i < R; ++i)
      for (int b = 0; b < 4; ++b) { p.SA[i][b] = 127; p.SB[i][b] = 127; }
    const Variant vs = {R, 0, 0, 0, 0, R == 32 ? one_mfma<32, 0, 0, 0, 0> : one_mfma<16, 0, 0, 0, 0>};
    const Variant vu = {R, 0, 0, 0, 0, R == 32 ? one_mfma_unscaled<32> : one_mfma_unscaled<16>};
    if (run(p, vs, false, false, scaled) || run(p, vu, false, false, unscaled)) return 2;
    const int nr = R == 32 ? 16 : 4;
    int differ = 0;
    for (int l = 0; l < 64; ++l) differ += memcmp(&scaled[l * 16], &unscaled[l * 16], nr * 4) != 0;
    const int bad_s = mismatches(p, scaled), bad_u = mismatches(p, unscaled);
    printf("%dx%dx%d  fp8 x fp8, unscaled opcode against scaled with bytes 127: %d / 64 lanes differ in bits; against the exact product: "
           "scaled %d, unscaled %d of %d differ  %s\n", R, R, p.KD, differ, bad_s, bad_u, R * R, differ || bad_s || bad_u ? "DIFFERS" : "ok");
    failures += differ || bad_s || bad_u;
  }
  printf("%s\n", failures ? "MX LAB: FINDINGS CONTRADICT THE HYPOTHESIS" : "MX LAB: hypothesis H holds");
  return failures ? 1 : 0;
}
