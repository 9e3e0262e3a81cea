// tools/kbench.hip -- kernel-level check + timing harness over the C-ABI (no Python, no torch: starts in
// milliseconds on a fresh GPU box).  Build: make -C tools.  Run: tools/kbench [gemm|gemv|hessian|probe|all]
//
// Everything here is test infrastructure: the references are a naive fp32 kernel and the library's own
// first-generation tilings (which the pytest suite pins against the oracle).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <cstring>
#include <vector>

#include "../include/inc_mi355x.h"
#include "../neural_compressor_amd/csrc/gptq_common.hpp"  // the harness flag names of the GPTQ kernel families

// A/B switch of the HARNESS build of the library (tools/libinc_mi355x_kbench.so, -DINC_KBENCH): 0 = shipped kernels;
// 1 = first-generation kernels; 2 = second-generation 256x256 two-stage dequant-GEMM; 4 / 6 = the other instruction
// schedules of the 3A2B dequant-GEMM; 20-30, 31-37 = timing-only ablations of its step (wrong results by construction).
// Not part of libinc_mi355x.so.
extern "C" void inc_debug_set_small_tiles(int on);

#define HIPCHECK(x)                                                                      \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                           \
    }                                                                                    \
  } while (0)
#define INCCHECK(x)                                                                \
  do {                                                                             \
    int r_ = (x);                                                                  \
    if (r_ != INC_OK) {                                                            \
      fprintf(stderr, "INC error %d (%s) at %s:%d\n", r_, inc_error_string(r_), __FILE__, __LINE__); \
      exit(3);                                                                     \
    }                                                                              \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static inline uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}
static inline float rnd_uniform() { return (float)(rnd() & 0xffffff) / 16777216.f; }  // [0, 1)
static inline float rnd_normal() {  // sum of 4 uniforms, unit variance, zero mean
  float s = 0.f;
  for (int i = 0; i < 4; ++i) s += (float)(rnd() & 0xffffff) / 16777216.f - 0.5f;
  return s * 1.7320508f;
}
static inline uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static inline uint16_t f2h(float f) {
  _Float16 h = (_Float16)f;
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  explicit DevBuf(size_t n_) : n(n_) { HIPCHECK(hipMalloc(&p, n * sizeof(T))); }
  ~DevBuf() { (void)hipFree(p); }
  void upload(const std::vector<T>& h) { HIPCHECK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); }
  std::vector<T> download() const {
    std::vector<T> h(n);
    HIPCHECK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
  void zero() { HIPCHECK(hipMemset(p, 0, n * sizeof(T))); }
};

// y_ref[m, n] = sum_k x[m,k] * w[n,k] in fp32 (bf16 inputs), rows listed in `rows`
__global__ void ref_gemm_rows(const uint16_t* x, const uint16_t* w, const int* rows, int nrows, int64_t N, int64_t K,
                              float* out) {
  const int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (n >= N || r >= nrows) return;
  const uint16_t* xr = x + (int64_t)rows[r] * K;
  const uint16_t* wr = w + n * K;
  float acc = 0.f;
  for (int64_t k = 0; k < K; ++k)
    acc += __uint_as_float((uint32_t)xr[k] << 16) * __uint_as_float((uint32_t)wr[k] << 16);
  out[(int64_t)r * N + n] = acc;
}

// H_ref[i, j] = sum_t x[t,i] x[t,j] for sampled (i, j)
__global__ void ref_hessian_samples(const uint16_t* x, int64_t T, int64_t K, const int* ii, const int* jj, int ns,
                                    double* out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  double acc = 0.0;
  for (int64_t t = 0; t < T; ++t)
    acc += (double)__uint_as_float((uint32_t)x[t * K + ii[s]] << 16) * (double)__uint_as_float((uint32_t)x[t * K + jj[s]] << 16);
  out[s] = acc;
}

struct Timer {
  hipEvent_t a, b;
  Timer() { HIPCHECK(hipEventCreate(&a)); HIPCHECK(hipEventCreate(&b)); }
  void start() { HIPCHECK(hipEventRecord(a, 0)); }
  float stop_ms() {
    HIPCHECK(hipEventRecord(b, 0));
    HIPCHECK(hipEventSynchronize(b));
    float ms;
    HIPCHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
};

struct Packed {
  int64_t N, K, G;
  int gs;
  DevBuf<int32_t> qweight, qzeros;
  DevBuf<uint16_t> scales;
  Packed(int64_t N_, int64_t K_, int gs_, bool sym)
      : N(N_), K(K_), G((K_ + gs_ - 1) / gs_), gs(gs_), qweight((size_t)(K_ / 8) * N_), qzeros((size_t)((K_ + gs_ - 1) / gs_) * ((N_ + 7) / 8)),
        scales((size_t)((K_ + gs_ - 1) / gs_) * N_) {
    std::vector<int32_t> qw(qweight.n), qz(qzeros.n);
    std::vector<uint16_t> sc(scales.n);
    for (auto& v : qw) v = (int32_t)rnd();
    for (auto& v : qz) v = sym ? 0x77777777 : (int32_t)rnd();
    for (auto& v : sc) v = f2h(0.004f + 0.004f * ((rnd() & 0xffff) / 65536.f));
    qweight.upload(qw);
    qzeros.upload(qz);
    scales.upload(sc);
  }
};

static int run_gemm_case(int64_t M, int64_t N, int64_t K, int gs, bool sym, bool with_bias, bool time_it, int check_rows) {
  Packed W(N, K, gs, sym);
  DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N), y_old((size_t)M * N), dense((size_t)N * K), bias((size_t)N);
  {
    std::vector<uint16_t> hx(x.n), hb(N);
    for (auto& v : hx) v = f2bf(rnd_normal());
    for (auto& v : hb) v = f2bf(rnd_normal());
    x.upload(hx);
    bias.upload(hb);
  }
  const int64_t wsb = inc_woq_gemm_workspace_bytes(M, N, K);
  DevBuf<char> ws((size_t)(wsb > 0 ? wsb : 16));
  ws.zero();
  const void* bp = with_bias ? bias.p : nullptr;
  inc_debug_set_small_tiles(0);
  INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
  HIPCHECK(hipDeviceSynchronize());
  inc_debug_set_small_tiles(1);
  INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y_old.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
  HIPCHECK(hipDeviceSynchronize());
  inc_debug_set_small_tiles(0);
  // (0) the alternative schedules of the 3A2B kernel keep the accumulation order: bit-identical outputs required
  std::vector<uint16_t> hy = y.download(), hyo = y_old.download();
  int sched_mismatch = 0;
  if (M > 64) {  // (M <= 64 takes the streaming kernel: another summation order)
    // reference for the bitwise check: the producer / consumer tile kernel (flag 42; the DEFAULT route of a mid-M shape is the strip
    // kernel, which sums in another order)
    inc_debug_set_small_tiles(42);
    INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y_old.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    const std::vector<uint16_t> hpc = y_old.download();
    const int alts[3] = {40, 4, 6};  // 3A2B pinned / compiler-ordered / ping-pong vs the producer-consumer kernel
    for (int a = 0; a < 3; ++a) {
      inc_debug_set_small_tiles(alts[a]);
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y_old.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
      HIPCHECK(hipDeviceSynchronize());
      std::vector<uint16_t> ha = y_old.download();
      if (memcmp(ha.data(), hpc.data(), hpc.size() * 2) != 0) {
        ++sched_mismatch;
        printf("  schedule flag %d: output differs from the producer / consumer kernel\n", alts[a]);
      }
    }
    inc_debug_set_small_tiles(0);
  }
  // (1) full coverage: new tiling vs first-generation tiling (same arithmetic, different fp32 summation order)
  double num = 0, den = 0;
  int64_t big = 0;
  for (size_t i = 0; i < hy.size(); ++i) {
    const double a = bf2f(hy[i]), b = bf2f(hyo[i]);
    num += (a - b) * (a - b);
    den += b * b;
    if (fabs(a - b) > 0.02 * (fabs(b) + 1.0)) ++big;
  }
  const double rel_old = sqrt(num / (den + 1e-30));
  // (2) sampled rows vs a naive fp32 GEMM over the library's own dequantised (bf16) weight
  INCCHECK(inc_woq_dequant(W.qweight.p, W.scales.p, W.qzeros.p, nullptr, dense.p, INC_BF16, N, K, W.G, gs, 4, nullptr));
  std::vector<int> rows;
  for (int r = 0; r < check_rows; ++r) rows.push_back((int)(((int64_t)r * 7919) % M));
  rows[0] = 0;
  rows[check_rows - 1] = (int)(M - 1);
  DevBuf<int> drows(rows.size());
  drows.upload(rows);
  DevBuf<float> ref((size_t)check_rows * N);
  ref_gemm_rows<<<dim3((unsigned)((N + 255) / 256), (unsigned)check_rows), 256>>>(x.p, dense.p, drows.p, check_rows, N, K, ref.p);
  HIPCHECK(hipDeviceSynchronize());
  std::vector<float> href = ref.download();
  std::vector<uint16_t> hb = bias.download();
  double num2 = 0, den2 = 0, maxabs = 0;
  for (int r = 0; r < check_rows; ++r)
    for (int64_t n = 0; n < N; ++n) {
      const double b = href[(size_t)r * N + n] + (with_bias ? bf2f(hb[n]) : 0.f);
      const double a = bf2f(hy[(size_t)rows[r] * N + n]);
      num2 += (a - b) * (a - b);
      den2 += b * b;
      if (fabs(a - b) > maxabs) maxabs = fabs(a - b);
    }
  const double rel_ref = sqrt(num2 / (den2 + 1e-30));
  const bool ok = rel_old < 3e-3 && rel_ref < 3e-3 && big == 0 && sched_mismatch == 0;
  printf("GEMM M=%ld N=%ld K=%ld gs=%d %s%s: rel(new vs old tiling)=%.2e outliers=%ld rel(new vs fp32 ref, %d rows)=%.2e maxabs=%.3g  %s\n",
         (long)M, (long)N, (long)K, gs, sym ? "sym" : "asym", with_bias ? "+bias" : "", rel_old, (long)big, check_rows, rel_ref, maxabs,
         ok ? "OK" : "FAIL");
  if (time_it) {
    // interleaved rounds (the first variant timed after an idle gap runs at lower clocks: single back-to-back timings were
    // biased by ~8 %): every round times every variant, rotating the order; the median over rounds is reported
    Timer t;
    const int modes[3] = {0, M <= 64 ? 42 : 40, 4};
    const char* labels[3] = {M <= 64 ? "streaming (default)" : "PC producer/consumer", M <= 64 ? "256-row tile + split-K" : "3A2B pinned pipeline", "3A2B compiler sched"};
    const int nv = 3, rounds = 5, iters = M <= 16 ? 100 : 8;
    std::vector<std::vector<float>> ms(nv);
    for (int i = 0; i < 10; ++i)  // warm the clocks
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
    for (int r = 0; r < rounds; ++r)
      for (int vi = 0; vi < nv; ++vi) {
        const int mi = (vi + r) % nv, mode = modes[mi];
        if (mode != 0 && M <= 16) continue;
        if (mode == 4 && M <= 64) continue;
        inc_debug_set_small_tiles(mode);
        INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
        t.start();
        for (int i = 0; i < iters; ++i)
          INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
        ms[mi].push_back(t.stop_ms() / iters);
      }
    const double flops = 2.0 * M * N * K;
    const double bytes = (double)N * K / 2 + (double)W.G * N * 2 + (double)W.G * (N / 8) * 4 + (double)M * K * 2 + (double)M * N * 2;
    for (int mi = 0; mi < nv; ++mi) {
      if (ms[mi].empty()) continue;
      std::sort(ms[mi].begin(), ms[mi].end());
      const float med = ms[mi][ms[mi].size() / 2], best = ms[mi][0];
      printf("  %-22s median %9.4f ms %8.1f TFLOP/s %8.1f GB/s   (best %9.4f ms %8.1f TFLOP/s)\n", labels[mi], med, flops / med / 1e9,
             bytes / med / 1e6, best, flops / best / 1e9);
    }
    inc_debug_set_small_tiles(0);
  }
  return ok ? 0 : 1;
}

// ---- direct-to-register dequant-GEMM (gemm_d2r.hip, harness flags 90..99) vs the producer / consumer kernel (flag 42): bitwise, then timed ----
static int run_d2r_case(int64_t M, int64_t N, int64_t K, int gs, bool sym, bool with_bias, bool time_it, bool ablate) {
  Packed W(N, K, gs, sym);
  DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N), y2((size_t)M * N), bias((size_t)N);
  {
    std::vector<uint16_t> hx(x.n), hb(N);
    for (auto& v : hx) v = f2bf(rnd_normal());
    for (auto& v : hb) v = f2bf(rnd_normal());
    x.upload(hx);
    bias.upload(hb);
  }
  const int64_t wsb = inc_woq_gemm_workspace_bytes(M, N, K);
  DevBuf<char> ws((size_t)(wsb > 0 ? wsb : 16));
  ws.zero();
  const void* bp = with_bias ? bias.p : nullptr;
  auto run = [&](int mode, uint16_t* out) {
    inc_debug_set_small_tiles(mode);
    INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, out, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
  };
  HIPCHECK(hipMemset(y.p, 0xff, y.n * 2));
  HIPCHECK(hipMemset(y2.p, 0xee, y2.n * 2));
  run(42, y.p);
  HIPCHECK(hipDeviceSynchronize());
  int fails = 0;
  const int chk[3] = {90, 91, 97};
  std::vector<uint16_t> h1 = y.download();
  for (int c = 0; c < 3; ++c) {
    HIPCHECK(hipMemset(y2.p, 0xee, y2.n * 2));
    run(chk[c], y2.p);
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint16_t> h2 = y2.download();
    size_t diff = 0, first = 0;
    for (size_t i = 0; i < h1.size(); ++i)
      if (h1[i] != h2[i]) { if (!diff) first = i; ++diff; }
    printf("D2R M=%ld N=%ld K=%ld gs=%d %s%s flag %d: %zu of %zu outputs differ from the producer/consumer kernel%s", (long)M, (long)N, (long)K, gs,
           sym ? "sym" : "asym", with_bias ? "+bias" : "", chk[c], diff, h1.size(), diff ? "" : "  OK\n");
    if (diff) { printf(" (first at row %zu col %zu: %04x vs %04x)  FAIL\n", first / N, first % N, h2[first], h1[first]); ++fails; }
  }
  if (time_it) {
    const int nv_all = 9;
    const int modes[nv_all] = {42, 90, 97, 91, 92, 93, 94, 95, 96};
    const char* labels[nv_all] = {"PC producer/consumer", "D2R 4 x-stages", "D2R8 two waves per SIMD", "D2R 3 x-stages", "D2R - x LDS-DMA", "D2R - W loads", "D2R - all global traffic",
                                  "D2R - global - barrier", "D2R - epilogue stores"};
    const int nv = ablate ? nv_all : 3, rounds = 5, iters = 8;
    std::vector<std::vector<float>> ms(nv);
    Timer t;
    for (int i = 0; i < 10; ++i) run(42, y.p);
    for (int r = 0; r < rounds; ++r)
      for (int vi = 0; vi < nv; ++vi) {
        const int mi = (vi + r) % nv;
        run(modes[mi], y.p);
        t.start();
        for (int i = 0; i < iters; ++i) run(modes[mi], y.p);
        ms[mi].push_back(t.stop_ms() / iters);
      }
    for (int mi = 0; mi < nv; ++mi) {
      std::sort(ms[mi].begin(), ms[mi].end());
      const float med = ms[mi][ms[mi].size() / 2];
      printf("  %-28s median %8.4f ms %8.1f TFLOP/s   (best %8.4f ms %8.1f)\n", labels[mi], med, 2.0 * M * N * K / med / 1e9, ms[mi][0], 2.0 * M * N * K / ms[mi][0] / 1e9);
    }
  }
  inc_debug_set_small_tiles(0);
  return fails;
}


// ---- per-workgroup timeline of the direct-to-register dequant-GEMM (harness flag 98): where the kernel's span goes ----
extern "C" int inc_debug_set_d2r_timeline(void* dev_buffer);
extern "C" int64_t inc_debug_lazy_x3_bytes(int64_t N, int64_t K);
extern "C" int inc_debug_lazy_x3_prepare(const float* Hinv, int64_t N, int64_t K, void* planes, inc_stream_t stream);
extern "C" void inc_debug_set_d2r_abl(int abl);
static void run_d2r_timeline(int64_t M, int64_t N, int64_t K, int abl = 256, const char* label = "full kernel") {
  Packed W(N, K, 128, true);
  DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N);
  {
    std::vector<uint16_t> hx(x.n);
    for (auto& v : hx) v = f2bf(rnd_normal());
    x.upload(hx);
  }
  const int64_t nwg = ((M + 255) / 256) * ((N + 255) / 256);
  DevBuf<unsigned long long> tl((size_t)nwg * 10 + 256);
  tl.zero();
  inc_debug_set_d2r_timeline(tl.p);
  inc_debug_set_small_tiles(90);
  for (int i = 0; i < 6; ++i)  // warm clocks with the plain kernel
    INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
  inc_debug_set_small_tiles(98);
  inc_debug_set_d2r_abl(abl);
  Timer t;
  for (int i = 0; i < 3; ++i)
    INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
  t.start();
  INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
  const float ev_ms = t.stop_ms();
  HIPCHECK(hipDeviceSynchronize());
  inc_debug_set_small_tiles(0);
  inc_debug_set_d2r_timeline(nullptr);
  std::vector<unsigned long long> h = tl.download();
  const double tick_us = 0.01;  // s_memrealtime: 100 MHz
  unsigned long long t_first = ~0ull, t_last = 0;
  for (int64_t w = 0; w < nwg; ++w) {
    t_first = std::min(t_first, h[w * 10 + 0]);
    t_last = std::max(t_last, h[w * 10 + 3]);
  }
  std::vector<double> start, pro, loop, epi, endgap, cyc_step, mhz;
  double xcd_loop[8] = {0}, xcd_end[8] = {0};
  int xcd_n[8] = {0};
  const int nk = (int)(K / 64);
  for (int64_t w = 0; w < nwg; ++w) {
    const unsigned long long* e = &h[w * 10];
    start.push_back((e[0] - t_first) * tick_us);
    pro.push_back((e[1] - e[0]) * tick_us);
    loop.push_back((e[2] - e[1]) * tick_us);
    epi.push_back((e[3] - e[2]) * tick_us);
    endgap.push_back((t_last - e[3]) * tick_us);
    cyc_step.push_back((double)(e[6] - e[5]) / nk);
    mhz.push_back((double)(e[6] - e[5]) / ((e[2] - e[1]) * tick_us));
    const int xc = (int)(e[8] & 7);
    xcd_loop[xc] += (e[2] - e[1]) * tick_us;
    xcd_end[xc] += (e[3] - t_first) * tick_us;
    ++xcd_n[xc];
  }
  auto stats = [](std::vector<double> v, const char* label, const char* unit) {
    std::sort(v.begin(), v.end());
    double sum = 0;
    for (double a : v) sum += a;
    printf("    %-34s mean %9.2f  min %9.2f  p10 %9.2f  p50 %9.2f  p90 %9.2f  max %9.2f %s\n", label, sum / v.size(), v.front(), v[v.size() / 10], v[v.size() / 2],
           v[v.size() * 9 / 10], v.back(), unit);
  };
  printf("D2R TIMELINE [%s] M=%ld N=%ld K=%ld: %ld workgroups (%.2f per CU), %d K-steps; HIP-event time %.1f us, first entry -> last store acknowledged %.1f us\n", label,
         (long)M, (long)N, (long)K, (long)nwg, nwg / 256.0, nk, ev_ms * 1e3, (t_last - t_first) * tick_us);
  stats(start, "entry after the first entry", "us");
  stats(pro, "prologue (entry -> first K-step)", "us");
  stats(loop, "K-loop", "us");
  stats(epi, "epilogue (-> stores acknowledged)", "us");
  stats(endgap, "finished before the last one by", "us");
  stats(cyc_step, "shader cycles per K-step", "cycles (2048 = MFMA-bound)");
  stats(mhz, "shader clock inside the K-loop", "MHz");
  printf("    per XCD (mean K-loop us / mean end time us / workgroups):");
  for (int i = 0; i < 8; ++i) printf("  %d: %.1f / %.1f / %d", i, xcd_n[i] ? xcd_loop[i] / xcd_n[i] : 0.0, xcd_n[i] ? xcd_end[i] / xcd_n[i] : 0.0, xcd_n[i]);
  printf("\n");
}

// ---- mid-M strip kernel vs the 256-row tile + split-K path: checked against the fp32 reference rows, then timed --------
static int run_strip_case(int64_t M, int64_t N, int64_t K, int gs, bool sym, bool with_bias, bool time_it) {
  Packed W(N, K, gs, sym);
  DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N), dense((size_t)N * K), bias((size_t)N);
  {
    std::vector<uint16_t> hx(x.n), hb(N);
    for (auto& v : hx) v = f2bf(rnd_normal());
    for (auto& v : hb) v = f2bf(rnd_normal());
    x.upload(hx);
    bias.upload(hb);
  }
  const int64_t wsb = inc_woq_gemm_workspace_bytes(M, N, K);
  DevBuf<char> ws((size_t)(wsb > 0 ? wsb : 16));
  ws.zero();
  const void* bp = with_bias ? bias.p : nullptr;
  INCCHECK(inc_woq_dequant(W.qweight.p, W.scales.p, W.qzeros.p, nullptr, dense.p, INC_BF16, N, K, W.G, gs, 4, nullptr));
  const int check_rows = (int)(M < 96 ? M : 96);
  std::vector<int> rows;
  for (int r = 0; r < check_rows; ++r) rows.push_back((int)(((int64_t)r * 7919) % M));
  rows[0] = 0;
  rows[check_rows - 1] = (int)(M - 1);
  DevBuf<int> drows(rows.size());
  drows.upload(rows);
  DevBuf<float> ref((size_t)check_rows * N);
  ref_gemm_rows<<<dim3((unsigned)((N + 255) / 256), (unsigned)check_rows), 256>>>(x.p, dense.p, drows.p, check_rows, N, K, ref.p);
  HIPCHECK(hipDeviceSynchronize());
  std::vector<float> href = ref.download();
  std::vector<uint16_t> hb = bias.download();
  const int NV = 7;
  const int modes[NV] = {M <= 64 ? 83 : 0, 42, M <= 64 ? 0 : 40, 84, 100, 101, 102};
  const char* labels[NV] = {"strip (LDS-DMA rings)", "PC 256-row tile + split-K", M <= 64 ? "streaming kernel (default)" : "3A2B 256-row tile + split-K",
                            "strip, 4 waves x 6-deep ring", "strip, LDS reads 1 ahead", "strip, setprio on compute", "strip, reads ahead + prio"};
  int fails = 0;
  std::vector<uint16_t> first;
  for (int mi = 0; mi < NV; ++mi) {
    inc_debug_set_small_tiles(modes[mi]);
    y.zero();
    for (int rep = 0; rep < 2; ++rep)  // twice: the arrival counters must have been re-armed
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint16_t> hy = y.download();
    double num = 0, den = 0, maxabs = 0;
    for (int r = 0; r < check_rows; ++r)
      for (int64_t n = 0; n < N; ++n) {
        const double b = href[(size_t)r * N + n] + (with_bias ? bf2f(hb[n]) : 0.f);
        const double a = bf2f(hy[(size_t)rows[r] * N + n]);
        num += (a - b) * (a - b);
        den += b * b;
        if (fabs(a - b) > maxabs) maxabs = fabs(a - b);
      }
    const double rel = sqrt(num / (den + 1e-30));
    const bool ok = rel < 3e-3;
    if (!ok) ++fails;
    printf("STRIP M=%ld N=%ld K=%ld gs=%d %s%s [%s]: rel vs fp32 ref (%d rows)=%.2e maxabs=%.3g %s\n", (long)M, (long)N, (long)K, gs,
           sym ? "sym" : "asym", with_bias ? "+bias" : "", labels[mi], check_rows, rel, maxabs, ok ? "OK" : "FAIL");
  }
  inc_debug_set_small_tiles(0);
  if (time_it) {
    Timer t;
    const int rounds = 5, iters = 20;
    std::vector<std::vector<float>> ms(NV);
    for (int i = 0; i < 10; ++i)
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
    for (int r = 0; r < rounds; ++r)
      for (int vi = 0; vi < NV; ++vi) {
        const int mi = (vi + r) % NV;
        inc_debug_set_small_tiles(modes[mi]);
        INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
        t.start();
        for (int i = 0; i < iters; ++i)
          INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
        ms[mi].push_back(t.stop_ms() / iters);
      }
    const double flops = 2.0 * M * N * K;
    for (int mi = 0; mi < NV; ++mi) {
      std::sort(ms[mi].begin(), ms[mi].end());
      const float med = ms[mi][ms[mi].size() / 2];
      printf("  %-24s median %9.4f ms %8.1f TFLOP/s\n", labels[mi], med, flops / med / 1e9);
    }
    inc_debug_set_small_tiles(0);
  }
  return fails;
}

// ---- decode (M <= 16): streaming split-K kernel vs the no-split kernel, each checked against the fp32 reference ------------
static int run_decode_case(int64_t M, int64_t N, int64_t K, int gs, bool sym, bool with_bias, bool time_it) {
  Packed W(N, K, gs, sym);
  DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N), dense((size_t)N * K), bias((size_t)N);
  {
    std::vector<uint16_t> hx(x.n), hb(N);
    for (auto& v : hx) v = f2bf(rnd_normal());
    for (auto& v : hb) v = f2bf(rnd_normal());
    x.upload(hx);
    bias.upload(hb);
  }
  const int64_t wsb = inc_woq_gemm_workspace_bytes(M, N, K);
  DevBuf<char> ws((size_t)(wsb > 0 ? wsb : 16));
  ws.zero();
  const void* bp = with_bias ? bias.p : nullptr;
  INCCHECK(inc_woq_dequant(W.qweight.p, W.scales.p, W.qzeros.p, nullptr, dense.p, INC_BF16, N, K, W.G, gs, 4, nullptr));
  const int check_rows = (int)M;
  std::vector<int> rows;
  for (int r = 0; r < check_rows; ++r) rows.push_back(r);
  DevBuf<int> drows(rows.size());
  drows.upload(rows);
  DevBuf<float> ref((size_t)check_rows * N);
  ref_gemm_rows<<<dim3((unsigned)((N + 255) / 256), (unsigned)check_rows), 256>>>(x.p, dense.p, drows.p, check_rows, N, K, ref.p);
  HIPCHECK(hipDeviceSynchronize());
  std::vector<float> href = ref.download();
  std::vector<uint16_t> hb = bias.download();
  const int modes[5] = {0, 85, 103, 104, 0};
  const char* labels[5] = {"default dispatch", "16 columns x whole K (no split-K)", "no split-K, non-temporal W loads", "streaming, non-temporal W loads", "default dispatch (again)"};
  int fails = 0;
  for (int mi = 0; mi < 4; ++mi) {  // (flag 103 needs K <= 12288: the dispatch falls back to the default otherwise)
    inc_debug_set_small_tiles(modes[mi]);
    y.zero();
    INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint16_t> hy = y.download();
    double num = 0, den = 0;
    for (int r = 0; r < check_rows; ++r)
      for (int64_t n = 0; n < N; ++n) {
        const double b = href[(size_t)r * N + n] + (with_bias ? bf2f(hb[n]) : 0.f);
        const double a = bf2f(hy[(size_t)r * N + n]);
        num += (a - b) * (a - b);
        den += b * b;
      }
    const double rel = sqrt(num / (den + 1e-30));
    const bool ok = rel < 3e-3;
    if (!ok) ++fails;
    printf("DECODE M=%ld N=%ld K=%ld gs=%d %s%s [%s]: rel vs fp32 ref=%.2e %s\n", (long)M, (long)N, (long)K, gs, sym ? "sym" : "asym",
           with_bias ? "+bias" : "", labels[mi], rel, ok ? "OK" : "FAIL");
  }
  inc_debug_set_small_tiles(0);
  if (time_it) {
    Timer t;
    const int rounds = 5, iters = 200;
    std::vector<std::vector<float>> ms(5);
    for (int i = 0; i < 50; ++i)
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
    for (int r = 0; r < rounds; ++r)
      for (int vi = 0; vi < 5; ++vi) {
        const int mi = (vi + r) % 5;
        inc_debug_set_small_tiles(modes[mi]);
        INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
        t.start();
        for (int i = 0; i < iters; ++i)
          INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, bp, y.p, M, N, K, W.G, gs, 4, ws.p, wsb, nullptr));
        ms[mi].push_back(t.stop_ms() / iters);
      }
    const double bytes = (double)N * K / 2 + (double)W.G * N * 2 + (double)W.G * (N / 8) * 4 + (double)M * K * 2 + (double)M * N * 2;
    for (int mi = 0; mi < 5; ++mi) {
      std::sort(ms[mi].begin(), ms[mi].end());
      const float med = ms[mi][ms[mi].size() / 2];
      printf("  %-36s median %8.2f us %8.1f GB/s\n", labels[mi], med * 1e3, bytes / med / 1e6);
    }
    inc_debug_set_small_tiles(0);
  }
  return fails;
}

static int run_gemv_repeat(int64_t N, int64_t K, int M) {
  // the arrival counters must re-arm: 50 back-to-back calls on one workspace give bit-identical outputs
  Packed W(N, K, 128, true);
  DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N);
  std::vector<uint16_t> hx(x.n);
  for (auto& v : hx) v = f2bf(rnd_normal());
  x.upload(hx);
  const int64_t wsb = inc_woq_gemm_workspace_bytes(M, N, K);
  DevBuf<char> ws((size_t)wsb);
  ws.zero();
  std::vector<uint16_t> first;
  int bad = 0;
  for (int it = 0; it < 50; ++it) {
    INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, ws.p, wsb, nullptr));
    std::vector<uint16_t> hy = y.download();
    if (it == 0) first = hy;
    else if (memcmp(first.data(), hy.data(), hy.size() * 2) != 0) ++bad;
  }
  printf("GEMV repeat M=%d N=%ld K=%ld: %d of 49 repeats differ from the first call  %s\n", M, (long)N, (long)K, bad, bad ? "FAIL" : "OK");
  return bad ? 1 : 0;
}

// K14: W8A8 GEMM -- a sampled check against a naive int32 dot product, then timing (Llama-2-13B shapes of BASELINE config #4)
__global__ void ref_i8_rows(const int8_t* xq, const int8_t* wq, const int* rows, int nrows, int64_t N, int64_t K, int* out) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (n >= N || r >= nrows) return;
  const int8_t* a = xq + (int64_t)rows[r] * K;
  const int8_t* b = wq + n * K;
  int acc = 0;
  for (int64_t k = 0; k < K; ++k) acc += (int)a[k] * (int)b[k];
  out[(int64_t)r * N + n] = acc;
}

static int run_i8_case(int64_t M, int64_t N, int64_t K) {
  DevBuf<int8_t> xq((size_t)M * K), wq((size_t)N * K);
  DevBuf<float> alpha((size_t)N);
  DevBuf<int32_t> corr((size_t)N);
  DevBuf<uint16_t> y((size_t)M * N);
  {
    std::vector<int8_t> hx(xq.n), hw(wq.n);
    for (auto& v : hx) v = (int8_t)((int)(rnd_uniform() * 256.f) - 128);
    for (auto& v : hw) v = (int8_t)((int)(rnd_uniform() * 256.f) - 128);
    std::vector<float> ha(N);
    std::vector<int32_t> hc(N);
    for (int64_t n = 0; n < N; ++n) { ha[n] = 1e-5f * (1.f + rnd_uniform()); hc[n] = (int32_t)(rnd_uniform() * 20000.f) - 10000; }
    xq.upload(hx); wq.upload(hw); alpha.upload(ha); corr.upload(hc);
  }
  const int64_t wsb = inc_w8a8_gemm_workspace_bytes(M, N, K);
  DevBuf<char> ws((size_t)(wsb > 0 ? wsb : 16));
  ws.zero();
  DevBuf<uint16_t> y1((size_t)M * N);
  INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, corr.p, nullptr, y1.p, INC_BF16, M, N, K, nullptr, 0, nullptr));  // unsplit
  INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, corr.p, nullptr, y.p, INC_BF16, M, N, K, ws.p, wsb, nullptr));
  INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, corr.p, nullptr, y.p, INC_BF16, M, N, K, ws.p, wsb, nullptr));     // tickets re-armed
  HIPCHECK(hipDeviceSynchronize());
  const int check_rows = 16;
  std::vector<int> rows;
  for (int r = 0; r < check_rows; ++r) rows.push_back((int)(((int64_t)r * 7919) % M));
  rows[check_rows - 1] = (int)(M - 1);
  DevBuf<int> drows(rows.size());
  drows.upload(rows);
  DevBuf<int> ref((size_t)check_rows * N);
  ref_i8_rows<<<dim3((unsigned)((N + 255) / 256), (unsigned)check_rows), 256>>>(xq.p, wq.p, drows.p, check_rows, N, K, ref.p);
  HIPCHECK(hipDeviceSynchronize());
  std::vector<int> href = ref.download();
  std::vector<uint16_t> hy = y.download(), hy1 = y1.download();
  const bool split_same = memcmp(hy.data(), hy1.data(), hy.size() * 2) == 0;
  std::vector<float> ha = alpha.download();
  std::vector<int32_t> hc = corr.download();
  int64_t bad = 0;
  for (int r = 0; r < check_rows; ++r)
    for (int64_t n = 0; n < N; ++n) {
      const float want = ha[n] * (float)(href[(size_t)r * N + n] + hc[n]);
      if (hy[(size_t)rows[r] * N + n] != f2bf(want)) ++bad;
    }
  if (!split_same) ++bad;
  Timer t;
  for (int i = 0; i < 10; ++i) INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, corr.p, nullptr, y.p, INC_BF16, M, N, K, ws.p, wsb, nullptr));
  std::vector<float> ms, ms1;
  for (int r = 0; r < 5; ++r) {
    t.start();
    for (int i = 0; i < 8; ++i) INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, corr.p, nullptr, y.p, INC_BF16, M, N, K, ws.p, wsb, nullptr));
    ms.push_back(t.stop_ms() / 8);
    t.start();
    for (int i = 0; i < 8; ++i) INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, corr.p, nullptr, y.p, INC_BF16, M, N, K, nullptr, 0, nullptr));
    ms1.push_back(t.stop_ms() / 8);
  }
  std::sort(ms.begin(), ms.end());
  std::sort(ms1.begin(), ms1.end());
  printf("  tail split-K %s (workspace %ld B): unsplit median %8.4f ms, outputs %s\n", wsb > 0 ? "on" : "not needed", (long)wsb, ms1[2],
         split_same ? "bit-identical" : "DIFFER");
  const double ops = 2.0 * M * N * K, bytes = (double)M * K + (double)N * K + 2.0 * M * N;
  printf("W8A8 GEMM M=%ld N=%ld K=%ld: %ld mismatching outputs in %d sampled rows  median %8.4f ms %8.1f TOP/s %7.1f GB/s  (best %8.4f ms %8.1f TOP/s)  %s\n",
         (long)M, (long)N, (long)K, (long)bad, check_rows, ms[2], ops / ms[2] / 1e9, bytes / ms[2] / 1e6, ms[0], ops / ms[0] / 1e9, bad ? "FAIL" : "OK");
  return bad ? 1 : 0;
}

static int run_hessian_case(int64_t T, int64_t K, bool time_it) {
  DevBuf<uint16_t> x((size_t)T * K);
  {
    std::vector<uint16_t> hx(x.n);
    for (auto& v : hx) v = f2bf(rnd_normal());
    x.upload(hx);
  }
  DevBuf<float> H((size_t)K * K), Hold((size_t)K * K);
  H.zero();
  Hold.zero();
  inc_debug_set_small_tiles(0);  // default: the transpose-read generation
  INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, H.p, 0.f, 1.f, nullptr));
  INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, H.p, 0.5f, 0.25f, nullptr));  // exercises beta/alpha
  inc_debug_set_small_tiles(1);
  INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, Hold.p, 0.f, 1.f, nullptr));
  INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, Hold.p, 0.5f, 0.25f, nullptr));
  inc_debug_set_small_tiles(0);
  HIPCHECK(hipDeviceSynchronize());
  std::vector<float> h = H.download(), ho = Hold.download();
  double num = 0, den = 0;
  int64_t differ = 0;
  for (int64_t i = 0; i < K; ++i)
    for (int64_t j = i; j < K; ++j) {  // upper triangle only (syrk contract)
      const double a = h[i * K + j], b = ho[i * K + j];
      num += (a - b) * (a - b);
      den += b * b;
      if (a != b) ++differ;
    }
  const double rel = sqrt(num / (den + 1e-30));
  // sampled entries vs fp64
  const int ns = 256;
  std::vector<int> ii(ns), jj(ns);
  for (int s = 0; s < ns; ++s) {
    int a = (int)(rnd() % K), b = (int)(rnd() % K);
    if (a > b) { int t = a; a = b; b = t; }
    if (s < 8) { a = b = (int)((K - 1) * s / 7); }
    ii[s] = a; jj[s] = b;
  }
  DevBuf<int> dii(ns), djj(ns);
  dii.upload(ii); djj.upload(jj);
  DevBuf<double> dref(ns);
  ref_hessian_samples<<<(ns + 63) / 64, 64>>>(x.p, T, K, dii.p, djj.p, ns, dref.p);
  HIPCHECK(hipDeviceSynchronize());
  std::vector<double> r = dref.download();
  double maxrel = 0;
  for (int s = 0; s < ns; ++s) {
    const double want = 0.75 * r[s];  // 0.5*(1*S) + 0.25*S
    const double got = h[(int64_t)ii[s] * K + jj[s]];
    const double e = fabs(got - want) / (fabs(want) + 1e-3 * sqrt((double)T));
    if (e > maxrel) maxrel = e;
  }
  // correct A/B partners: the same tile with its LDS-DMA requests spread over the step's MFMA rows (and its row fragments requested two rows
  // ahead) -- same arithmetic, same bits
  int64_t spread_differ = 0;
  for (int flag : {LAB_HESSIAN_SPREAD, LAB_HESSIAN_SPREAD_ROLL, LAB_HESSIAN_SPREAD_ROLL_PRIO, LAB_HESSIAN_ROLL_PRIO, LAB_HESSIAN_ROUND4}) {
    if (K % 8 != 0) break;
    Hold.zero();
    inc_debug_set_small_tiles(flag);
    INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, Hold.p, 0.f, 1.f, nullptr));
    INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, Hold.p, 0.5f, 0.25f, nullptr));
    inc_debug_set_small_tiles(0);
    HIPCHECK(hipDeviceSynchronize());
    ho = Hold.download();
    for (int64_t i = 0; i < K; ++i)
      for (int64_t j = i; j < K; ++j)
        if (h[i * K + j] != ho[i * K + j]) ++spread_differ;
  }
  const bool ok = rel < 1e-5 && maxrel < 1e-3 && spread_differ == 0;
  printf("HESSIAN T=%ld K=%ld: rel(256-tile vs 128-tile)=%.2e (%ld entries differ) max rel err vs fp64 on %d samples=%.2e; spread-DMA tile: %ld entries differ from the default  %s\n", (long)T,
         (long)K, rel, (long)differ, ns, maxrel, (long)spread_differ, ok ? "OK" : "FAIL");
  if (time_it) {
    Timer t;
    const int modes[14] = {0, LAB_HESSIAN_ROUND4, LAB_HESSIAN_ROLL, LAB_HESSIAN_PRIO, LAB_HESSIAN_ROLL_PRIO, LAB_HESSIAN_PIPELINE, LAB_HESSIAN_SPREAD,
                           LAB_HESSIAN_STAGES_4X32, LAB_HESSIAN_REG_TRANSPOSE, 1, LAB_HESSIAN_NO_DMA, LAB_HESSIAN_NO_MFMA, LAB_HESSIAN_NO_DMA_NO_MFMA, 0};
    const char* labels[14] = {"256x256 TR 2x64 (pipeline + prio)", "256x256 TR 2x64, round-4 form", "256x256 TR 2x64, rolling frags", "256x256 TR 2x64, prio 1 for waves 4-7", "256x256 TR 2x64, rolling + prio",
                              "256x256 TR 2x64, one pipeline per step",
                              "256x256 TR 2x64, DMA spread", "256x256 transpose-read 4x32", "256x256 register transpose", "128x128 tiles",
                             "  TR timing-only: no LDS-DMA", "  TR timing-only: no MFMA / frag reads", "  TR timing-only: barriers + epilogue",
                             "256x256 transpose-read 2x64 (again)"};
    for (int mi = 0; mi < 14; ++mi) {
      inc_debug_set_small_tiles(modes[mi]);
      for (int i = 0; i < 2; ++i) INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, H.p, 0.5f, 0.5f, nullptr));
      const int iters = 10;
      t.start();
      for (int i = 0; i < iters; ++i) INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, H.p, 0.5f, 0.5f, nullptr));
      const float ms = t.stop_ms() / iters;
      printf("  %-28s %9.4f ms  %8.1f TFLOP/s (2*T*K^2 convention)\n", labels[mi], ms, 2.0 * T * K * K / ms / 1e9);
    }
    inc_debug_set_small_tiles(0);
  }
  return ok ? 0 : 1;
}

// the Llama-block launch of the bench: three K = 4096 Hessians and one K = 11008 Hessian of one forward in ONE launch
static int run_hessian_multi_case(int64_t T) {
  const int64_t Ks[4] = {4096, 4096, 4096, 11008};
  std::vector<DevBuf<uint16_t>*> xs;
  std::vector<DevBuf<float>*> Hs;
  const void* xp[4];
  float* hp[4];
  int64_t ld[4];
  float betas[4], alphas[4];
  double flops = 0;
  for (int i = 0; i < 4; ++i) {
    xs.push_back(new DevBuf<uint16_t>((size_t)T * Ks[i]));
    Hs.push_back(new DevBuf<float>((size_t)Ks[i] * Ks[i]));
    std::vector<uint16_t> hx((size_t)T * Ks[i]);
    for (auto& v : hx) v = f2bf(rnd_normal());
    xs[i]->upload(hx);
    Hs[i]->zero();
    xp[i] = xs[i]->p; hp[i] = Hs[i]->p; ld[i] = Ks[i]; betas[i] = 0.5f; alphas[i] = 0.5f;
    flops += 2.0 * T * Ks[i] * Ks[i];
  }
  printf("HESSIAN multi T=%ld K=4096+4096+4096+11008 (one launch)\n", (long)T);
  DevBuf<char> hws((size_t)inc_gptq_hessian_accum_multi_workspace_bytes());
  int bad = 0;
  {  // the split tail against the unsplit launch (LAB_HESSIAN_NO_TAIL_SPLIT): identical outside the tail tiles, fp32 rounding inside
    std::vector<std::vector<float>> ref;
    for (int pass = 0; pass < 2; ++pass) {
      inc_debug_set_small_tiles(pass == 0 ? LAB_HESSIAN_NO_TAIL_SPLIT : 0);
      for (int i = 0; i < 4; ++i) Hs[i]->zero();
      float b0[4] = {0.f, 0.f, 0.f, 0.f};
      INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hp, b0, alphas, hws.p, (int64_t)hws.n, nullptr));
      INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hp, betas, alphas, hws.p, (int64_t)hws.n, nullptr));  // beta != 0 too
      HIPCHECK(hipDeviceSynchronize());
      for (int i = 0; i < 4; ++i) {
        std::vector<float> h = Hs[i]->download();
        if (pass == 0) { ref.push_back(h); continue; }
        size_t ndiff = 0;
        double worst = 0, norm = 0;
        for (int64_t r = 0; r < Ks[i]; ++r)
          for (int64_t c = r; c < Ks[i]; ++c) {  // (upper-triangular tiles are what the kernel writes; the strict lower part of a diagonal tile too)
            const float a = h[r * Ks[i] + c], b = ref[i][r * Ks[i] + c];
            if (memcmp(&a, &b, 4) != 0) { ++ndiff; worst = std::max(worst, (double)fabsf(a - b)); }
            norm = std::max(norm, (double)fabsf(b));
          }
        const bool ok = worst <= 5e-6 * norm;
        printf("  split tail vs one workgroup per tile, K=%ld: %zu elements differ, worst |diff| %.3g (largest |H| %.3g)  %s\n", (long)Ks[i], ndiff, worst,
               norm, ok ? "OK" : "FAIL");
        bad += ok ? 0 : 1;
      }
    }
    inc_debug_set_small_tiles(0);
  }
  Timer t;
  const int nm = 10;
  const int modes[nm] = {0, LAB_HESSIAN_ROUND4, LAB_HESSIAN_ROLL, LAB_HESSIAN_PRIO, LAB_HESSIAN_ROLL_PRIO, LAB_HESSIAN_PIPELINE, LAB_HESSIAN_NO_TAIL_SPLIT,
                         LAB_HESSIAN_STAGES_4X32, LAB_HESSIAN_REG_TRANSPOSE, 0};
  const char* labels[nm] = {"transpose-read 2x64", "  round-4 form", "  rolling frags", "  prio 1 for waves 4-7", "  rolling + prio", "  one pipeline per step",
                            "  - tail split", "transpose-read 4x32", "register transpose", "transpose-read 2x64 (again)"};
  for (int mi = 0; mi < nm; ++mi) {
    inc_debug_set_small_tiles(modes[mi]);
    for (int i = 0; i < 2; ++i) INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hp, betas, alphas, hws.p, (int64_t)hws.n, nullptr));
    const int iters = 10;
    t.start();
    for (int i = 0; i < iters; ++i) INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hp, betas, alphas, hws.p, (int64_t)hws.n, nullptr));
    const float ms = t.stop_ms() / iters;
    printf("  %-28s %9.4f ms  %8.1f TFLOP/s (2*T*K^2 convention)\n", labels[mi], ms, flops / ms / 1e9);
  }
  inc_debug_set_small_tiles(0);
  for (auto* b : xs) delete b;
  for (auto* b : Hs) delete b;
  return bad;
}

// ---- round 5: A/B of tile variants in the batched Hessian launch, timed there and back (kbench hpf) ----
__global__ void fill_bf16_kernel(uint16_t* x, size_t n, uint32_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u ^ (uint32_t)(i >> 32) * 40503u ^ seed;
    float acc = 0.f;
    for (int r = 0; r < 4; ++r) {  // sum of four uniforms: bell-shaped, every mantissa bit busy
      h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
      acc += (float)(h & 0xffffff) * (1.f / 16777216.f) - 0.5f;
    }
    const uint32_t u = __float_as_uint(acc * 1.7f);
    x[i] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  }
}
__global__ void count_diff_kernel(const float* a, const float* b, size_t n, unsigned long long* out) {
  unsigned long long c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    c += __float_as_uint(a[i]) != __float_as_uint(b[i]);
  if (c) atomicAdd(out, c);
}
static int run_hessian_pf_case(int64_t T, int passes) {
  const int64_t Ks[4] = {4096, 4096, 4096, 11008};
  std::vector<DevBuf<uint16_t>*> xs;
  std::vector<DevBuf<float>*> Hs, Hr;
  const void* xp[4];
  float *hp[4], *hr[4];
  int64_t ld[4];
  float betas[4], alphas[4], b0[4] = {0.f, 0.f, 0.f, 0.f};
  double flops = 0;
  for (int i = 0; i < 4; ++i) {
    xs.push_back(new DevBuf<uint16_t>((size_t)T * Ks[i]));
    Hs.push_back(new DevBuf<float>((size_t)Ks[i] * Ks[i]));
    Hr.push_back(new DevBuf<float>((size_t)Ks[i] * Ks[i]));
    fill_bf16_kernel<<<2048, 256>>>(xs[i]->p, xs[i]->n, 0x9e3779b9u * (i + 1));
    Hs[i]->zero(); Hr[i]->zero();
    xp[i] = xs[i]->p; hp[i] = Hs[i]->p; hr[i] = Hr[i]->p; ld[i] = Ks[i]; betas[i] = 0.5f; alphas[i] = 0.5f;
    flops += 2.0 * T * Ks[i] * Ks[i];
  }
  HIPCHECK(hipDeviceSynchronize());
  printf("HESSIAN tile variants (harness flags), multi T=%ld K=4096+4096+4096+11008 (one launch)\n", (long)T);
  DevBuf<char> hws((size_t)inc_gptq_hessian_accum_multi_workspace_bytes());
  DevBuf<unsigned long long> dcount(1);
  constexpr int NM = 4;
  const int modes[NM] = {0, LAB_HESSIAN_PIPELINE_PRIO, LAB_HESSIAN_ROUND4, LAB_HESSIAN_PIPELINE_PRIO};  // product (one-block issue), the same without it, the round-4 form
  int bad = 0;
  inc_debug_set_small_tiles(0);
  INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hr, b0, alphas, hws.p, (int64_t)hws.n, nullptr));
  for (int mi = 1; mi < NM; ++mi) {
    inc_debug_set_small_tiles(modes[mi]);
    INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hp, b0, alphas, hws.p, (int64_t)hws.n, nullptr));
    dcount.zero();
    for (int i = 0; i < 4; ++i) count_diff_kernel<<<1024, 256>>>(hp[i], hr[i], Hs[i]->n, dcount.p);
    HIPCHECK(hipDeviceSynchronize());
    const unsigned long long nd = dcount.download()[0];
    printf("  flag %d: %llu elements differ from the product launch  %s\n", modes[mi], nd, nd ? "FAIL" : "OK");
    bad += nd ? 1 : 0;
  }
  Timer t;
  std::vector<std::vector<float>> ms(NM);
  for (int pass = 0; pass < passes; ++pass)
    for (int k = 0; k < NM; ++k) {
      const int mi = (pass & 1) ? NM - 1 - k : k;  // there and back: position in the sequence must not decide
      inc_debug_set_small_tiles(modes[mi]);
      INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hp, betas, alphas, hws.p, (int64_t)hws.n, nullptr));
      const int iters = 4;
      t.start();
      for (int i = 0; i < iters; ++i) INCCHECK(inc_gptq_hessian_accum_multi(4, xp, INC_BF16, T, Ks, ld, hp, betas, alphas, hws.p, (int64_t)hws.n, nullptr));
      ms[mi].push_back(t.stop_ms() / iters);
    }
  inc_debug_set_small_tiles(0);
  for (int mi = 0; mi < NM; ++mi) {
    std::vector<float> v = ms[mi];
    std::sort(v.begin(), v.end());
    printf("  flag %3d  median %8.4f ms  min %8.4f  max %8.4f  %8.1f TFLOP/s (2*T*K^2, median) |", modes[mi], v[v.size() / 2], v.front(), v.back(),
           flops / v[v.size() / 2] / 1e9);
    for (float m : ms[mi]) printf(" %.3f", m);
    printf("\n");
  }
  for (auto* b : xs) delete b;
  for (auto* b : Hs) delete b;
  for (auto* b : Hr) delete b;
  return bad;
}

// ---- GPTQ column loop: quad-per-row quant block + lazy update generations (3rd = default, 2nd = LAB_LAZY_V2, 1st = flag 1) --------
static void colloop_inputs(int64_t N, int64_t K, int gs, std::vector<float>& hw, std::vector<float>& hh, std::vector<float>& hs, std::vector<float>& hz) {
  hw.resize((size_t)N * K); hh.assign((size_t)K * K, 0.f);
  for (auto& v : hw) v = 0.02f * rnd_normal();
  for (int64_t i = 0; i < K; ++i) {  // upper-triangular "Cholesky factor of H^-1": positive diagonal, small off-diagonal
    hh[i * K + i] = 0.5f + (float)(rnd() & 0xffff) / 65536.f;
    for (int64_t j = i + 1; j < K; ++j) hh[i * K + j] = 0.02f * rnd_normal();
  }
  const int64_t G = (K + gs - 1) / gs;
  hs.resize((size_t)N * G); hz.assign((size_t)N * G, 8.f);
  for (auto& v : hs) v = 0.01f + 0.005f * (float)(rnd() & 0xffff) / 65536.f;
}

static int run_colloop_case(int64_t N, int64_t K, int gs, int nblocks, bool time_it) {
  std::vector<float> hw, hh, hs, hz;
  colloop_inputs(N, K, gs, hw, hh, hs, hz);
  const int64_t G = (K + gs - 1) / gs;
  DevBuf<float> Hinv((size_t)K * K), sc(hs.size()), ze(hz.size());
  Hinv.upload(hh); sc.upload(hs); ze.upload(hz);
  constexpr int NV = 4;
  const int flag[NV] = {0, LAB_LAZY_V2, 1, LAB_LAZY_V3_ONLY};
  const char* label[NV] = {"product (4th / 3rd)", "second generation", "first generation", "third generation only"};
  std::vector<DevBuf<float>*> W, E;
  std::vector<DevBuf<uint8_t>*> C;
  std::vector<DevBuf<uint16_t>*> Q;
  for (int m = 0; m < NV; ++m) {
    W.push_back(new DevBuf<float>((size_t)N * K)); E.push_back(new DevBuf<float>((size_t)N * 128));
    C.push_back(new DevBuf<uint8_t>((size_t)N * K)); Q.push_back(new DevBuf<uint16_t>((size_t)N * K));
    W[m]->upload(hw); C[m]->zero(); Q[m]->zero();
  }
  const int nb = (int)(nblocks < K / 128 ? nblocks : K / 128);
  for (int m = 0; m < NV; ++m) {
    inc_debug_set_small_tiles(flag[m]);
    for (int b = 0; b < nb; ++b) {
      INCCHECK(inc_gptq_quant_block(W[m]->p, Hinv.p, sc.p, ze.p, C[m]->p, Q[m]->p, INC_BF16, E[m]->p, N, K, G, (int64_t)b * 128, 128, gs, 4, nullptr));
      if (m == 0 && (b & 1) && (int64_t)(b + 2) * 128 < K) {  // every other block in the look-ahead loop's two pieces
        INCCHECK(inc_gptq_lazy_update_cols(W[m]->p, Hinv.p, E[m]->p, N, K, (int64_t)b * 128, 128, (int64_t)(b + 1) * 128, (int64_t)(b + 2) * 128, nullptr));
        INCCHECK(inc_gptq_lazy_update_cols(W[m]->p, Hinv.p, E[m]->p, N, K, (int64_t)b * 128, 128, (int64_t)(b + 2) * 128, K, nullptr));
      } else {
        INCCHECK(inc_gptq_lazy_update(W[m]->p, Hinv.p, E[m]->p, N, K, (int64_t)b * 128, 128, nullptr));
      }
    }
  }
  inc_debug_set_small_tiles(0);
  HIPCHECK(hipDeviceSynchronize());
  bool ok = true;
  std::vector<float> w0 = W[0]->download(), e0 = E[0]->download();
  std::vector<uint8_t> c0 = C[0]->download();
  std::vector<uint16_t> q0 = Q[0]->download();
  for (int m = 1; m < NV; ++m) {
    std::vector<float> w1 = W[m]->download(), e1 = E[m]->download();
    std::vector<uint8_t> c1 = C[m]->download();
    std::vector<uint16_t> q1 = Q[m]->download();
    int64_t dw = 0, de = 0, dc = 0, dq = 0;
    for (size_t i = 0; i < w0.size(); ++i) { dw += memcmp(&w0[i], &w1[i], 4) != 0; dc += c0[i] != c1[i]; dq += q0[i] != q1[i]; }
    for (size_t i = 0; i < e0.size(); ++i) de += memcmp(&e0[i], &e1[i], 4) != 0;
    const bool okm = dw == 0 && de == 0 && dc == 0 && dq == 0;
    ok = ok && okm;
    printf("COLLOOP N=%ld K=%ld gs=%d blocks=%d: differing W=%ld Err=%ld codes=%ld Q=%ld (product vs %s, bitwise)  %s\n", (long)N,
           (long)K, gs, nb, (long)dw, (long)de, (long)dc, (long)dq, label[m], okm ? "OK" : "FAIL");
  }
  if (time_it) {
    Timer t;
    for (int m = 0; m < NV; ++m) {
      inc_debug_set_small_tiles(flag[m]);
      float tq = 0, tl = 0, tn = 0;
      int nn = 0;
      for (int b = 0; b < nb; ++b) {
        t.start();
        INCCHECK(inc_gptq_quant_block(W[m]->p, Hinv.p, sc.p, ze.p, C[m]->p, Q[m]->p, INC_BF16, E[m]->p, N, K, G, (int64_t)b * 128, 128, gs, 4, nullptr));
        tq += t.stop_ms();
        t.start();
        INCCHECK(inc_gptq_lazy_update(W[m]->p, Hinv.p, E[m]->p, N, K, (int64_t)b * 128, 128, nullptr));
        tl += t.stop_ms();
        if (m < 2 && (int64_t)(b + 2) * 128 <= K) {  // the look-ahead loop's "next 128 columns" piece alone
          t.start();
          INCCHECK(inc_gptq_lazy_update_cols(W[m]->p, Hinv.p, E[m]->p, N, K, (int64_t)b * 128, 128, (int64_t)(b + 1) * 128, (int64_t)(b + 2) * 128, nullptr));
          tn += t.stop_ms();
          ++nn;
        }
      }
      double fl = 0;
      for (int b = 0; b < nb; ++b) fl += 2.0 * N * 128 * (double)(K - (b + 1) * 128);
      printf("  %-22s quant_block %8.3f ms/block   lazy_update %8.3f ms/block (%7.1f TFLOP/s fp32)   next-128 piece %8.3f ms\n", label[m],
             tq / nb, tl / nb, fl / (tl * 1e9), nn ? tn / nn : 0.f);
    }
    // timing-only variants of the third generation's whole-tile kernel
    const int afl[3] = {LAB_LAZY_NO_MFMA, LAB_LAZY_NO_LOADS, LAB_LAZY_NO_STORES};
    const char* alab[3] = {"3rd gen - MFMAs", "3rd gen - loads / DMA", "3rd gen - stores"};
    for (int v = 0; v < 3; ++v) {
      inc_debug_set_small_tiles(afl[v]);
      float tl = 0;
      for (int b = 0; b < nb; ++b) {
        t.start();
        INCCHECK(inc_gptq_lazy_update(W[0]->p, Hinv.p, E[0]->p, N, K, (int64_t)b * 128, 128, nullptr));
        tl += t.stop_ms();
      }
      printf("  %-22s lazy_update %8.3f ms/block (timing only)\n", alab[v], tl / nb);
    }
    inc_debug_set_small_tiles(0);
  }
  for (int m = 0; m < NV; ++m) { delete W[m]; delete E[m]; delete C[m]; delete Q[m]; }
  return ok ? 0 : 1;
}

// ---- inc_gptq_quantize_layer end to end (two streams, look-ahead): us per column; third vs second lazy-update generation bitwise ----
static int run_qlayer_case(int64_t N, int64_t K, int gs) {
  std::vector<float> hw, hh, hs, hz;
  colloop_inputs(N, K, gs, hw, hh, hs, hz);
  const int64_t G = (K + gs - 1) / gs;
  DevBuf<float> Hinv((size_t)K * K);
  Hinv.upload(hh);
  hipStream_t aux;
  HIPCHECK(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
  // third variant (LAB_LAZY_X3, an EXPERIMENT): the lazy update with split (bf16 x 3) products -- not bit-identical by construction; the
  // count of differing codes and the time are the result
  const bool x3 = (K % 128) == 0;
  DevBuf<char> planes((size_t)(x3 ? inc_debug_lazy_x3_bytes(N, K) : 16));
  const int flag[3] = {0, LAB_LAZY_V2, LAB_LAZY_X3};
  std::vector<uint8_t> codes[3];
  std::vector<float> scales[3];
  float ms[3] = {0, 0, 0}, host_ms[3] = {0, 0, 0};
  for (int m = 0; m < (x3 ? 3 : 2); ++m) {
    if (m == 2) INCCHECK(inc_debug_lazy_x3_prepare(Hinv.p, N, K, planes.p, nullptr));
    inc_debug_set_small_tiles(flag[m]);
    DevBuf<float> W((size_t)N * K), sc((size_t)N * G), ze((size_t)N * G), ews((size_t)2 * N * 128);
    DevBuf<uint8_t> C((size_t)N * K);
    DevBuf<uint16_t> Q((size_t)N * K);
    std::vector<float> t_all;
    for (int rep = 0; rep < 4; ++rep) {
      W.upload(hw);
      HIPCHECK(hipDeviceSynchronize());
      Timer t;
      t.start();
      const auto h0 = std::chrono::steady_clock::now();
      INCCHECK(inc_gptq_quantize_layer(W.p, Hinv.p, sc.p, ze.p, G, nullptr, nullptr, 0, C.p, Q.p, INC_BF16, ews.p, N, K, gs, gs, 128, 4, 1,
                                       INC_GPTQ_DYNAMIC_GROUPS, nullptr, aux));
      host_ms[m] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - h0).count();  // time to ENQUEUE the loop
      t_all.push_back(t.stop_ms());
    }
    HIPCHECK(hipDeviceSynchronize());
    std::sort(t_all.begin() + 1, t_all.end());
    ms[m] = t_all[2];
    codes[m] = C.download();
    scales[m] = sc.download();
  }
  // the strip form of the trailing update (fourth generation, the product) against the third generation everywhere (LAB_LAZY_V3_ONLY) and
  // with short strips everywhere (LAB_LAZY_SHORT_STRIPS) and strips cut at 16 tiles (LAB_LAZY_STRIP_CAP_16): interleaved repeats, codes compared bit for bit
  {
    const int vflag[4] = {0, LAB_LAZY_V3_ONLY, LAB_LAZY_SHORT_STRIPS, LAB_LAZY_STRIP_CAP_16};
    const char* vname[4] = {"strip form (product)", "third generation everywhere", "short strips (<= 8 tiles) everywhere", "strips <= 16 tiles"};
    std::vector<float> vt[4];
    int64_t vdiff[4] = {0, 0, 0, 0};
    DevBuf<float> W((size_t)N * K), sc((size_t)N * G), ze((size_t)N * G), ews((size_t)2 * N * 128);
    DevBuf<uint8_t> C((size_t)N * K);
    DevBuf<uint16_t> Q((size_t)N * K);
    for (int rep = 0; rep < 5; ++rep)
      for (int v = 0; v < 4; ++v) {
        inc_debug_set_small_tiles(vflag[v]);
        W.upload(hw);
        HIPCHECK(hipDeviceSynchronize());
        Timer t;
        t.start();
        INCCHECK(inc_gptq_quantize_layer(W.p, Hinv.p, sc.p, ze.p, G, nullptr, nullptr, 0, C.p, Q.p, INC_BF16, ews.p, N, K, gs, gs, 128, 4, 1,
                                         INC_GPTQ_DYNAMIC_GROUPS, nullptr, aux));
        const float ms1 = t.stop_ms();
        if (rep > 0) vt[v].push_back(ms1);
        if (rep == 4) {
          HIPCHECK(hipDeviceSynchronize());
          std::vector<uint8_t> c = C.download();
          for (size_t i = 0; i < c.size(); ++i) vdiff[v] += c[i] != codes[0][i];
        }
      }
    for (int v = 0; v < 4; ++v) {
      std::sort(vt[v].begin(), vt[v].end());
      printf("QLAYER N=%ld K=%ld lazy-update form [%s]: min %.3f median %.3f ms, codes differing from the product's first run: %ld\n", (long)N, (long)K,
             vname[v], vt[v][0], vt[v][vt[v].size() / 2], (long)vdiff[v]);
    }
  }
  inc_debug_set_small_tiles(0);
  INCCHECK(inc_debug_lazy_x3_prepare(nullptr, 0, 0, nullptr, nullptr));
  HIPCHECK(hipStreamDestroy(aux));
  if (x3) {
    int64_t dc3 = 0, rows3 = 0;
    double ds3 = 0;
    for (int64_t r = 0; r < N; ++r) {
      bool any = false;
      for (int64_t c = 0; c < K; ++c)
        if (codes[0][(size_t)r * K + c] != codes[2][(size_t)r * K + c]) { ++dc3; any = true; }
      rows3 += any;
    }
    for (size_t i = 0; i < scales[0].size(); ++i) ds3 = std::max(ds3, (double)fabsf(scales[0][i] - scales[2][i]) / (fabsf(scales[0][i]) + 1e-30));
    printf("QLAYER N=%ld K=%ld gs=%d [split-product lazy update, EXPERIMENT]: %.3f ms (%.3f exact fp32), %ld of %ld codes differ in %ld rows, max rel scale diff %.2e\n",
           (long)N, (long)K, gs, ms[2], ms[0], (long)dc3, (long)(N * K), (long)rows3, ds3);
  }
  int64_t dc = 0, ds = 0;
  for (size_t i = 0; i < codes[0].size(); ++i) dc += codes[0][i] != codes[1][i];
  for (size_t i = 0; i < scales[0].size(); ++i) ds += memcmp(&scales[0][i], &scales[1][i], 4) != 0;
  const bool ok = dc == 0 && ds == 0;
  printf("QLAYER N=%ld K=%ld gs=%d: %.3f ms = %.3f us/column, host enqueue %.3f ms (lazy update 2nd generation: %.3f ms = %.3f us/column); differing codes=%ld scales=%ld  %s\n",
         (long)N, (long)K, gs, ms[0], ms[0] * 1e3 / K, host_ms[0], ms[1], ms[1] * 1e3 / K, (long)dc, (long)ds, ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}

// ---- ds_read_b64_tr_b16 probe: which LDS halfwords does lane l receive? ----------------------------
__global__ void probe_tr(uint32_t* out, int addr_mode) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[4096];
  for (int i = threadIdx.x; i < 4096; i += 64) lds[i] = (uint16_t)i;
  __syncthreads();
  const int lane = threadIdx.x;
  // addr_mode 0: lane*8 bytes (every lane its own 4-halfword chunk, contiguous)
  // addr_mode 1: row-major [rows of 64 halfwords]: lane -> row (lane&15)... 128-byte pitch: (lane&15)*128 + (lane>>4)*8
  uint32_t addr = addr_mode == 0 ? lane * 8 : ((lane & 15) * 128 + (lane >> 4) * 8);
  addr += (uint32_t)(uintptr_t)lds;
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
  out[lane * 2] = v.x;
  out[lane * 2 + 1] = v.y;
}
static void run_probe() {
  DevBuf<uint32_t> out(128);
  for (int mode = 0; mode < 2; ++mode) {
    probe_tr<<<1, 64>>>(out.p, mode);
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h = out.download();
    printf("PROBE ds_read_b64_tr_b16 addr_mode=%d (value = LDS halfword index; mode0 addr=lane*8B, mode1 addr=(lane&15)*128B+(lane>>4)*8B)\n", mode);
    for (int l = 0; l < 64; ++l) {
      printf("  lane %2d: %4u %4u %4u %4u", l, h[2 * l] & 0xffff, h[2 * l] >> 16, h[2 * l + 1] & 0xffff, h[2 * l + 1] >> 16);
      if (l % 2 == 1) printf("\n");
    }
  }
}

// ---- LDS-DMA bandwidth probe: how many bytes per clock does ONE CU pull from L2 / HBM into LDS, as a function of the 1-KiB pieces
// it keeps in flight?  (The Hessian syrk and the split-product GEMM both need ~32 B/clk/CU and get ~18: is that latency x bytes
// in flight, or the issue rate of global_load_lds_dwordx4?)  One workgroup per CU (128 KiB of LDS), WAVES waves, each keeps DEPTH
// pieces in flight (issue one, wait until DEPTH - 1 are outstanding) for `iters` pieces; the source is a `span`-byte window that
// every workgroup walks from its own offset (span <= 2 MiB: L2-resident after the first pass; span = 4 GiB: streaming from HBM).
template <int DEPTH>
__global__ __launch_bounds__(1024) void dmabw_kernel(const char* __restrict__ src, uint64_t span, int iters, uint32_t* __restrict__ sink) {
  extern __shared__ __attribute__((aligned(1024))) char dm_smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)dm_smem + wave * 8192);  // 8 slots of 1 KiB per wave
  const uint32_t voff = lane * 16;
  uint64_t pos = (((uint64_t)blockIdx.x * nw + wave) * 1024 * 64) & (span - 1);  // workgroups start 64 KiB x waves apart
  const uint64_t stride = (uint64_t)nw * 1024;                          // a workgroup's waves read consecutive pieces
  for (int i = 0; i < iters; ++i) {
    const char* sp = src + pos;
    const uint32_t dst = lds0 + (i & 7) * 1024;
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sp), "s"(dst) : "memory");
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(DEPTH - 1) : "memory");
    pos = (pos + stride * 61) & (span - 1);  // (span is a power of two) an odd multiple of the stride: neighbouring pieces far apart in time
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) sink[blockIdx.x] = *reinterpret_cast<uint32_t*>(dm_smem);
}
static void run_dmabw() {
  hipDeviceProp_t prop;
  HIPCHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const uint64_t big = (uint64_t)4 << 30;
  DevBuf<char> buf((size_t)big);
  HIPCHECK(hipMemset(buf.p, 1, big));
  DevBuf<uint32_t> sink(4096);
  const int smem = 128 * 1024;
  printf("DMABW: one workgroup per CU (%d), 1-KiB pieces by global_load_lds_dwordx4; GB/s per CU and B/clk at 2.1 GHz\n", cus);
  for (uint64_t span : {(uint64_t)1 << 20, big}) {
    for (int waves : {4, 8, 16}) {
      for (int depth : {1, 2, 4, 8}) {
        const int iters = 2048 / (waves / 4);  // ~the same bytes per workgroup for every wave count
        auto launch = [&]() {
#define DM_CASE(D) case D: (void)hipFuncSetAttribute((const void*)dmabw_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, smem); \
                           dmabw_kernel<D><<<cus, waves * 64, smem>>>(buf.p, span, iters, sink.p); break;
          switch (depth) { DM_CASE(1) DM_CASE(2) DM_CASE(4) DM_CASE(8) }
#undef DM_CASE
        };
        launch();
        HIPCHECK(hipDeviceSynchronize());
        Timer t;
        t.start();
        for (int r = 0; r < 5; ++r) launch();
        const float ms = t.stop_ms() / 5;
        const double bytes_cu = (double)waves * iters * 1024, gbs = bytes_cu / (ms * 1e-3) / 1e9;
        printf("DMABW %-9s waves=%2d in-flight=%3d KiB/CU : %7.3f ms  %7.1f GB/s per CU = %5.1f B/clk, chip %6.2f TB/s, latency by Little's law %5.2f us\n",
               span == big ? "streaming" : "L2 1 MiB", waves, waves * depth, ms, gbs, gbs / 2.1, gbs * cus / 1e3, (double)waves * depth * 1024 / (gbs * 1e3));
      }
    }
  }
}

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "all";
  hipDeviceProp_t prop;
  HIPCHECK(hipGetDeviceProperties(&prop, 0));
  printf("device: %s, %d CUs, %s, ABI %d\n", prop.name, prop.multiProcessorCount, prop.gcnArchName, inc_abi_version());
  int fails = 0;
  if (what == "strip" || what == "all") {
    fails += run_strip_case(65, 200, 96, 32, false, true, false);       // ragged everything, gs=32 asym, 3 steps
    fails += run_strip_case(100, 1000, 416, 32, false, true, false);    // 13 steps over 4 waves (uneven), ragged N
    fails += run_strip_case(130, 520, 2048, 2048, true, false, false);  // single group, split-K
    fails += run_strip_case(32, 4096, 4096, 128, true, false, true);
    fails += run_strip_case(48, 4096, 4096, 128, true, false, true);
    fails += run_strip_case(64, 4096, 4096, 128, true, false, true);
    fails += run_strip_case(64, 11008, 4096, 128, true, false, true);
    fails += run_strip_case(64, 4096, 11008, 128, true, false, true);
    fails += run_strip_case(128, 4096, 4096, 128, true, false, true);
    fails += run_strip_case(256, 4096, 4096, 128, true, false, true);
    fails += run_strip_case(512, 4096, 4096, 128, false, true, true);
    fails += run_strip_case(1024, 4096, 4096, 128, true, false, true);
    fails += run_strip_case(128, 11008, 4096, 128, true, false, true);
    fails += run_strip_case(512, 11008, 4096, 128, true, false, true);
    fails += run_strip_case(512, 4096, 11008, 128, true, false, true);
  }
  if (what == "d2r" || what == "all") {
    fails += run_d2r_case(256, 256, 128, 64, false, true, false, false);      // one tile, two K-steps, gs=64 asym + bias
    fails += run_d2r_case(300, 1000, 256, 64, false, true, false, false);     // ragged M and N
    fails += run_d2r_case(700, 520, 384, 128, false, true, false, false);     // split-K slabs, ragged tiles
    fails += run_d2r_case(1024, 768, 1024, 1024, true, false, false, false);  // single group
    fails += run_d2r_case(512, 512, 896, 128, true, false, false, false);     // 14 K-steps: every remainder of the 3-step unroll
    fails += run_d2r_case(4096, 4096, 4096, 128, true, false, true, true);
    fails += run_d2r_case(4096, 11008, 4096, 128, true, false, true, false);
    fails += run_d2r_case(4096, 4096, 11008, 128, true, false, true, false);
    fails += run_d2r_case(8192, 4096, 4096, 128, false, true, true, false);
  }
  if (what == "dmabw") run_dmabw();
  if (what == "stripabl") {  // timing-only ablations of the mid-M strip kernel (outputs are wrong by construction)
    for (int64_t M : {128, 512}) {
      const int64_t N = 4096, K = 4096;
      Packed W(N, K, 128, true);
      DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N);
      std::vector<uint16_t> hx(x.n);
      for (auto& v : hx) v = f2bf(rnd_normal());
      x.upload(hx);
      const int64_t wsb = inc_woq_gemm_workspace_bytes(M, N, K);
      DevBuf<char> ws((size_t)(wsb > 0 ? wsb : 16));
      ws.zero();
      const int nv = 6, rounds = 5, iters = 20;
      const int modes[nv] = {0, 85, 86, 87, 88, 89};
      const char* labels[nv] = {"full step", "- x requests", "- W requests", "- x and W requests", "- dequant + MFMA", "- requests - dequant - MFMA"};
      std::vector<std::vector<float>> ms(nv);
      Timer t;
      for (int r = 0; r < rounds; ++r)
        for (int vi = 0; vi < nv; ++vi) {
          const int mi = (vi + r) % nv;
          inc_debug_set_small_tiles(modes[mi]);
          INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, ws.p, wsb, nullptr));
          t.start();
          for (int i = 0; i < iters; ++i)
            INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, ws.p, wsb, nullptr));
          ms[mi].push_back(t.stop_ms() / iters);
        }
      for (int mi = 0; mi < nv; ++mi) {
        std::sort(ms[mi].begin(), ms[mi].end());
        printf("STRIPABL M=%ld %-30s median %8.2f us\n", (long)M, labels[mi], ms[mi][ms[mi].size() / 2] * 1e3);
      }
      inc_debug_set_small_tiles(0);
    }
  }
  if (what == "d2rtl") {
    run_d2r_timeline(4096, 4096, 4096);
    run_d2r_timeline(4096, 4096, 11008);
    run_d2r_timeline(8192, 4096, 4096);
    run_d2r_timeline(4096, 11008, 4096);
    // timing-only ablations (wrong results by construction): cycles per K-step AND the clock each variant sustains
    run_d2r_timeline(4096, 4096, 4096, 260, "- x LDS-DMA");
    run_d2r_timeline(4096, 4096, 4096, 264, "- W loads");
    run_d2r_timeline(4096, 4096, 4096, 268, "- all global traffic");
    run_d2r_timeline(4096, 4096, 4096, 320, "- barrier");
    run_d2r_timeline(4096, 4096, 4096, 332, "- global traffic - barrier");
    run_d2r_timeline(4096, 4096, 4096, 768, "- scalar pointer arithmetic");
    run_d2r_timeline(4096, 4096, 4096, 844, "- traffic - barrier - pointer arithmetic");
    run_d2r_timeline(4096, 4096, 4096, 256, "full kernel again");
  }
  if (what == "gemm" || what == "all") {
    fails += run_gemm_case(256, 256, 64, 32, false, true, false, 64);     // one tile, one K-step, gs=32 asym
    fails += run_gemm_case(300, 1000, 192, 64, false, true, false, 64);   // ragged M and N
    fails += run_gemm_case(1024, 768, 1024, 1024, true, false, false, 64);  // single group (g_shift = -1)
    fails += run_gemm_case(300, 1000, 256, 64, false, true, false, 64);   // producer/consumer kernel: ragged M and N, gs=64 asym
    fails += run_gemm_case(700, 520, 384, 128, false, true, false, 64);   // ... odd number of K-steps per slab guard, ragged tiles
    fails += run_gemm_case(4096, 4096, 4096, 128, true, false, true, 64);
    fails += run_gemm_case(4096, 11008, 4096, 128, true, false, true, 32);
    fails += run_gemm_case(4096, 4096, 11008, 128, true, false, true, 32);
    fails += run_gemm_case(8192, 4096, 4096, 128, false, true, true, 32);
    fails += run_gemm_case(512, 4096, 4096, 128, true, false, true, 64);
    fails += run_gemm_case(128, 4096, 4096, 128, true, false, true, 64);
    fails += run_gemm_case(64, 4096, 4096, 128, true, false, true, 64);
    fails += run_gemm_case(32, 11008, 4096, 128, true, false, true, 32);
    fails += run_gemm_case(17, 4096, 11008, 128, true, false, true, 17);
    fails += run_gemm_case(33, 1000, 416, 32, false, true, false, 33);   // streaming kernel, 3 row blocks used of 4, ragged N, gs=32
    fails += run_gemm_case(48, 4096, 4096, 128, false, true, true, 48);
    fails += run_gemm_case(256, 4096, 4096, 128, true, false, true, 64);
  }
  if (what == "decode" || what == "all") {
    fails += run_decode_case(3, 1000, 416, 32, false, true, false);   // ragged N, 13 K-steps over 16 waves, gs=32 asym
    fails += run_decode_case(16, 200, 2048, 2048, true, true, false);  // one group
    fails += run_decode_case(1, 4096, 4096, 128, true, false, true);
    fails += run_decode_case(4, 4096, 4096, 128, true, false, true);
    fails += run_decode_case(16, 4096, 4096, 128, false, true, true);
    fails += run_decode_case(1, 11008, 4096, 128, true, false, true);
    fails += run_decode_case(1, 4096, 11008, 128, true, false, true);
    fails += run_decode_case(8, 4096, 11008, 128, true, true, true);
    fails += run_decode_case(1, 8192, 8192, 128, true, false, true);
    fails += run_decode_case(1, 5120, 5120, 128, true, false, true);
  }
  if (what == "gemv" || what == "all") {
    fails += run_gemm_case(1, 4096, 4096, 128, true, false, true, 1);
    fails += run_gemm_case(16, 4096, 4096, 128, false, true, true, 16);
    fails += run_gemm_case(4, 11008, 4096, 128, true, false, true, 4);
    fails += run_gemm_case(8, 4096, 11008, 128, true, true, true, 8);
    fails += run_gemm_case(3, 1000, 416, 32, false, true, false, 3);   // ragged N, K tail of the split, gs=32
    fails += run_gemv_repeat(4096, 4096, 1);
    fails += run_gemv_repeat(4096, 11008, 16);
  }
  if (what == "i8gemm" || what == "all") {
    fails += run_i8_case(300, 1000, 384);
    fails += run_i8_case(1, 5120, 5120);        // decode
    fails += run_i8_case(16, 13824, 5120);
    fails += run_i8_case(64, 5120, 5120);       // batched decode
    fails += run_i8_case(128, 13824, 5120);
    fails += run_i8_case(4096, 5120, 5120);     // Llama-2-13B q/k/v/o
    fails += run_i8_case(4096, 13824, 5120);    // gate / up
    fails += run_i8_case(4096, 5120, 13824);    // down
    fails += run_i8_case(8192, 8192, 8192);
  }
  if (what == "hessian" || what == "all") {
    fails += run_hessian_case(200, 320, false);     // token tail + ragged feature tile
    fails += run_hessian_case(2048, 4096, true);
    fails += run_hessian_case(2048, 11008, true);
    fails += run_hessian_case(16384, 4096, true);
    fails += run_hessian_case(16384, 11008, true);
    fails += run_hessian_case(1000, 520, false);      // 40-token tail, feature chunks clamped at K
    fails += run_hessian_multi_case(16384);
  }
  if (what == "hpf") {
    fails += run_hessian_pf_case(16384, 6);
    fails += run_hessian_pf_case(65536, 6);
  }
  if (what == "qlayer" || what == "all") {
    fails += run_qlayer_case(300, 640, 64);
    fails += run_qlayer_case(260, 520, 64);        // K not a multiple of 128: one stream, partial last tile, ragged last block
    fails += run_qlayer_case(4096, 4096, 128);
    fails += run_qlayer_case(12288, 4096, 128);
    fails += run_qlayer_case(22016, 4096, 128);
    fails += run_qlayer_case(4096, 11008, 128);
  }
  if (what == "colloop" || what == "all") {
    fails += run_colloop_case(200, 512, 32, 4, false);      // ragged rows, 4 groups per block
    fails += run_colloop_case(260, 520, 64, 4, false);      // partial last column tile (8 columns), ragged rows
    fails += run_colloop_case(4100, 1288, 128, 10, false);  // a row tile with 4 rows, partial last tile, whole and quarter tiles
    fails += run_colloop_case(4100, 2600, 128, 6, false);   // the strip form's edges: a row tile with 4 rows, a last tile of 8 columns
    fails += run_colloop_case(4096, 4096, 128, 32, true);
    fails += run_colloop_case(11008, 4096, 128, 8, true);
    fails += run_colloop_case(4096, 11008, 128, 8, true);
  }
  if (what == "profstrip") {  // mid-M strip kernel alone, for rocprofv3 --pmc passes
    const int64_t M = 512, N = 4096, K = 4096;
    Packed W(N, K, 128, true);
    DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N);
    std::vector<uint16_t> hx(x.n);
    for (auto& v : hx) v = f2bf(rnd_normal());
    x.upload(hx);
    const int64_t wsb = inc_woq_gemm_workspace_bytes(M, N, K);
    DevBuf<char> ws((size_t)wsb);
    ws.zero();
    for (int i = 0; i < 5; ++i)
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, ws.p, wsb, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    return 0;
  }
  if (what == "prof") {  // short, kernel-only workload for rocprofv3 --pmc passes (no reference kernels)
    {
      const int64_t M = 4096, N = 4096, K = 4096;
      Packed W(N, K, 128, true);
      DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N);
      std::vector<uint16_t> hx(x.n);
      for (auto& v : hx) v = f2bf(rnd_normal());
      x.upload(hx);
      for (int i = 0; i < 5; ++i)
        INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
      DevBuf<uint16_t> x1((size_t)K);
      x1.upload(std::vector<uint16_t>(hx.begin(), hx.begin() + K));
      const int64_t wsb = inc_woq_gemm_workspace_bytes(1, N, K);
      DevBuf<char> ws((size_t)wsb);
      ws.zero();
      for (int i = 0; i < 5; ++i)
        INCCHECK(inc_woq_gemm(x1.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, 1, N, K, W.G, 128, 4, ws.p, wsb, nullptr));
    }
    {
      const int64_t T = 16384, K = 11008;  // the bench's launch shape: 8 staged samples per launch
      DevBuf<uint16_t> x((size_t)T * K);
      std::vector<uint16_t> hx(x.n);
      for (auto& v : hx) v = f2bf(rnd_normal());
      x.upload(hx);
      DevBuf<float> H((size_t)K * K);
      H.zero();
      for (int i = 0; i < 5; ++i) INCCHECK(inc_gptq_hessian_accum(x.p, INC_BF16, T, K, K, H.p, 0.5f, 0.5f, nullptr));
    }
    {
      const int64_t M = 4096, N = 5120, K = 13824;  // W8A8 GEMM, Llama-2-13B down_proj (tail K-split active)
      DevBuf<int8_t> xq((size_t)M * K), wq((size_t)N * K);
      std::vector<int8_t> hx(xq.n), hw(wq.n);
      for (auto& v : hx) v = (int8_t)((int)(rnd_uniform() * 256.f) - 128);
      for (auto& v : hw) v = (int8_t)((int)(rnd_uniform() * 256.f) - 128);
      xq.upload(hx);
      wq.upload(hw);
      DevBuf<float> alpha((size_t)N);
      alpha.upload(std::vector<float>(N, 1e-5f));
      DevBuf<uint16_t> y((size_t)M * N);
      const int64_t wsb = inc_w8a8_gemm_workspace_bytes(M, N, K);
      DevBuf<char> ws((size_t)(wsb > 0 ? wsb : 16));
      for (int i = 0; i < 5; ++i)
        INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, nullptr, nullptr, y.p, INC_BF16, M, N, K, ws.p, wsb, nullptr));
      for (int i = 0; i < 5; ++i)
        INCCHECK(inc_w8a8_gemm(xq.p, wq.p, alpha.p, nullptr, nullptr, y.p, INC_BF16, 1, N, K, nullptr, 0, nullptr));
    }
    HIPCHECK(hipDeviceSynchronize());
    printf("prof workload done\n");
  }
  if (what == "ablate") {  // timing-only ablations of the 3A2B dequant-GEMM step (outputs are wrong by construction)
    const int64_t M = 4096, N = 4096, K = 4096;
    Packed W(N, K, 128, true);
    DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N);
    std::vector<uint16_t> hx(x.n);
    for (auto& v : hx) v = f2bf(rnd_normal());
    x.upload(hx);
    const int nv = 17, rounds = 5, iters = 8;
    const int modes[nv] = {0, 20, 21, 22, 23, 24, 25, 26, 6, 31, 32, 34, 37, 27, 28, 29, 30};
    const char* labels[nv] = {"full step", "- dequant arithmetic", "- ds_write of W", "- fragment reads", "- global loads + DMA", "- barrier",
                              "MFMA + barrier only", "MFMA only", "ping-pong full", "ping-pong - loads", "ping-pong - dequant/write",
                              "ping-pong - frag reads", "ping-pong MFMA+barriers", "- vmcnt waits only", "loads of K-tile 0 only",
                              "- the 6 W-side loads", "- the 4 x LDS-DMAs"};
    std::vector<std::vector<float>> ms(nv);
    Timer t;
    for (int i = 0; i < 10; ++i)
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
    for (int r = 0; r < rounds; ++r)
      for (int vi = 0; vi < nv; ++vi) {
        const int mi = (vi + r) % nv;
        inc_debug_set_small_tiles(modes[mi]);
        INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
        t.start();
        for (int i = 0; i < iters; ++i)
          INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
        ms[mi].push_back(t.stop_ms() / iters);
      }
    for (int mi = 0; mi < nv; ++mi) {
      std::sort(ms[mi].begin(), ms[mi].end());
      const float med = ms[mi][ms[mi].size() / 2];
      printf("ABLATE %-24s median %8.4f ms  (%7.1f TFLOP/s equivalent)  best %8.4f\n", labels[mi], med, 2.0 * M * N * K / med / 1e9, ms[mi][0]);
    }
    inc_debug_set_small_tiles(0);
  }
  if (what == "pcablate") {  // timing-only ablations of the producer / consumer dequant-GEMM step (outputs are wrong by construction)
    const int64_t M = 4096, N = 4096, K = 4096;
    Packed W(N, K, 128, true);
    DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N);
    std::vector<uint16_t> hx(x.n);
    for (auto& v : hx) v = f2bf(rnd_normal());
    x.upload(hx);
    const int nv = 24, rounds = 5, iters = 8;
    const int modes[nv] = {0, 40, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72};
    const char* labels[nv] = {"PC full step", "3A2B full step", "P: - dequant arithmetic", "P: - dequant - ds_write", "P: - x LDS-DMA", "P: - W loads",
                              "P: - all global traffic", "P: idle (no loads, no dequant)", "C: - fragment reads", "MFMA + barrier only",
                              "MFMA only", "C: - MFMA", "- barrier", "producers ALONE: full", "  alone - dequant arithmetic",
                              "  alone - dequant - ds_write", "  alone - x LDS-DMA", "  alone - W loads", "  alone - all global traffic",
                              "  alone: barriers only", "- epilogue stores", "consumers at s_setprio 2", "producers at s_setprio 2",
                              "prologue + barriers, no stores"};
    std::vector<std::vector<float>> ms(nv);
    Timer t;
    for (int i = 0; i < 10; ++i)
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
    for (int r = 0; r < rounds; ++r)
      for (int vi = 0; vi < nv; ++vi) {
        const int mi = (vi + r) % nv;
        inc_debug_set_small_tiles(modes[mi]);
        INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
        t.start();
        for (int i = 0; i < iters; ++i)
          INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
        ms[mi].push_back(t.stop_ms() / iters);
      }
    for (int mi = 0; mi < nv; ++mi) {
      std::sort(ms[mi].begin(), ms[mi].end());
      const float med = ms[mi][ms[mi].size() / 2];
      printf("PCABLATE %-32s median %8.4f ms  (%7.1f TFLOP/s equivalent)  best %8.4f\n", labels[mi], med, 2.0 * M * N * K / med / 1e9, ms[mi][0]);
    }
    inc_debug_set_small_tiles(0);
  }
  if (what == "pcfma") {  // producer / consumer kernel: v_pk_fma_f32 vs scalar v_fma_f32 in the dequantisation (same outputs required)
    const int64_t shapes[3][3] = {{4096, 4096, 4096}, {4096, 11008, 4096}, {4096, 4096, 11008}};
    for (int si = 0; si < 3; ++si) {
      const int64_t M = shapes[si][0], N = shapes[si][1], K = shapes[si][2];
      Packed W(N, K, 128, true);
      DevBuf<uint16_t> x((size_t)M * K), y((size_t)M * N), y2((size_t)M * N);
      std::vector<uint16_t> hx(x.n);
      for (auto& v : hx) v = f2bf(rnd_normal());
      x.upload(hx);
      inc_debug_set_small_tiles(0);
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
      inc_debug_set_small_tiles(73);
      INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y2.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
      HIPCHECK(hipDeviceSynchronize());
      std::vector<uint16_t> h1 = y.download(), h2 = y2.download();
      const bool same = memcmp(h1.data(), h2.data(), h1.size() * 2) == 0;
      if (!same) ++fails;
      const int modes[3] = {0, 73, 74};
      const char* labels[3] = {"v_fma_f32 x 8 (default)", "v_pk_fma_f32 x 4", "v_cvt_f32_fp8 x 8 + v_fma x 8"};
      std::vector<std::vector<float>> ms(3);
      Timer t;
      for (int r = 0; r < 7; ++r)
        for (int vi = 0; vi < 3; ++vi) {
          const int mi = (vi + r) % 3;
          inc_debug_set_small_tiles(modes[mi]);
          INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
          t.start();
          for (int i = 0; i < 8; ++i)
            INCCHECK(inc_woq_gemm(x.p, INC_BF16, W.qweight.p, W.scales.p, W.qzeros.p, nullptr, nullptr, y.p, M, N, K, W.G, 128, 4, nullptr, 0, nullptr));
          ms[mi].push_back(t.stop_ms() / 8);
        }
      printf("PCFMA M=%ld N=%ld K=%ld outputs %s\n", (long)M, (long)N, (long)K, same ? "bit-identical" : "DIFFER (FAIL)");
      for (int mi = 0; mi < 3; ++mi) {
        std::sort(ms[mi].begin(), ms[mi].end());
        const float med = ms[mi][ms[mi].size() / 2];
        printf("  %-30s median %8.4f ms %8.1f TFLOP/s\n", labels[mi], med, 2.0 * M * N * K / med / 1e9);
      }
      inc_debug_set_small_tiles(0);
    }
  }
  if (what == "probe") run_probe();
  printf("kbench: %d failing case(s)\n", fails);
  return fails ? 1 : 0;
}
