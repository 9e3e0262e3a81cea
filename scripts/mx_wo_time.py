"""Times of the weight-only MX cell (inc_mx_wo_gemv / inc_mx_wo_gemm: MXFP4 / MXFP8 weights against bf16 activations) on an MI355X,
against what such a checkpoint runs as without it and against the neighbouring cells, on the Llama-2-13B shapes:

  wo_fp4 / wo_fp8   the new kernels: the GEMV up to 16 rows, the tile GEMM above; at M <= 16 the tile GEMM too (gemm_fp4 / gemm_fp8),
                    which is the crossover MXWeightOnlyLinear.DECODE_MAX_M is set from;
  bf16              torch.mm on recover(bfloat16);
  mx_a8w4 / mx_a8w8 inc_mx_quant(x, fp8) + inc_mx_gemv / inc_mx_gemm (MX activations as well);
  int4              inc_woq_gemm, group size 128.

The method is scripts/mx_gemm_time.py's: every call timed by its own pair of device events, the variants alternating inside one loop
with a rotating order, every variant's weights from a ring of buffers larger than the caches ("cold"), the median over the loop.
usage: python scripts/mx_wo_time.py [--out profiles/mx/mx_wo_time.log]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from neural_compressor_amd import _lib, ops  # noqa: E402
import mx_gemm_time as T  # noqa: E402  (say, ring_len, time_alternating, codes)

FP8, FP4 = T.FP8, T.FP4
dev = T.dev
SHAPES = ((5120, 5120), (13824, 5120), (5120, 13824))
ROWS = (1, 16, 64, 512, 4096)


def section():
    T.say("== weight-only MX against torch.mm on recover(bf16), the MX cell with fp8 activations and INT4 g128 "
          "(bf16 output, no bias, cold weights, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for N, K in SHAPES:
        w8 = [T.codes(N, K, FP8) for _ in range(T.ring_len(N * K))]
        w4 = [T.codes(N, K, FP4) for _ in range(T.ring_len(N * K // 2))]
        wb = [torch.randn(K, N, device=dev, dtype=torch.bfloat16) for _ in range(T.ring_len(N * K * 2))]
        wi = [(torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), device=dev, dtype=torch.int32),
               (torch.rand(K // 128, N, device=dev) * 0.01 + 0.001).half(),
               torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 128, N // 8), device=dev, dtype=torch.int32)) for _ in range(T.ring_len(N * K // 2))]
        for M in ROWS:
            xb = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

            def wo(entry, ring, wf):
                f = getattr(_lib.lib, entry)

                def run(i):
                    w = ring[i % len(ring)]
                    rc = f(xb.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), wf, None, y.data_ptr(), _lib.INC_BF16, M, N, K, K, stream)
                    assert rc == 0, rc
                return run

            def mx(ring, wf):
                f = _lib.lib.inc_mx_gemv if M <= 16 else _lib.lib.inc_mx_gemm

                def run(i):
                    w = ring[i % len(ring)]
                    xq, xs = ops.mx_quant(xb, FP8, K)
                    rc = f(xq.data_ptr(), xs.data_ptr(), FP8, w[0].data_ptr(), w[1].data_ptr(), wf, None, y.data_ptr(), _lib.INC_BF16, M, N, K, stream)
                    assert rc == 0, rc
                return run

            def bf16(i):
                torch.mm(xb, wb[i % len(wb)], out=y)

            def int4(i):
                q, s, z = wi[i % len(wi)]
                ops.woq_gemm(xb, q, s, z, None, N, K, 128, 4)

            first = "inc_mx_wo_gemv" if M <= 16 else "inc_mx_wo_gemm"
            variants = {"wo_fp4": wo(first, w4, FP4), "wo_fp8": wo(first, w8, FP8), "bf16": bf16, "mx_a8w4": mx(w4, FP4),
                        "mx_a8w8": mx(w8, FP8), "int4": int4}
            if M <= 16:
                variants["gemm_fp4"] = wo("inc_mx_wo_gemm", w4, FP4)
                variants["gemm_fp8"] = wo("inc_mx_wo_gemm", w8, FP8)
            t = T.time_alternating(variants, 200 if M <= 64 else 40 if M <= 512 else 20)
            T.say(f"M={M:5d} N={N:5d} K={K:5d}: " + "   ".join(f"{k} {v:8.1f}" for k, v in t.items())
                  + f"   wo_fp4 / bf16 {t['wo_fp4'] / t['bf16']:.2f}   wo_fp8 / bf16 {t['wo_fp8'] / t['bf16']:.2f}   wo_fp4 / int4 {t['wo_fp4'] / t['int4']:.2f}"
                  + (f"   {2.0 * M * N * K / (t['wo_fp4'] * 1e-6) / 1e12:6.1f} T/s fp4" if M > 16 else
                     f"   {(N * K / 2 + N * K / 32) / (t['wo_fp4'] * 1e-6) / T.HBM_PEAK:5.3f} of HBM peak fp4"))
        del w8, w4, wb, wi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "mx_wo_time.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    T.say(f"device: {torch.cuda.get_device_name(0)}; HBM peak taken as {T.HBM_PEAK / 1e12:.1f} TB/s")
    section()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(T.lines) + "\n")


if __name__ == "__main__":
    main()
