"""Times of the FP8 per-token / per-channel cell next to the MXFP8 cell, the int8 per-token cell and bf16, on an MI355X.

  quantiser   inc_fp8_quant_rows against inc_sq_quant_act_token and inc_mx_quant (fp8) on the same bf16 input, with the share of the HBM
              peak on the algorithmic bytes;
  product     inc_fp8_gemm / inc_fp8_gemv against inc_mx_gemm / inc_mx_gemv (fp8, fp8), inc_w8a8_gemm_rowscale (which picks its own
              GEMV for few rows) and torch.mm in bf16;
  module      the forward of FP8Linear, MXLinear and W8A8Linear(act_quant="per_token") on the same fp16 input (quantiser + product).
Shapes: the Llama-2-13B linears (N, K) = (5120, 5120), (13824, 5120), (5120, 13824) at M = 1, 16, 4096.

Every call is timed by its own pair of device events.  Before each timed call a 512 MiB buffer is rewritten, outside the event pair, so
that operands come from HBM and not from L2 or the 256 MiB MALL ("cold").  The variants alternate inside one loop in one process and
their order rotates from pass to pass; the figure is the median over the loop.
usage: python scripts/fp8_gemm_time.py [--out profiles/fp8/fp8_gemm_time.log] [--iters-large 30] [--iters-small 100]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_compressor_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12         # bytes / s
FLUSH_BYTES = 512 << 20   # past L2 (8 x 4 MiB) and the 256 MiB MALL
FP8 = 0
SHAPES = ((5120, 5120), (13824, 5120), (5120, 13824))
ROWS = (1, 16, 4096)
dev = torch.device("cuda:0")
lines = []
L = _lib.lib


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def time_alternating(variants, iters, flush):
    """variants: {name: fn()} -> {name: median microseconds}.  One warm-up pass over every variant first."""
    names = list(variants)
    for k in names:
        variants[k]()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in variants}
    call = 0
    for it in range(iters):
        for j in range(len(names)):
            k = names[(it + j) % len(names)]
            flush.fill_(call & 0x7F)        # rewrite 512 MiB: nothing of the last call is left in a cache
            call += 1
            a, b = ev[k][it]
            a.record()
            variants[k]()
            b.record()
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in ev[k]) * 1e3 for k in variants}


def codes(rows, K):
    """Random e4m3 codes (no NaN code) and MX scale bytes 127."""
    q = torch.randint(0, 256, (rows, K), device=dev, dtype=torch.uint8)
    q[(q & 0x7F) == 0x7F] = 0
    return q, torch.full((rows, K // 32), 127, device=dev, dtype=torch.uint8)


def ok(rc):
    assert rc == 0, rc


def quantiser_section(flush, a):
    say("== quantiser: inc_fp8_quant_rows against inc_sq_quant_act_token and inc_mx_quant fp8 (bf16 input, cold, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for K in (5120, 13824):
        for M in ROWS:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            q8 = torch.empty(M, K, dtype=torch.uint8, device=dev)
            sc = torch.empty(M, K // 32, dtype=torch.uint8, device=dev)
            rs = torch.empty(M, dtype=torch.float32, device=dev)
            t = time_alternating({
                "fp8": lambda: ok(L.inc_fp8_quant_rows(x.data_ptr(), _lib.INC_BF16, M, K, K, None, q8.data_ptr(), rs.data_ptr(), stream)),
                "int8": lambda: ok(L.inc_sq_quant_act_token(x.data_ptr(), _lib.INC_BF16, M, K, K, None, q8.data_ptr(), rs.data_ptr(), stream)),
                "mxfp8": lambda: ok(L.inc_mx_quant(x.data_ptr(), _lib.INC_BF16, M, K, K, FP8, q8.data_ptr(), sc.data_ptr(), stream)),
            }, a.iters_large if M > 16 else a.iters_small, flush)
            by = M * K * 3 + 4 * M
            say(f"M={M:5d} K={K:5d}: fp8 per-token {t['fp8']:8.1f} us ({by / (t['fp8'] * 1e-6) / HBM_PEAK:6.3f} of HBM peak)   "
                f"int8 per-token {t['int8']:8.1f} us   mxfp8 {t['mxfp8']:8.1f} us   fp8 / int8 {t['fp8'] / t['int8']:.2f}   "
                f"fp8 / mxfp8 {t['fp8'] / t['mxfp8']:.2f}")


def product_section(flush, a):
    say()
    say("== product: inc_fp8_gemm (M = 4096) / inc_fp8_gemv (M <= 16) against the MXFP8 entry points of the same shape, "
        "inc_w8a8_gemm_rowscale and torch.mm bf16 (bf16 output, no bias, cold, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for M in ROWS:
        for N, K in SHAPES:
            w8, ws = codes(N, K)
            x8, xs = codes(M, K)
            wi = torch.randint(-127, 128, (N, K), device=dev, dtype=torch.int8)
            xi = torch.randint(-127, 128, (M, K), device=dev, dtype=torch.int8)
            wb = torch.randn(K, N, device=dev, dtype=torch.bfloat16)
            xb = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            alpha = torch.rand(N, device=dev) * 1e-4 + 1e-5
            rs = torch.rand(M, device=dev) * 1e-2 + 1e-3
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            need = L.inc_w8a8_gemm_workspace_bytes(M, N, K)
            wsp = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            fp8_fn, mx_fn = (L.inc_fp8_gemv, L.inc_mx_gemv) if M <= 16 else (L.inc_fp8_gemm, L.inc_mx_gemm)
            t = time_alternating({
                "fp8": lambda: ok(fp8_fn(x8.data_ptr(), rs.data_ptr(), w8.data_ptr(), alpha.data_ptr(), None, y.data_ptr(), _lib.INC_BF16,
                                         M, N, K, stream)),
                "mxfp8": lambda: ok(mx_fn(x8.data_ptr(), xs.data_ptr(), FP8, w8.data_ptr(), ws.data_ptr(), FP8, None, y.data_ptr(),
                                          _lib.INC_BF16, M, N, K, stream)),
                "int8": lambda: ok(L.inc_w8a8_gemm_rowscale(xi.data_ptr(), wi.data_ptr(), rs.data_ptr(), alpha.data_ptr(), None, y.data_ptr(),
                                                            _lib.INC_BF16, M, N, K, wsp.data_ptr(), need, stream)),
                "bf16": lambda: torch.mm(xb, wb, out=y),
            }, a.iters_large if M > 16 else a.iters_small, flush)
            ops_, by = 2.0 * M * N * K, (M + N) * K + 4 * (M + N) + 2 * M * N
            rate = (lambda k: f"{ops_ / (t[k] * 1e-6) / 1e12:7.1f} T/s") if M > 16 else (lambda k: f"{by / (t[k] * 1e-6) / HBM_PEAK:6.3f} of HBM peak")
            say(f"M={M:5d} N={N:5d} K={K:5d}: fp8 {t['fp8']:8.1f} us ({rate('fp8')})   mxfp8 {t['mxfp8']:8.1f} us   int8 {t['int8']:8.1f} us   "
                f"bf16 {t['bf16']:8.1f} us   fp8 / mxfp8 {t['fp8'] / t['mxfp8']:.2f}   fp8 / int8 {t['fp8'] / t['int8']:.2f}"
                + (f"   share of the mxfp8 - int8 gap closed {(t['mxfp8'] - t['fp8']) / (t['mxfp8'] - t['int8']):.2f}" if M > 16 else ""))
            del w8, ws, wi, wb


def module_section(flush, a):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    say()
    say("== module forward (quantiser + product, fp16 input and output, no bias, cold, median us) ==")
    for N, K in SHAPES:
        lin = torch.nn.Linear(K, N, bias=False).to(dev).half()
        mods = {"fp8": FP8Linear.from_float(lin, device=dev), "mxfp8": MXLinear.from_float(lin, device=dev),
                "int8": W8A8Linear.from_float(lin, device=dev, act_quant="per_token")}
        for M in ROWS:
            x = torch.randn(M, K, device=dev, dtype=torch.float16)
            with torch.no_grad():
                t = time_alternating({k: (lambda m=m: m(x)) for k, m in mods.items()} | {"fp16": lambda: lin(x)},
                                     a.iters_large if M > 16 else a.iters_small, flush)
            say(f"M={M:5d} N={N:5d} K={K:5d}: FP8Linear {t['fp8']:8.1f} us   MXLinear {t['mxfp8']:8.1f} us   W8A8Linear per-token "
                f"{t['int8']:8.1f} us   nn.Linear fp16 {t['fp16']:8.1f} us   fp8 / mxfp8 {t['fp8'] / t['mxfp8']:.2f}   fp8 / int8 {t['fp8'] / t['int8']:.2f}")
        del lin, mods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8", "fp8_gemm_time.log"))
    ap.add_argument("--iters-large", type=int, default=30)
    ap.add_argument("--iters-small", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    say(f"device: {torch.cuda.get_device_name(0)}; HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s; {FLUSH_BYTES >> 20} MiB rewritten before every timed call")
    flush = torch.empty(FLUSH_BYTES, dtype=torch.uint8, device=dev)
    quantiser_section(flush, a)
    product_section(flush, a)
    module_section(flush, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
