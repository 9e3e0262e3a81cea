"""Times of the MX cell (MXFP8 / MXFP4 on the block-scaled matrix instruction) next to the int8 per-token cell and bf16, on an MI355X.

  quantiser   inc_mx_quant (fp8 and fp4 codes) against inc_sq_quant_act_token on the same bf16 input, M = 16 / 4096 at K = 5120 / 13824,
              with the share of the HBM peak on the algorithmic bytes;
  GEMM        inc_mx_gemm for (act, weight) = (fp8, fp8), (fp8, fp4), (fp4, fp4) against inc_w8a8_gemm_rowscale (the int8 launch: the same
              MFMA rate and the same operand bytes as MXFP8) and torch.mm in bf16, on the Llama-2-13B shapes at M = 4096 and M = 16.

Every call is timed by its own pair of device events; the variants alternate inside one loop and their order rotates from pass to pass;
every variant takes its weights from a ring of buffers of its own that is larger than the caches ("cold"), the quantiser its input.
The figure is the median over the loop.
usage: python scripts/mx_gemm_time.py [--out profiles/mx/mx_gemm_time.log]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_compressor_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s
COLD_BYTES = 768 << 20   # a ring at least this large: well past L2 (8 x 4 MiB) and the 256 MiB MALL
FP8, FP4 = 0, 4
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def ring_len(nbytes):
    return max(2, -(-COLD_BYTES // max(nbytes, 1)))


def time_alternating(variants, iters):
    """variants: {name: fn(call number)} -> {name: median microseconds}.  One warm-up pass over every variant first."""
    names = list(variants)
    call = 0
    for k in names:
        variants[k](call)
        call += 1
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in variants}
    for it in range(iters):
        for j in range(len(names)):
            k = names[(it + j) % len(names)]
            a, b = ev[k][it]
            a.record()
            variants[k](call)
            call += 1
            b.record()
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in ev[k]) * 1e3 for k in variants}


def codes(rows, K, fmt):
    """Random codes as inc_mx_quant stores them (no e4m3 NaN code) and scale bytes around 2^0."""
    q = torch.randint(0, 256, (rows, K if fmt == FP8 else K // 2), device=dev, dtype=torch.uint8)
    if fmt == FP8:
        q[(q & 0x7F) == 0x7F] = 0
    return q, torch.randint(120, 135, (rows, K // 32), device=dev, dtype=torch.uint8)


def quantiser_section():
    say("== quantiser: inc_mx_quant against inc_sq_quant_act_token (bf16 input, cold, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for K in (5120, 13824):
        for M in (16, 4096):
            n = ring_len(M * K * 2) if M > 16 else 64
            xs = [torch.randn(M, K, device=dev, dtype=torch.bfloat16) for _ in range(n)]
            q8 = torch.empty(M, K, dtype=torch.uint8, device=dev)
            sc = torch.empty(M, K // 32, dtype=torch.uint8, device=dev)
            rs = torch.empty(M, dtype=torch.float32, device=dev)

            def mx(fmt):
                def run(i):
                    _lib.check(_lib.lib.inc_mx_quant(xs[i % n].data_ptr(), _lib.INC_BF16, M, K, K, fmt, q8.data_ptr(), sc.data_ptr(), stream), "mx")
                return run

            def token(i):
                _lib.check(_lib.lib.inc_sq_quant_act_token(xs[i % n].data_ptr(), _lib.INC_BF16, M, K, K, None, q8.data_ptr(), rs.data_ptr(), stream), "token")

            t = time_alternating({"mxfp8": mx(FP8), "mxfp4": mx(FP4), "int8_token": token}, 200 if M <= 16 else 60)
            b8, b4, bi = M * K * 2 + M * K + M * K // 32, M * K * 2 + M * K // 2 + M * K // 32, M * K * 2 + M * K + 4 * M
            say(f"M={M:5d} K={K:5d}: mxfp8 {t['mxfp8']:8.1f} us ({b8 / (t['mxfp8'] * 1e-6) / HBM_PEAK:6.3f} of HBM peak)   "
                f"mxfp4 {t['mxfp4']:8.1f} us ({b4 / (t['mxfp4'] * 1e-6) / HBM_PEAK:6.3f})   "
                f"int8 per-token {t['int8_token']:8.1f} us ({bi / (t['int8_token'] * 1e-6) / HBM_PEAK:6.3f})   "
                f"mxfp8 / int8 {t['mxfp8'] / t['int8_token']:.2f}")
            del xs


def gemm_section():
    say()
    say("== GEMM: inc_mx_gemm against inc_w8a8_gemm_rowscale and torch.mm bf16 (bf16 output, no bias, cold weights, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for M in (4096, 16):
        for N, K in ((5120, 5120), (13824, 5120), (5120, 13824)):
            n8, n4, nb = ring_len(N * K), ring_len(N * K // 2), ring_len(N * K * 2)
            w8 = [codes(N, K, FP8) for _ in range(n8)]
            w4 = [codes(N, K, FP4) for _ in range(n4)]
            wi = [torch.randint(-127, 128, (N, K), device=dev, dtype=torch.int8) for _ in range(n8)]
            wb = [torch.randn(K, N, device=dev, dtype=torch.bfloat16) for _ in range(nb)]
            x8, x4 = codes(M, K, FP8), codes(M, K, FP4)
            xi = torch.randint(-127, 128, (M, K), device=dev, dtype=torch.int8)
            xb = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            alpha = torch.rand(N, device=dev) * 1e-4 + 1e-5
            rs = torch.rand(M, device=dev) * 1e-2 + 1e-3
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            need = _lib.lib.inc_w8a8_gemm_workspace_bytes(M, N, K)
            wsp = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

            def mx(x, xf, ring, wf):
                def run(i):
                    w = ring[i % len(ring)]
                    rc = _lib.lib.inc_mx_gemm(x[0].data_ptr(), x[1].data_ptr(), xf, w[0].data_ptr(), w[1].data_ptr(), wf, None, y.data_ptr(),
                                              _lib.INC_BF16, M, N, K, stream)
                    assert rc == 0, rc
                return run

            def int8(i):
                rc = _lib.lib.inc_w8a8_gemm_rowscale(xi.data_ptr(), wi[i % n8].data_ptr(), rs.data_ptr(), alpha.data_ptr(), None, y.data_ptr(),
                                                     _lib.INC_BF16, M, N, K, wsp.data_ptr(), need, stream)
                assert rc == 0, rc

            def bf16(i):
                torch.mm(xb, wb[i % nb], out=y)

            t = time_alternating({"a8w8": mx(x8, FP8, w8, FP8), "a8w4": mx(x8, FP8, w4, FP4), "a4w4": mx(x4, FP4, w4, FP4), "int8": int8,
                                  "bf16": bf16}, 40 if M > 16 else 200)
            ops_ = 2.0 * M * N * K
            say(f"M={M:5d} N={N:5d} K={K:5d}: " + "   ".join(
                f"{k} {t[k]:8.1f} us ({ops_ / (t[k] * 1e-6) / 1e12:7.1f} T/s)" for k in ("a8w8", "a8w4", "a4w4", "int8", "bf16"))
                + f"   a8w8 / int8 {t['a8w8'] / t['int8']:.2f}   a4w4 / a8w8 {t['a4w4'] / t['a8w8']:.2f}")
            del w8, w4, wi, wb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "mx_gemm_time.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    say(f"device: {torch.cuda.get_device_name(0)}; HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s")
    quantiser_section()
    gemm_section()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
