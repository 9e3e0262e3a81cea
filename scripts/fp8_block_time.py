"""Times of the block-scaled FP8 cell (128 x 128 weight blocks, 1 x 128 activation groups) next to the per-token cell, on an MI355X.

  quantisers  inc_fp8_quant_groups and inc_fp8_quant_blocks against inc_fp8_quant_rows on the same bf16 input;
  product     inc_fp8_block_gemm (M = 4096) / inc_fp8_block_gemv (M <= 16) against inc_fp8_gemm / inc_fp8_gemv on the SAME codes, and
              both against what a user of such a checkpoint has today: FP8BlockLinear.recover() to bf16, then torch.mm (the dequantisation
              is timed with the product: the checkpoint holds fp8, a bf16 copy kept around would double its memory; "mm" alone is
              the product on a bf16 copy that is already there);
  module      the forward of FP8BlockLinear next to FP8Linear (quantiser + product).
Shapes, timing, cold operands and alternation: scripts/fp8_gemm_time.py, whose helpers this script runs.
usage: python scripts/fp8_block_time.py [--out profiles/fp8/fp8_block_time.log] [--iters-large 30] [--iters-small 100]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_gemm_time as T  # noqa: E402  (say, time_alternating, codes, ok, SHAPES, ROWS; puts the repository root on sys.path)
from neural_compressor_amd import _lib  # noqa: E402

L, dev, say, BF16 = _lib.lib, T.dev, T.say, _lib.INC_BF16


def quantiser_section(flush, a):
    say("== quantisers: inc_fp8_quant_groups / inc_fp8_quant_blocks against inc_fp8_quant_rows (bf16 input, cold, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for K in (5120, 13824):
        for M in T.ROWS + (5120,):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            q8 = torch.empty(M, K, dtype=torch.uint8, device=dev)
            sc = torch.empty(M * (K // 128), dtype=torch.float32, device=dev)
            t = T.time_alternating({
                "rows": lambda: T.ok(L.inc_fp8_quant_rows(x.data_ptr(), BF16, M, K, K, None, q8.data_ptr(), sc.data_ptr(), stream)),
                "groups": lambda: T.ok(L.inc_fp8_quant_groups(x.data_ptr(), BF16, M, K, K, q8.data_ptr(), sc.data_ptr(), stream)),
                "blocks": lambda: T.ok(L.inc_fp8_quant_blocks(x.data_ptr(), BF16, M, K, K, q8.data_ptr(), sc.data_ptr(), stream)),
            }, a.iters_large if M > 16 else a.iters_small, flush)
            by = M * K * 3
            say(f"rows={M:5d} K={K:5d}: groups {t['groups']:8.1f} us ({by / (t['groups'] * 1e-6) / T.HBM_PEAK:6.3f} of HBM peak)   blocks "
                f"{t['blocks']:8.1f} us ({by / (t['blocks'] * 1e-6) / T.HBM_PEAK:6.3f})   per-row {t['rows']:8.1f} us   groups / per-row "
                f"{t['groups'] / t['rows']:.2f}   blocks / per-row {t['blocks'] / t['rows']:.2f}")


def product_section(flush, a):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear

    say()
    say("== product: inc_fp8_block_gemm (M = 4096) / inc_fp8_block_gemv (M <= 16) against the per-token entry points on the same codes and "
        "against recover() + torch.mm in bf16 (bf16 output, no bias, cold, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for M in T.ROWS:
        for N, K in T.SHAPES:
            w8, x8 = T.codes(N, K)[0], T.codes(M, K)[0]
            m = FP8BlockLinear(K, N, device=dev, float_type=torch.bfloat16)
            m.qweight.copy_(w8)
            m.w_scale.copy_(torch.rand(m.w_scale.shape, device=dev) * 1e-4 + 1e-5)
            xs = torch.rand(M, K // 128, device=dev) * 1e-2 + 1e-3
            alpha, rs = torch.rand(N, device=dev) * 1e-4 + 1e-5, xs[:, 0].contiguous()
            xb, wb = torch.randn(M, K, device=dev, dtype=torch.bfloat16), m.recover(torch.bfloat16).T.contiguous()
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            blk, tok = (L.inc_fp8_block_gemv, L.inc_fp8_gemv) if M <= 16 else (L.inc_fp8_block_gemm, L.inc_fp8_gemm)
            t = T.time_alternating({
                "block": lambda: T.ok(blk(x8.data_ptr(), xs.data_ptr(), w8.data_ptr(), m.w_scale.data_ptr(), None, y.data_ptr(), BF16, M, N, K, stream)),
                "token": lambda: T.ok(tok(x8.data_ptr(), rs.data_ptr(), w8.data_ptr(), alpha.data_ptr(), None, y.data_ptr(), BF16, M, N, K, stream)),
                "deq_mm": lambda: torch.mm(xb, m.recover(torch.bfloat16).T, out=y),
                "mm": lambda: torch.mm(xb, wb, out=y),
            }, a.iters_large if M > 16 else a.iters_small, flush)
            rate = f"{2.0 * M * N * K / (t['block'] * 1e-6) / 1e12:7.1f} T/s" if M > 16 else \
                f"{((M + N) * K + 2 * M * N) / (t['block'] * 1e-6) / T.HBM_PEAK:6.3f} of HBM peak"
            say(f"M={M:5d} N={N:5d} K={K:5d}: block {t['block']:8.1f} us ({rate})   per-token {t['token']:8.1f} us   recover + mm bf16 "
                f"{t['deq_mm']:8.1f} us   mm bf16 alone {t['mm']:8.1f} us   block / per-token {t['block'] / t['token']:.2f}   "
                f"block / (recover + mm) {t['block'] / t['deq_mm']:.2f}   block / mm {t['block'] / t['mm']:.2f}")
            del m, w8, wb


def module_section(flush, a):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear, FP8Linear

    say()
    say("== module forward (quantiser + product, bf16 input and output, no bias, cold, median us) ==")
    for N, K in T.SHAPES:
        lin = torch.nn.Linear(K, N, bias=False).to(dev).to(torch.bfloat16)
        mods = {"block": FP8BlockLinear.from_float(lin, device=dev), "token": FP8Linear.from_float(lin, device=dev), "bf16": lin}
        for M in T.ROWS:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            with torch.no_grad():
                t = T.time_alternating({k: (lambda m=m: m(x)) for k, m in mods.items()}, a.iters_large if M > 16 else a.iters_small, flush)
            say(f"M={M:5d} N={N:5d} K={K:5d}: FP8BlockLinear {t['block']:8.1f} us   FP8Linear {t['token']:8.1f} us   nn.Linear bf16 "
                f"{t['bf16']:8.1f} us   block / per-token {t['block'] / t['token']:.2f}   block / bf16 {t['block'] / t['bf16']:.2f}")
        del lin, mods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "fp8", "fp8_block_time.log"))
    ap.add_argument("--iters-large", type=int, default=30)
    ap.add_argument("--iters-small", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    say(f"device: {torch.cuda.get_device_name(0)}; HBM peak taken as {T.HBM_PEAK / 1e12:.1f} TB/s; {T.FLUSH_BYTES >> 20} MiB rewritten before every timed call")
    flush = torch.empty(T.FLUSH_BYTES, dtype=torch.uint8, device=dev)
    quantiser_section(flush, a)
    product_section(flush, a)
    module_section(flush, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(T.lines) + "\n")


if __name__ == "__main__":
    main()
