"""Times of the MXFP6 linears (inc_mx_quant_fp6, inc_mx_gemv, inc_mx_gemm with e2m3 operands) beside MXFP8 and MXFP4 in the same
run, on an MI355X: the Llama-2-13B shapes at M = 1, 16 (decode GEMV and, for the route rule, the tile kernel) and 4096 (tile kernel).

The method is scripts/mx_gemm_time.py's (its time_alternating and its cold rings): one device-event pair per call, the variants
alternating in one loop with rotating order, weights from a ring of >= 768 MiB of distinct buffers, the median over the loop.
A row where an fp6 pair is slower than MXFP8 is marked with `<< fp6 slower than fp8`.
usage: python scripts/mx_fp6_time.py [--out profiles/mx/mx_fp6_time.log]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_gemm_time as T  # noqa: E402  (puts the repository root on sys.path)
from neural_compressor_amd import _lib  # noqa: E402

FP8, E2M3, FP4 = 0, 2, 4
PAIRS = {"a8w8": (FP8, FP8), "a8w6": (FP8, E2M3), "a6w6": (E2M3, E2M3), "a4w4": (FP4, FP4)}   # (activation, weight)
SHAPES = ((5120, 5120), (13824, 5120), (5120, 13824))
dev, say = T.dev, T.say


def row_bytes(K, fmt):
    return {FP8: K, E2M3: K // 4 * 3, FP4: K // 2}[fmt]


def codes(rows, K, fmt):
    """Random codes in the format's storage (any six bits are an fp6 value) and scale bytes around 2^0."""
    if fmt != E2M3:
        return T.codes(rows, K, fmt)
    return (torch.randint(0, 256, (rows, row_bytes(K, fmt)), device=dev, dtype=torch.uint8),
            torch.randint(120, 135, (rows, K // 32), device=dev, dtype=torch.uint8))


def operand_bytes(rows, K, fmt):
    return rows * row_bytes(K, fmt) + rows * K // 32


def quantiser_section():
    say("== quantiser: inc_mx_quant_fp6 (e2m3) beside inc_mx_quant (fp8, fp4) (bf16 input, cold, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for K in (5120, 13824):
        for M in (1, 16, 4096):
            n = T.ring_len(M * K * 2) if M > 16 else 64
            xs = [torch.randn(M, K, device=dev, dtype=torch.bfloat16) for _ in range(n)]
            out = {f: codes(M, K, f) for f in (FP8, E2M3, FP4)}

            def quant(fmt):
                fn = _lib.lib.inc_mx_quant_fp6 if fmt == E2M3 else _lib.lib.inc_mx_quant

                def run(i):
                    rc = fn(xs[i % n].data_ptr(), _lib.INC_BF16, M, K, K, fmt, out[fmt][0].data_ptr(), out[fmt][1].data_ptr(), stream)
                    assert rc == 0, rc
                return run

            t = T.time_alternating({"fp8": quant(FP8), "fp6": quant(E2M3), "fp4": quant(FP4)}, 200)
            cells = [f"{k} {t[k]:7.1f} us ({(2 * M * K + operand_bytes(M, K, f)) / (t[k] * 1e-6) / T.HBM_PEAK:5.3f} of HBM peak)"
                     for k, f in (("fp8", FP8), ("fp6", E2M3), ("fp4", FP4))]
            say(f"M={M:4d} K={K:5d}: " + "   ".join(cells) + ("   << fp6 slower than fp8" if t["fp6"] > t["fp8"] else ""))


def product_section():
    say()
    say("== products: inc_mx_gemv (M <= 16) and inc_mx_gemm per pair (bf16 output, no bias, cold weights, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    tile_wins = []
    for N, K in SHAPES:
        ring = {f: [codes(N, K, f) for _ in range(T.ring_len(N * row_bytes(K, f)))] for f in (FP8, E2M3, FP4)}
        for M in (1, 16, 4096):
            x = {f: codes(M, K, f) for f in (FP8, E2M3, FP4)}
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

            def mx(entry, xf, wf):
                fn, xq, w = getattr(_lib.lib, entry), x[xf], ring[wf]

                def run(i):
                    wq = w[i % len(w)]
                    rc = fn(xq[0].data_ptr(), xq[1].data_ptr(), xf, wq[0].data_ptr(), wq[1].data_ptr(), wf, None, y.data_ptr(), _lib.INC_BF16,
                            M, N, K, stream)
                    assert rc == 0, rc
                return run

            variants = {}
            for name, (xf, wf) in PAIRS.items():
                variants["gemm_" + name] = mx("inc_mx_gemm", xf, wf)
                if M <= 16:
                    variants["gemv_" + name] = mx("inc_mx_gemv", xf, wf)
            t = T.time_alternating(variants, 200 if M <= 16 else 60)
            cells = []
            for name, (xf, wf) in PAIRS.items():
                gm = t["gemm_" + name]
                if M <= 16:
                    gv = t["gemv_" + name]
                    nbytes = operand_bytes(N, K, wf) + operand_bytes(M, K, xf) + 2 * M * N
                    cells.append(f"{name} gemv {gv:7.1f} us ({nbytes / (gv * 1e-6) / T.HBM_PEAK:5.3f} of HBM peak) gemm {gm:7.1f} us")
                    if "6" in name and gm < gv:
                        tile_wins.append((M, N, K, name))
                else:
                    cells.append(f"{name} gemm {gm:8.1f} us ({2 * M * N * K / (gm * 1e-6) / 1e15:5.3f} Pflop/s)")
            key = "gemv_" if M <= 16 else "gemm_"
            slower = [n for n in ("a8w6", "a6w6") if t[key + n] > t[key + "a8w8"]]
            say(f"M={M:4d} N={N:5d} K={K:5d}: " + "   ".join(cells) + (f"   << fp6 slower than fp8: {', '.join(slower)}" if slower else ""))
        del ring
    say()
    say("== route rule: MXLinear.DECODE_GEMV stays the route for <= 16 rows unless the tile kernel wins a decode row of an fp6 pair ==")
    say("the tile kernel wins: " + (", ".join(f"M={m} N={n} K={k} {p}" for m, n, k, p in tile_wins) if tile_wins else "no decode row"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "mx", "mx_fp6_time.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    say(f"device: {torch.cuda.get_device_name(0)}; HBM peak taken as {T.HBM_PEAK / 1e12:.1f} TB/s")
    quantiser_section()
    product_section()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(T.lines) + "\n")


if __name__ == "__main__":
    main()
