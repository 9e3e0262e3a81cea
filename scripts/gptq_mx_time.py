"""Times of the GPTQ column loop on the MX grid (inc_gptq_quantize_layer_mx, MXFP4 / MXFP8) beside the integer loop it is built
from (inc_gptq_quantize_layer, bits=4, group_size=32, sym, the scales found inside the chain) on an MI355X, on the Llama-2-7B shapes
(o_proj, stacked q/k/v, stacked gate/up, down_proj), in one process.

Every variant restores its fp32 working copy from the same weights (the loop consumes it), then runs the whole loop with the
look-ahead stream the product uses; `copy` is that restore alone.  The factor is synthetic (unit diagonal, small upper triangle): the
time of the loop does not depend on the values.  The method is scripts/mx_gemm_time.py's: every call timed by its own pair of device
events, the variants alternating inside one loop with a rotating order, the median over the loop.
usage: python scripts/gptq_mx_time.py [--out profiles/mx/gptq_mx_time.log]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from neural_compressor_amd import ops  # noqa: E402
import mx_gemm_time as T  # noqa: E402  (say, time_alternating, lines)

dev = T.dev
SHAPES = (("o_proj", 4096, 4096), ("q/k/v", 12288, 4096), ("gate/up", 22016, 4096), ("down_proj", 4096, 11008))


def section(iters):
    T.say("== GPTQ column loop, one layer: integer (4 bit, groups of 32, sym) against MXFP4 / MXFP8 (fp32 Q, look-ahead on, median ms) ==")
    side = torch.cuda.Stream(device=dev)
    for name, N, K in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        w0 = torch.randn(N, K, device=dev, generator=g) * 0.02
        hinv = (torch.triu(torch.randn(K, K, device=dev, generator=g), 1) * (0.05 / K ** 0.5) + torch.eye(K, device=dev)).contiguous()
        w, Q = torch.empty_like(w0), torch.empty_like(w0)
        err_ws = torch.empty((2, N, 128), device=dev)
        scale, zero = torch.empty((N, K // 32), device=dev), torch.empty((N, K // 32), device=dev)
        codes = torch.empty((N, K), dtype=torch.uint8, device=dev)

        def copy(i):
            w.copy_(w0)

        def integer(i):
            w.copy_(w0)
            ops.gptq_quantize_layer(w, hinv, scale, zero, None, None, codes, Q, err_ws, 32, 32, 128, 4, True, ops.GPTQ_DYNAMIC_GROUPS,
                                    aux_stream=side)

        def mx(fmt):
            def run(i):
                w.copy_(w0)
                ops.gptq_quantize_layer_mx(w, hinv, Q, err_ws, fmt, aux_stream=side)
            return run

        t = T.time_alternating({"copy": copy, "int4_g32": integer, "mx_fp4": mx(ops.MX_FP4_E2M1), "mx_fp8": mx(ops.MX_FP8_E4M3)}, iters)
        loop = {k: (v - t["copy"]) / 1e3 for k, v in t.items() if k != "copy"}
        T.say(f"{name:9s} N={N:5d} K={K:5d}: copy {t['copy'] / 1e3:7.3f}   " + "   ".join(f"{k} {v:8.3f}" for k, v in loop.items())
              + f"   mx_fp4 / int4 {loop['mx_fp4'] / loop['int4_g32']:.3f}   mx_fp8 / int4 {loop['mx_fp8'] / loop['int4_g32']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "gptq_mx_time.log"))
    ap.add_argument("--iters", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    T.say(f"device: {torch.cuda.get_device_name(0)}")
    section(a.iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(T.lines) + "\n")


if __name__ == "__main__":
    main()
