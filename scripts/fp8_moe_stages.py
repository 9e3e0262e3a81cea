"""Per-stage times of the fused FP8 and MXFP8 experts forwards on the Mixtral-8x7B shape at T = 1 and 16: every one of the six launches
on its own and the whole forward, device events, cold weights (512 MiB rewritten before every timed call), median of 9.  A companion of
scripts/fp8_moe_time.py: it shows which stage a difference between the two forwards comes from.  One process; run it under a time limit.

    timeout 280 python scripts/fp8_moe_stages.py | tee profiles/fp8/fp8_moe_stages.log
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd import ops  # noqa: E402
from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts  # noqa: E402
from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts  # noqa: E402
from scripts.moe_woq_time import SHAPES, _float_experts  # noqa: E402

dev = torch.device("cuda:0")
flush = torch.zeros((512 << 20) // 4, dtype=torch.int32, device=dev)
H, I, E, k = SHAPES["mixtral"]
fm = _float_experts(H, I, E, k, dev)
fp8 = FP8Experts.from_float(fm, device=dev)
mx = MXExperts.from_float(fm, "fp8_e4m3", "fp8_e4m3", device=dev)
del fm
torch.cuda.empty_cache()

def timed(fn, reps=9):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        flush.add_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)

for T in (1, 16):
    g = torch.Generator(device=dev).manual_seed(T)
    x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
    wts, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=g, device=dev), -1), k, dim=-1)
    wts = (wts / wts.sum(-1, keepdim=True)).to(torch.bfloat16)
    route = ops.moe_route(idx, E)
    xq, xs = ops.fp8_quant_rows(x, None, fp8.kp_h)
    h = ops.fp8_moe_gemm(0, xq, xs, route, fp8.gate_up_qweight, fp8.gate_up_w_scale, T, k, out_dtype=torch.bfloat16)
    hq, hs = ops.fp8_quant_rows(h, None, fp8.kp_i)
    y = ops.fp8_moe_gemm(1, hq, hs, route, fp8.down_qweight, fp8.down_w_scale, T, k, routing_weights=wts)
    mxq, mxs = ops.mx_quant(x, 0, mx.kp_h)
    mh = ops.mx_moe_gemm(0, mxq, mxs, 0, route, mx.gate_up_qweight, mx.gate_up_w_scale, 0, T, k, out_dtype=torch.bfloat16)
    mhq, mhs = ops.mx_quant(mh, 0, mx.kp_i)
    stages = {
        "route": lambda: ops.moe_route(idx, E),
        "fp8 quant x": lambda: ops.fp8_quant_rows(x, None, fp8.kp_h),
        "mx  quant x": lambda: ops.mx_quant(x, 0, mx.kp_h),
        "fp8 gemm 0": lambda: ops.fp8_moe_gemm(0, xq, xs, route, fp8.gate_up_qweight, fp8.gate_up_w_scale, T, k, out_dtype=torch.bfloat16),
        "mx  gemm 0": lambda: ops.mx_moe_gemm(0, mxq, mxs, 0, route, mx.gate_up_qweight, mx.gate_up_w_scale, 0, T, k, out_dtype=torch.bfloat16),
        "fp8 quant h": lambda: ops.fp8_quant_rows(h, None, fp8.kp_i),
        "mx  quant h": lambda: ops.mx_quant(mh, 0, mx.kp_i),
        "fp8 gemm 1": lambda: ops.fp8_moe_gemm(1, hq, hs, route, fp8.down_qweight, fp8.down_w_scale, T, k, routing_weights=wts),
        "mx  gemm 1": lambda: ops.mx_moe_gemm(1, mhq, mhs, 0, route, mx.down_qweight, mx.down_w_scale, 0, T, k, routing_weights=wts),
        "combine": lambda: ops.moe_combine(y, route, T, k, E, torch.bfloat16),
        "fp8 forward": lambda: fp8(x, idx, wts),
        "mx  forward": lambda: mx(x, idx, wts),
    }
    with torch.no_grad():
        for name, fn in stages.items():
            print(f"T {T:>3} {name:<12} {timed(fn):9.1f} us", flush=True)
