"""Host enqueue time of every prepared decode route: what Python spends per forward between the module's __call__ and the launch.

One small module or group per route -- plain 4-bit, 4-bit act_order, 3-bit plain and act_order, NF4 (inc_woq_gemm_lut), a q / k / v
group (woq_linear_group) and a gate / up pair (woq_gated_pair) -- at N = 256, K = 512, M = 1, bf16: so small that the device is never
the bound (the kernels take a few us and the queue stays short), and the figure is the cost of issuing the call.  Every route is
warmed up (the prepared call exists), then a host clock is read around CALLS back-to-back forwards, with one synchronise after the
window and none inside it; WINDOWS such windows per route, the median and the range are printed in us per call.

The figure moves with the machine's load and between processes: compare two trees by alternating fresh processes of each.
usage: python scripts/decode_host_time.py [--calls C] [--windows W]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd import ops  # noqa: E402
from neural_compressor_amd.torch.algorithms.weight_only import modules as W  # noqa: E402

dev = torch.device("cuda:0")
N, K, GS = 256, 512, 128


def int_module(bits, act_order, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = W.MI355XWeightOnlyLinear(K, N, bits=bits, group_size=GS, zp=True, g_idx=act_order, device=dev)
    codes = torch.randint(0, 1 << bits, (N, K), generator=gen, device=dev, dtype=torch.int32)
    zp = torch.randint(1, 1 << bits, (N, K // GS), generator=gen, device=dev, dtype=torch.int32)
    m.pack(codes, torch.rand(N, K // GS, generator=gen, device=dev) * 0.02 + 1e-3, zp, None,
           g_idx=torch.randperm(K, generator=gen, device=dev) if act_order else None)
    return m


def nf4_module(seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = W.MI355XWeightOnlyLinear(K, N, dtype="nf4", bits=4, group_size=GS, use_optimum_format=False, device=dev)
    m.pack(torch.randint(-8, 8, (N, K), generator=gen, device=dev, dtype=torch.int32),
           torch.rand(N, K // GS, generator=gen, device=dev) * 0.02 + 1e-3, None, None)
    return m


def routes():
    """(name, forward of one x, check that the prepared route served it)."""
    m4, m4a, m3, m3a, nf4 = int_module(4, False, 1), int_module(4, True, 2), int_module(3, False, 3), int_module(3, True, 4), nf4_module(5)
    qkv = [int_module(4, False, 10 + i) for i in range(3)]
    gate, up = int_module(4, False, 20), int_module(4, False, 21)
    gate.bias = up.bias = None  # (the gated launch takes modules without a bias)

    def single(m, cls, perm):
        return lambda: type(m.__dict__.get("_call")) is cls and (m.__dict__["_call"].ko is not None) == perm

    return [
        ("int4", m4, single(m4, ops.WoqGemmCall, False)),
        ("int4 act_order", m4a, single(m4a, ops.WoqGemmCall, True)),
        ("int3", m3, single(m3, ops.WoqGemvAnywCall, False)),
        ("int3 act_order", m3a, single(m3a, ops.WoqGemvAnywCall, True)),
        ("nf4 lut", nf4, single(nf4, ops.WoqGemmLutCall, False)),
        ("q/k/v group", lambda x: W.woq_linear_group(x, qkv), lambda: len(qkv[0].__dict__.get("_group_calls", ())) == 1),
        ("gate/up gated pair", lambda x: W.woq_gated_pair(x, gate, up), lambda: len(gate.__dict__.get("_gated_calls", ())) == 1),
    ]


def main(calls, windows):
    x = torch.randn(1, K, device=dev, dtype=torch.bfloat16)
    for name, fwd, served in routes():
        for _ in range(200):
            fwd(x)
        torch.cuda.synchronize()
        assert served(), f"{name}: the prepared route did not serve the call"
        t = []
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(calls):
                fwd(x)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t.append((t1 - t0) / calls * 1e6)
        print(f"host enqueue time  {name:20s} {N}x{K} bf16 M=1: {statistics.median(t):6.2f} us per call "
              f"(median of {windows} windows of {calls} calls, {min(t):.2f}-{max(t):.2f})", flush=True)


if __name__ == "__main__":
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default  # noqa: E731
    main(arg("--calls", 4000), arg("--windows", 7))
