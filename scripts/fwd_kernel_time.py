#!/usr/bin/env python
"""Time the three forward elementwise kernels (csrc/fwd_elementwise.hip) at the shapes of one stacked calibration forward of the
benchmark (65 536 tokens of Llama-2-7B, bf16) against the copy probe, in ONE process: HIP events over `--calls` calls per timing.

    python scripts/fwd_kernel_time.py --out kernel_time.json [--other-lib /path/to/another/libinc_mi355x.so]

With --other-lib the same three entry points of a second build of the library (say the parent commit's) are timed in the same process,
the two builds alternating in the order other, this, this, other -- twice -- so that every build has repeated timings of its own
(their spread is what a difference between the builds has to beat) and neither always runs first."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_compressor_amd import _lib, ops  # noqa: E402
from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff  # noqa: E402

TOKENS, HIDDEN, INTER, HEADS, HEAD_DIM, SEQ = 65536, 4096, 11008, 32, 128, 2048


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("inc_fwd_silu_mul", "inc_fwd_rope", "inc_fwd_rmsnorm"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    dt, code = torch.bfloat16, _lib.INC_BF16
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device=dev, dtype=torch.float32).to(dt)

    def stream():
        return torch.cuda.current_stream().cuda_stream

    # the copy ceiling: the best of the probe's 16 variants, 1 GiB read + 1 GiB written
    src, dst = torch.empty(1 << 30, dtype=torch.uint8, device=dev).random_(), torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    copy_ms = min(timed(lambda v=v: ops.probe_hbm_copy(dst, src, v), args.calls) for v in range(16))
    copy_gbs = 2 * (1 << 30) / copy_ms / 1e6
    del src, dst

    gate, up = rnd(TOKENS, INTER), rnd(TOKENS, INTER)
    out_mlp = torch.empty_like(gate)
    x, w = rnd(TOKENS, HIDDEN), rnd(HIDDEN)
    out_norm = torch.empty_like(x)
    B = TOKENS // SEQ
    q = rnd(B, SEQ, HEADS * HEAD_DIM).view(B, SEQ, HEADS, HEAD_DIM).transpose(1, 2)  # the views LlamaAttention hands over
    k = rnd(B, SEQ, HEADS * HEAD_DIM).view(B, SEQ, HEADS, HEAD_DIM).transpose(1, 2)
    ang = torch.rand(1, SEQ, HEAD_DIM, generator=g, device=dev) * 6.28
    cos, sin = ang.cos().to(dt), ang.sin().to(dt)
    qs, ks = ff._eager_rope_strides(q, k, cos, sin)
    q_out, k_out = torch.empty_strided(q.shape, qs, dtype=dt, device=dev), torch.empty_strided(k.shape, ks, dtype=dt, device=dev)
    strides = (ctypes.c_int64 * 12)(*q.stride()[:3], *k.stride()[:3], *qs[:3], *ks[:3])
    nbytes = {"silu_mul": 3 * gate.numel() * 2, "rmsnorm": 2 * x.numel() * 2, "rope": 2 * (q.numel() + k.numel()) * 2}

    def kernels(lib):
        def check(rc):
            assert rc == 0, rc

        return {
            "silu_mul": lambda: check(lib.inc_fwd_silu_mul(gate.data_ptr(), up.data_ptr(), out_mlp.data_ptr(), gate.numel(), code, stream())),
            "rmsnorm": lambda: check(lib.inc_fwd_rmsnorm(x.data_ptr(), w.data_ptr(), out_norm.data_ptr(), TOKENS, HIDDEN, 1e-5, code, stream())),
            "rope": lambda: check(lib.inc_fwd_rope(q.data_ptr(), k.data_ptr(), cos.data_ptr(), sin.data_ptr(), q_out.data_ptr(), k_out.data_ptr(),
                                                   B, HEADS, HEADS, SEQ, HEAD_DIM, strides, 1, code, stream())),
        }

    builds = {"this": kernels(bind(_lib.LIB_PATH))}
    order = ["this", "this"]
    if args.other_lib:
        builds["other"] = kernels(bind(args.other_lib))
        order = ["other", "this", "this", "other"] * 2
    runs = {name: {kn: [] for kn in nbytes} for name in builds}
    for name in order:
        for kn, fn in builds[name].items():
            runs[name][kn].append(round(timed(fn, args.calls), 4))
    result = {"shapes": f"{TOKENS} tokens, hidden {HIDDEN}, intermediate {INTER}, {HEADS} heads of {HEAD_DIM}, bf16", "calls_per_timing": args.calls,
              "order": order, "measured_hbm_copy_gbs": round(copy_gbs, 1), "bytes": nbytes}
    if args.other_lib:  # the two builds write the same bits
        outs = {"silu_mul": (out_mlp,), "rmsnorm": (out_norm,), "rope": (q_out, k_out)}
        result["outputs_equal"] = {}
        for kn in nbytes:
            builds["other"][kn]()
            kept = [t.clone() for t in outs[kn]]
            for t in outs[kn]:
                t.zero_()
            builds["this"][kn]()
            result["outputs_equal"][kn] = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(kept, outs[kn]))
    for name, per in runs.items():
        result[name] = {}
        for kn, ms in per.items():
            mean = sum(ms) / len(ms)
            gbs = nbytes[kn] / mean / 1e6
            result[name][kn] = {"ms": ms, "mean_ms": round(mean, 4), "spread_ms": round(max(ms) - min(ms), 4), "gbs": round(gbs, 1),
                                "of_copy_probe": round(gbs / copy_gbs, 3)}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
