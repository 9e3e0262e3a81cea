"""Time one MoE experts layer forward with MX experts on the MI355X: device events, cold weights (a buffer larger than the last-level
cache is rewritten before every timed call), the variants alternating inside one process, median of the repeats.

Variants, same inputs and routing (softmax top-k of random logits), per (w_dtype, act_dtype) pair:
  fused   MXExperts' fused route (route -> quantise x -> gate_up -> quantise h -> down -> combine, no host wait)
  dense   MXExperts with MOE_FUSED = False (per expert that was hit: quantise, inc_mx_gemv / inc_mx_gemm, host waits)
  int4    MI355XWeightOnlyExperts INT4 g32 on the same shape (its fused route)
  bf16    transformers' own experts module with bf16 weights (eager forward)
`bytes` is what the fused route must stream at least: the codes and scale bytes of the experts that were hit, plus x, the intermediate
and the output; `hbm` is that over the fused time as a fraction of 8 TB/s.

The last lines print the MOE_MAX_ROWS the rule gives: the largest measured rows-per-expert average (T k / E) up to which the fused
route is not slower than the dense route at every measured point of both shapes and all pairs.

    python scripts/mx_moe_time.py [--shapes mixtral,qwen3] [--ts 1,16,64,256,1024,4096] [--log profiles/mx/mx_moe_time.log]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.moe_woq_time import PEAK, SHAPES, _float_experts  # noqa: E402

PAIRS = (("fp8_e4m3", "fp8_e4m3"), ("fp4", "fp8_e4m3"), ("fp4", "fp4"))  # (w_dtype, act_dtype)
FLUSH_BYTES = 512 << 20


def _alternating(fns, reps, flush):
    """Median time in us of every fn of `fns` (a dict), one call of each per repeat, the caches flushed before every call."""
    times = {name: [] for name in fns}
    for name, fn in fns.items():  # warm-up: allocations, first-call setup
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in fns.items():
            flush.add_(1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    return {name: statistics.median(v) for name, v in times.items()}


def main():
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts
    from neural_compressor_amd.torch.algorithms.weight_only.experts import quantize_experts

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mixtral,qwen3")
    ap.add_argument("--ts", default="1,16,64,256,1024,4096")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    log = open(args.log, "w") if args.log else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    dev = torch.device("cuda:0")
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device=dev)
    ts = [int(t) for t in args.ts.split(",")]
    points = []  # (rows per expert, fused <= dense)
    say(f"device {torch.cuda.get_device_name(0)}; medians in us, weights cold ({FLUSH_BYTES >> 20} MiB rewritten before every call)")
    for shape in args.shapes.split(","):
        H, I, E, k = SHAPES[shape]
        fm = _float_experts(H, I, E, k, dev)
        int4 = quantize_experts(fm, dict(group_size=32, scheme="sym"), dev)
        int4.MOE_MAX_ROWS = 1 << 30
        mx = {}
        for w_dtype, act_dtype in PAIRS:
            m = MXExperts.from_float(fm, w_dtype, act_dtype, device=dev)
            m.MOE_MAX_ROWS = 1 << 30  # this script times the fused route at every T
            mx[(w_dtype, act_dtype)] = m
        say(f"== {shape}: H {H} I {I} E {E} k {k}")
        say(f"{'pair (w, act)':>20} {'T':>5} {'rows/E':>7} {'active':>6} {'bytes MB':>9} {'fused':>9} {'dense':>9} {'int4':>9} {'bf16':>9} "
            f"{'hbm':>6} {'vs dense':>8} {'vs int4':>7} {'vs bf16':>7}")
        for T in ts:
            g = torch.Generator(device=dev).manual_seed(T)
            x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
            wts, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=g, device=dev), -1), k, dim=-1)
            wts = (wts / wts.sum(-1, keepdim=True)).to(torch.bfloat16)
            active = int(torch.unique(idx).numel())
            reps = 9 if T <= 256 else 5
            for pair, m in mx.items():
                per_expert = sum(b[0].numel() for b in m.buffers())
                a_bytes = 1 if pair[1] == "fp8_e4m3" else 0.5
                nbytes = active * per_expert + T * H * 2 + T * (H + H / 32) * a_bytes + T * k * (I * 2 + I * a_bytes + H * 4) + T * H * 2

                def route(fused, m=m):
                    m.MOE_FUSED = fused
                    return m(x, idx, wts)

                fns = {"fused": lambda: route(True), "dense": lambda: route(False)}
                if pair == PAIRS[0]:  # the references do not depend on the pair: timed once per T
                    fns.update(int4=lambda: int4(x, idx, wts), bf16=lambda: fm(x, idx, wts))
                with torch.no_grad():
                    t = _alternating(fns, reps, flush)
                m.MOE_FUSED = True
                if pair == PAIRS[0]:
                    t_int4, t_bf16 = t["int4"], t["bf16"]
                rows = T * k / E
                points.append((rows, t["fused"] <= t["dense"], shape, pair))
                say(f"{pair[0] + ', ' + pair[1]:>20} {T:>5} {rows:>7.2f} {active:>6} {nbytes / 1e6:>9.1f} {t['fused']:>9.1f} {t['dense']:>9.1f} "
                    f"{t_int4:>9.1f} {t_bf16:>9.1f} {nbytes / (t['fused'] * 1e-6) / PEAK:>6.3f} {t['dense'] / t['fused']:>7.2f}x "
                    f"{t_int4 / t['fused']:>6.2f}x {t_bf16 / t['fused']:>6.2f}x")
        del fm, int4, mx
        torch.cuda.empty_cache()
    # the rule: the largest measured rows-per-expert average r such that fused <= dense at every measured point with rows <= r
    best = None
    for r in sorted({p[0] for p in points}):
        if all(ok for rows, ok, _, _ in points if rows <= r):
            best = r
        else:
            break
    lost = [(rows, shape, pair) for rows, ok, shape, pair in points if not ok]
    say(f"points where the dense route is faster: {lost if lost else 'none'}")
    say(f"rule: MOE_MAX_ROWS = {best if best is None else format(best, 'g')} (largest measured rows-per-expert average up to which fused <= dense "
        f"on both shapes and all pairs); shipped MXExperts.MOE_MAX_ROWS = {MXExperts.MOE_MAX_ROWS}")


if __name__ == "__main__":
    main()
