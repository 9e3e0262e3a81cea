"""Time one MoE experts layer forward with FP8 experts on the MI355X: device events, cold weights (a buffer larger than the last-level
cache is rewritten before every timed call), the variants alternating inside one process, median of the repeats.

Variants, same inputs and routing (softmax top-k of random logits):
  fused   FP8Experts' fused route (route -> quantise x -> gate_up -> quantise h -> down -> combine, no host wait)
  dense   FP8Experts with MOE_FUSED = False (per expert that was hit: quantise, inc_fp8_gemv / inc_fp8_gemm, host waits)
  mxfp8   MXExperts (fp8_e4m3, fp8_e4m3), its fused route
  int4    MI355XWeightOnlyExperts INT4 g32 on the same shape (its fused route)
`bytes` is what the fused route must stream at least: the codes and scales of the experts that were hit, plus x, the intermediate and
the output; `hbm` is that over the fused time as a fraction of 8 TB/s.

The driver process does not open the GPU: every shape is timed by a fresh child process under its own time limit (--limit seconds),
and the driver stops at the first child that fails or runs out of time.  The last lines print the MOE_MAX_ROWS the rule gives: the
largest measured rows-per-expert average (T k / E) up to which the fused route is not slower than the dense route at every measured
point of both shapes.

    python scripts/fp8_moe_time.py [--shapes mixtral,qwen3] [--ts 1,16,64,1024,4096] [--limit 240] [--log profiles/fp8/fp8_moe_time.log]
"""

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(shape, ts):
    """One shape in this process; a `POINT rows fused_le_dense mx_over_fused T` line follows every table row."""
    import torch

    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts
    from neural_compressor_amd.torch.algorithms.weight_only.experts import quantize_experts
    from scripts.moe_woq_time import PEAK, SHAPES, _float_experts
    from scripts.mx_moe_time import FLUSH_BYTES, _alternating

    dev = torch.device("cuda:0")
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device=dev)
    H, I, E, k = SHAPES[shape]
    fm = _float_experts(H, I, E, k, dev)
    int4 = quantize_experts(fm, dict(group_size=32, scheme="sym"), dev)
    mx = MXExperts.from_float(fm, "fp8_e4m3", "fp8_e4m3", device=dev)
    fp8 = FP8Experts.from_float(fm, device=dev)
    del fm
    torch.cuda.empty_cache()
    for m in (int4, mx, fp8):
        m.MOE_MAX_ROWS = 1 << 30  # this script times the fused routes at every T
    print(f"== {shape}: H {H} I {I} E {E} k {k} ({torch.cuda.get_device_name(0)})", flush=True)
    print(f"{'T':>5} {'rows/E':>7} {'active':>6} {'bytes MB':>9} {'fused':>9} {'dense':>9} {'mxfp8':>9} {'int4':>9} {'hbm':>6} "
          f"{'vs dense':>8} {'vs mxfp8':>8} {'vs int4':>7}", flush=True)
    per_expert = sum(b[0].numel() * b.element_size() for b in fp8.buffers())
    for T in ts:
        g = torch.Generator(device=dev).manual_seed(T)
        x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
        wts, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=g, device=dev), -1), k, dim=-1)
        wts = (wts / wts.sum(-1, keepdim=True)).to(torch.bfloat16)
        active = int(torch.unique(idx).numel())
        nbytes = active * per_expert + T * H * 2 + T * (H + 4) + T * k * (I * 2 + I + 4 + H * 4) + T * H * 2

        def route(fused):
            fp8.MOE_FUSED = fused
            return fp8(x, idx, wts)

        fns = {"fused": lambda: route(True), "dense": lambda: route(False), "mxfp8": lambda: mx(x, idx, wts),
               "int4": lambda: int4(x, idx, wts)}
        with torch.no_grad():
            t = _alternating(fns, 9 if T <= 256 else 5, flush)
        fp8.MOE_FUSED = True
        rows = T * k / E
        print(f"{T:>5} {rows:>7.2f} {active:>6} {nbytes / 1e6:>9.1f} {t['fused']:>9.1f} {t['dense']:>9.1f} {t['mxfp8']:>9.1f} "
              f"{t['int4']:>9.1f} {nbytes / (t['fused'] * 1e-6) / PEAK:>6.3f} {t['dense'] / t['fused']:>7.2f}x "
              f"{t['mxfp8'] / t['fused']:>7.2f}x {t['int4'] / t['fused']:>6.2f}x", flush=True)
        print(f"POINT {rows!r} {int(t['fused'] <= t['dense'])} {t['mxfp8'] / t['fused']!r} {T}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mixtral,qwen3")
    ap.add_argument("--ts", default="1,16,64,1024,4096")
    ap.add_argument("--limit", type=int, default=240, help="seconds one shape's child process may take")
    ap.add_argument("--log", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    ts = [int(t) for t in args.ts.split(",")]
    if args.worker:
        worker(args.worker, ts)
        return 0
    log = open(args.log, "w") if args.log else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    say("medians in us, weights cold (512 MiB rewritten before every call), variants alternating in one process per shape")
    points, status = [], 0
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--ts", args.ts]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, cwd=ROOT)
            out, rc = r.stdout, r.returncode
            err = r.stderr
        except subprocess.TimeoutExpired as e:
            out, rc, err = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124, "time limit"
        for line in out.splitlines():
            if line.startswith("POINT "):
                rows, ok, vs_mx, T = line.split()[1:]
                points.append((float(rows), ok == "1", shape, float(vs_mx), int(T)))
            else:
                say(line)
        if rc != 0:  # nothing more is started on the device after a failure
            say(f"{shape}: child ended with status {rc}; the remaining shapes are not measured\n{err[-2000:]}")
            status = 1
            break
    best = None
    for r in sorted({p[0] for p in points}):
        if all(ok for rows, ok, _, _, _ in points if rows <= r):
            best = r
        else:
            break
    lost = [(rows, shape) for rows, ok, shape, _, _ in points if not ok]
    slower = [(shape, T, round(v, 3)) for _, _, shape, v, T in points if v < 1.0]
    say(f"rows where the fused FP8 forward is slower than the fused MXFP8 forward (shape, T, mxfp8 / fp8): {slower if slower else 'none'}")
    say(f"points where the dense route is faster: {lost if lost else 'none'}")
    say(f"rule: MOE_MAX_ROWS = {best if best is None else format(best, 'g')} (largest measured rows-per-expert average up to which "
        f"fused <= dense on the measured shapes)")
    return status


if __name__ == "__main__":
    sys.exit(main())
