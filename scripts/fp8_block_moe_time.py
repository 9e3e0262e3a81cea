"""Time one MoE experts layer forward with block-scaled FP8 experts on the MI355X, by the method of scripts/fp8_moe_time.py: device
events, cold weights (a buffer larger than the last-level cache is rewritten before every timed call), the variants alternating inside
one process, median of the repeats.

Variants, same inputs and routing (softmax top-k of random logits):
  fused     FP8BlockExperts' fused route (route -> quantise x per group -> gate_up -> quantise h -> down -> combine, no host wait)
  dense     FP8BlockExperts with MOE_FUSED = False (per expert that was hit: inc_fp8_quant_groups, inc_fp8_block_gemv / _gemm, host waits)
  pertoken  FP8Experts (per-token / per-channel factors in the epilogue) on the SAME weight codes, its fused route: the yardstick; the
            ratio fused / pertoken is what promoting every K-tile inside the loop costs
The weights are random e4m3 codes (magnitudes up to 240) with random block scales: nothing is quantised from a float module, so the
DeepSeek-V3 shaped layer needs no 22 GB float copy.  `bytes` is what the fused route must stream at least; `hbm` is that over the fused
time as a fraction of 8 TB/s.

The driver process does not open the GPU: every shape is timed by a fresh child process under its own time limit (--limit seconds),
and the driver stops at the first child that fails or runs out of time.  The last lines print the MOE_MAX_ROWS the rule gives: the
largest measured rows-per-expert average (T k / E) up to which the fused route is not slower than the dense route at every measured
point of the measured shapes.

    python scripts/fp8_block_moe_time.py [--shapes qwen3,deepseek_v3] [--ts 1,16,64,1024,4096] [--limit 400] [--log profiles/fp8/fp8_block_moe_time.log]
"""

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"qwen3": (2048, 768, 128, 8), "deepseek_v3": (7168, 2048, 256, 8)}  # H, I, E, k
PEAK = 8.0e12


def _random_codes(t, g):
    """Fill the uint8 buffer t with random e4m3 codes of magnitude code < 0x78 (no NaN code), expert by expert."""
    import torch

    for e in range(t.shape[0]):
        q = torch.randint(0, 0x78, t[e].shape, generator=g, device=t.device, dtype=torch.uint8)
        t[e].copy_(q | (torch.randint(0, 2, t[e].shape, generator=g, device=t.device, dtype=torch.uint8) << 7))


def worker(shape, ts):
    """One shape in this process; a `POINT rows fused_le_dense fused_over_pertoken T` line follows every table row."""
    import torch

    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockExperts, FP8Experts
    from scripts.mx_moe_time import FLUSH_BYTES, _alternating

    dev = torch.device("cuda:0")
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device=dev)
    H, I, E, k = SHAPES[shape]
    g = torch.Generator(device=dev).manual_seed(E)
    blk = FP8BlockExperts(E, H, I, device=dev, float_type=torch.bfloat16)
    tok = FP8Experts(E, H, I, device=dev, float_type=torch.bfloat16)
    for prefix in ("gate_up", "down"):
        _random_codes(blk._buffers[f"{prefix}_qweight"], g)
        tok._buffers[f"{prefix}_qweight"] = blk._buffers[f"{prefix}_qweight"]  # the same codes, shared
        for m in (blk, tok):
            s = m._buffers[f"{prefix}_w_scale"]
            s.copy_(torch.rand(s.shape, generator=g, device=dev) * 2.0 ** -10 + 2.0 ** -11)
    for m in (blk, tok):
        m.MOE_MAX_ROWS = 1 << 30  # this script times the fused routes at every T
    print(f"== {shape}: H {H} I {I} E {E} k {k} ({torch.cuda.get_device_name(0)})", flush=True)
    print(f"{'T':>5} {'rows/E':>7} {'active':>6} {'bytes MB':>9} {'fused':>9} {'dense':>9} {'pertoken':>9} {'hbm':>6} {'vs dense':>8} "
          f"{'fused/pertoken':>14}", flush=True)
    per_expert = sum(b[0].numel() * b.element_size() for b in blk.buffers())
    for T in ts:
        gt = torch.Generator(device=dev).manual_seed(T)
        x = torch.randn(T, H, generator=gt, device=dev).to(torch.bfloat16)
        wts, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=gt, device=dev), -1), k, dim=-1)
        wts = (wts / wts.sum(-1, keepdim=True)).to(torch.bfloat16)
        active = int(torch.unique(idx).numel())
        nbytes = (active * per_expert + T * H * 2 + T * (H + 4 * blk.kp_h // 128)
                  + T * k * (I * 2 + I + 4 * blk.kp_i // 128 + H * 4) + T * H * 2)

        def route(fused):
            blk.MOE_FUSED = fused
            return blk(x, idx, wts)

        fns = {"fused": lambda: route(True), "dense": lambda: route(False), "pertoken": lambda: tok(x, idx, wts)}
        with torch.no_grad():
            t = _alternating(fns, 9 if T <= 256 else 5, flush)
        blk.MOE_FUSED = True
        rows = T * k / E
        print(f"{T:>5} {rows:>7.2f} {active:>6} {nbytes / 1e6:>9.1f} {t['fused']:>9.1f} {t['dense']:>9.1f} {t['pertoken']:>9.1f} "
              f"{nbytes / (t['fused'] * 1e-6) / PEAK:>6.3f} {t['dense'] / t['fused']:>7.2f}x {t['fused'] / t['pertoken']:>13.2f}x", flush=True)
        print(f"POINT {rows!r} {int(t['fused'] <= t['dense'])} {t['fused'] / t['pertoken']!r} {T}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="qwen3,deepseek_v3")
    ap.add_argument("--ts", default="1,16,64,1024,4096")
    ap.add_argument("--limit", type=int, default=400, help="seconds one shape's child process may take")
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
            out, rc, err = r.stdout, r.returncode, r.stderr
        except subprocess.TimeoutExpired as e:
            out, rc, err = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124, "time limit"
        for line in out.splitlines():
            if line.startswith("POINT "):
                rows, ok, cost, T = line.split()[1:]
                points.append((float(rows), ok == "1", shape, float(cost), int(T)))
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
    say(f"what the in-loop promotion costs (shape, T, fused / pertoken): {[(s, T, round(c, 3)) for _, _, s, c, T in points]}")
    say(f"points where the dense route is faster: {lost if lost else 'none'}")
    say(f"rule: MOE_MAX_ROWS = {best if best is None else format(best, 'g')} (largest measured rows-per-expert average up to which "
        f"fused <= dense on the measured shapes)")
    return status


if __name__ == "__main__":
    sys.exit(main())
