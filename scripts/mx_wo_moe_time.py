"""Time one experts layer forward of the weight-only MX cell on the MI355X against the MX cell on the same codes: device events, cold
weights (a buffer larger than the last-level cache is rewritten before every timed call), the variants alternating inside one process,
median of the repeats -- the method of scripts/mx_gpt_oss_time.py.  Every shape runs in a child process of its own under a time limit;
after a failed child nothing more is started.

Shapes (one layer, MXFP4 weights): gpt-oss-20b E 32, k 4, H = I = 2880 (Kp 2944: K < Kp in both products); gpt-oss-120b E 128, the same
H and I; Qwen3-30B-A3B E 128, k 8, H 2048, I 768 (SiLU experts).  Rows per point:
  wo       MXWeightOnly[GptOss]Experts' fused route: four launches, bf16 activations
  mx8      MX[GptOss]Experts with fp8_e4m3 activations on the same codes: six launches (two of them quantise x and h)
  dense    the weight-only module with MOE_FUSED = False (inc_mx_wo_gemv / inc_mx_wo_gemm per expert that was hit; host waits)
  g0 / g1  the routed GEMMs alone, mode 0 and mode 1: inc_mx_wo_moe_gemm[_glu] beside inc_mx_moe_gemm[_glu] on fp8 codes

The last lines print the MOE_MAX_ROWS the rule of scripts/mx_moe_time.py gives for the weight-only classes.

    python scripts/mx_wo_moe_time.py [--shapes 20b,120b,qwen3] [--ts 1,16,64,1024] [--log profiles/mx/mx_wo_moe_time.log]
"""

import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.mx_moe_time import FLUSH_BYTES, _alternating  # noqa: E402

SHAPES = {"20b": (2880, 2880, 32, 4, True), "120b": (2880, 2880, 128, 4, True), "qwen3": (2048, 768, 128, 8, False)}  # H, I, E, k, GPT-OSS
STEP_LIMIT = 420  # seconds, per shape


def _pair(H, I, E, oss, dev):
    """(weight-only module, MX module with fp8 activations) holding the same random MXFP4 codes, scale bytes 116 .. 123 and biases."""
    from neural_compressor_amd.torch.algorithms import mx_quant as Q

    wo_cls, mx_cls = (Q.MXWeightOnlyGptOssExperts, Q.MXGptOssExperts) if oss else (Q.MXWeightOnlyExperts, Q.MXExperts)
    wo = wo_cls(E, H, I, w_dtype="fp4", device=dev, float_type=torch.bfloat16)
    mx = mx_cls(E, H, I, w_dtype="fp4", act_dtype="fp8_e4m3", device=dev, float_type=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(E + H)
    for name, buf in wo.named_buffers():
        if name.endswith("_qweight"):
            K = H if name.startswith("gate_up") else I
            buf[:, :, :K // 2] = torch.randint(0, 256, (*buf.shape[:2], K // 2), generator=g, device=dev, dtype=torch.uint8)
        elif name.endswith("_w_scale"):
            buf.copy_(torch.randint(116, 124, buf.shape, generator=g, device=dev, dtype=torch.uint8))
        else:
            buf.copy_(torch.randn(buf.shape, generator=g, device=dev) * 0.1)
    mx.load_state_dict(wo.state_dict())
    for m in (wo, mx):
        m.MOE_MAX_ROWS = 1 << 30  # this script times the fused route at every T
    return wo, mx


def run_shape(shape, ts, say):
    """One shape, every T -> [(rows per expert, wo <= dense, wo <= mx8, shape)]."""
    from neural_compressor_amd import ops

    dev = torch.device("cuda:0")
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device=dev)
    H, I, E, k, oss = SHAPES[shape]
    wo, mx = _pair(H, I, E, oss, dev)
    say(f"== {shape}: H {H} I {I} E {E} k {k} Kp {wo.kp_h} / {wo.kp_i}, w fp4, {'clamped SwiGLU + biases' if oss else 'SiLU'}")
    say(f"{'T':>5} {'rows/E':>7} {'active':>6} {'wo':>9} {'mx8':>9} {'dense':>9} {'vs mx8':>7} {'vs dense':>8} | "
        f"{'g0 wo':>8} {'g0 mx8':>8} {'g1 wo':>8} {'g1 mx8':>8}")
    points = []
    for T in ts:
        g = torch.Generator(device=dev).manual_seed(T)
        x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
        wts, idx = torch.topk(torch.randn(T, E, generator=g, device=dev), k, dim=-1)
        wts = torch.softmax(wts, -1).to(torch.bfloat16)
        active = int(torch.unique(idx).numel())
        route = ops.moe_route(idx, E)
        xq, xs = ops.mx_quant(x, mx.act_fmt, mx.kp_h)
        h = torch.randn(T * k, I, generator=g, device=dev).to(torch.bfloat16)
        hq, hs = ops.mx_quant(h, mx.act_fmt, mx.kp_i)
        h0, y1 = torch.empty_like(h), torch.empty((T * k, H), dtype=torch.float32, device=dev)
        gu, dn = (wo.gate_up_qweight, wo.gate_up_w_scale, wo.w_fmt, T, k), (wo.down_qweight, wo.down_w_scale, wo.w_fmt, T, k)
        e0 = dict(bias=wo.gate_up_bias, alpha=wo.alpha, limit=wo.limit) if oss else {}
        e1 = dict(bias=wo.down_bias) if oss else {}
        wo_gemm, mx_gemm = (ops.mx_wo_moe_gemm_glu, ops.mx_moe_gemm_glu) if oss else (ops.mx_wo_moe_gemm, ops.mx_moe_gemm)

        def forward(m, fused):
            m.MOE_FUSED = fused
            return m(x, idx, wts)

        fns = {"wo": lambda: forward(wo, True), "mx8": lambda: forward(mx, True), "dense": lambda: forward(wo, False),
               "g0wo": lambda: wo_gemm(0, x, route, *gu, out=h0, **e0),
               "g0mx": lambda: mx_gemm(0, xq, xs, mx.act_fmt, route, *gu, out=h0, **e0),
               "g1wo": lambda: wo_gemm(1, h, route, *dn, routing_weights=wts, out=y1, **e1),
               "g1mx": lambda: mx_gemm(1, hq, hs, mx.act_fmt, route, *dn, routing_weights=wts, out=y1, **e1)}
        with torch.no_grad():
            t = _alternating(fns, 9 if T <= 256 else 5, flush)
        wo.MOE_FUSED = True
        rows = T * k / E
        points.append((rows, t["wo"] <= t["dense"], t["wo"] <= t["mx8"], shape))
        say(f"{T:>5} {rows:>7.2f} {active:>6} {t['wo']:>9.1f} {t['mx8']:>9.1f} {t['dense']:>9.1f} {t['mx8'] / t['wo']:>6.2f}x "
            f"{t['dense'] / t['wo']:>7.2f}x | {t['g0wo']:>8.1f} {t['g0mx']:>8.1f} {t['g1wo']:>8.1f} {t['g1mx']:>8.1f}")
    return points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20b,120b,qwen3")
    ap.add_argument("--ts", default="1,16,64,1024")
    ap.add_argument("--log", default=None)
    ap.add_argument("--child", default=None, help="internal: run this one shape and print POINT lines")
    args = ap.parse_args()
    ts = [int(t) for t in args.ts.split(",")]
    if args.child:
        for rows, ok, ok8, shape in run_shape(args.child, ts, lambda line: print(line, flush=True)):
            print(f"POINT {rows!r} {int(ok)} {int(ok8)} {shape}", flush=True)
        return
    log = open(args.log, "w") if args.log else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    say(f"medians in us, device events, weights cold ({FLUSH_BYTES >> 20} MiB rewritten before every call); vs mx8 = mx8 / wo, "
        f"vs dense = dense / wo (above 1: the four-launch route is faster)")
    points = []
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--ts", args.ts]
        try:
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            say(f"{shape}: not measured (the step ran past its limit of {STEP_LIMIT} s); nothing more is started")
            break
        for line in out.stdout.splitlines():
            if line.startswith("POINT "):
                _, rows, ok, ok8, sh = line.split()
                points.append((float(rows), bool(int(ok)), bool(int(ok8)), sh))
            else:
                say(line)
        if out.returncode != 0:
            say(f"{shape}: the step failed with status {out.returncode}; nothing more is started\n{out.stderr[-2000:]}")
            break
    best = None
    for r in sorted({p[0] for p in points}):
        if all(ok for rows, ok, _, _ in points if rows <= r):
            best = r
        else:
            break
    from neural_compressor_amd.torch.algorithms.mx_quant import MXWeightOnlyExperts

    say(f"points where the dense route is faster: {[(r, s) for r, ok, _, s in points if not ok] or 'none'}")
    say(f"points where the six-launch fp8 cell is faster: {[(r, s) for r, _, ok8, s in points if not ok8] or 'none'}")
    say(f"rule: MOE_MAX_ROWS = {best if best is None else format(best, 'g')} (largest measured rows-per-expert average up to which wo <= dense "
        f"on the measured shapes); shipped MXWeightOnlyExperts.MOE_MAX_ROWS = {MXWeightOnlyExperts.MOE_MAX_ROWS}")
    if log:
        log.close()


if __name__ == "__main__":
    main()
