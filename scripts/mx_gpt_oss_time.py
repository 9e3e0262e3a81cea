"""Time one GPT-OSS experts layer forward with MX experts on the MI355X: device events, cold weights (a buffer larger than the
last-level cache is rewritten before every timed call), the variants alternating inside one process, median of the repeats.  Modelled
on scripts/mx_moe_time.py.  Every shape runs in a child process of its own under a time limit; after a failed child nothing more is
started.

Shapes (one layer): gpt-oss-20b E 32, k 4, H = I = 2880 (Kp 2944); gpt-oss-120b E 128, k 4, the same H and I.  Weights are random
MXFP4 checkpoint tensors through MXGptOssExperts.from_mxfp4, with fp8_e4m3 and with fp4 (MXFP4) activations.  Four rows per point:
  fused    MXGptOssExperts' fused route (six launches, no host wait)
  dense    MXGptOssExperts with MOE_FUSED = False (per expert that was hit; host waits)
  bf16     transformers' GptOssExperts.forward, eager, bf16, on the recovered weights
  glu / silu / silu'   inc_mx_moe_gemm_glu mode 0 beside inc_mx_moe_gemm mode 0 on the same operands -- the two launches differ in the
           epilogue only -- and the SiLU launch a second time (A/A), so the run-to-run spread stands next to the A/B.

The last lines print the MOE_MAX_ROWS the rule of mx_moe_time.py gives on these shapes.

    python scripts/mx_gpt_oss_time.py [--shapes 20b,120b] [--ts 1,16,64,1024] [--log profiles/mx/mx_gpt_oss_time.log]
"""

import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.mx_moe_time import FLUSH_BYTES, _alternating  # noqa: E402

SHAPES = {"20b": (2880, 2880, 32, 4), "120b": (2880, 2880, 128, 4)}  # H, I, E, k
ACTS = ("fp8_e4m3", "fp4")
STEP_LIMIT = 420  # seconds, per shape


def _checkpoint(E, H, I, seed):
    g = torch.Generator().manual_seed(seed)
    gub = torch.randint(0, 256, (E, 2 * I, H // 32, 16), generator=g, dtype=torch.uint8)
    gus = torch.randint(116, 124, (E, 2 * I, H // 32), generator=g, dtype=torch.uint8)
    dnb = torch.randint(0, 256, (E, H, I // 32, 16), generator=g, dtype=torch.uint8)
    dns = torch.randint(116, 124, (E, H, I // 32), generator=g, dtype=torch.uint8)
    return gub, gus, torch.randn(E, 2 * I, generator=g) * 0.1, dnb, dns, torch.randn(E, H, generator=g) * 0.1


def _hf_experts(m, dev):
    from transformers import GptOssConfig
    from transformers.models.gpt_oss.modeling_gpt_oss import GptOssExperts

    with torch.device("meta"):
        ref = GptOssExperts(GptOssConfig(hidden_size=m.hidden_dim, intermediate_size=m.intermediate_dim, num_local_experts=m.num_experts,
                                         num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, head_dim=16, vocab_size=128))
    gu, dn = m.recover(torch.bfloat16)
    gb, db = m.recover_biases(torch.bfloat16)
    for name, v in (("gate_up_proj", gu), ("down_proj", dn), ("gate_up_proj_bias", gb), ("down_proj_bias", db)):
        setattr(ref, name, torch.nn.Parameter(v.to(dev), requires_grad=False))
    return ref


def run_shape(shape, ts, say):
    """One shape, every T and both activation formats -> [(rows per expert, fused <= dense, shape, act)]."""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts

    dev = torch.device("cuda:0")
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device=dev)
    H, I, E, k = SHAPES[shape]
    ck = _checkpoint(E, H, I, seed=E)
    mx = {}
    for act in ACTS:
        m = MXGptOssExperts.from_mxfp4(*ck, act_dtype=act, device=dev, float_type=torch.bfloat16)
        m.MOE_MAX_ROWS = 1 << 30  # this script times the fused route at every T
        mx[act] = m
    hf = _hf_experts(mx[ACTS[0]], dev)
    say(f"== gpt-oss-{shape}: H {H} I {I} E {E} k {k} Kp {mx[ACTS[0]].kp_h}, w fp4 (MXFP4 checkpoint bytes)")
    say(f"{'act':>9} {'T':>5} {'rows/E':>7} {'active':>6} {'fused':>9} {'dense':>9} {'bf16':>9} {'vs dense':>8} {'vs bf16':>7} | "
        f"{'glu':>8} {'silu':>8} {'silu^':>8} {'A/B':>6} {'A/A':>6}")
    points = []
    for T in ts:
        g = torch.Generator(device=dev).manual_seed(T)
        x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
        wts, idx = torch.topk(torch.randn(T, E, generator=g, device=dev), k, dim=-1)
        wts = torch.softmax(wts, -1).to(torch.bfloat16)
        active = int(torch.unique(idx).numel())
        reps = 9 if T <= 256 else 5
        for act, m in mx.items():
            route = ops.moe_route(idx, E)
            xq, xs = ops.mx_quant(x, m.act_fmt, m.kp_h)
            h = torch.empty((T * k, I), dtype=torch.bfloat16, device=dev)
            common = (0, xq, xs, m.act_fmt, route, m.gate_up_qweight, m.gate_up_w_scale, m.w_fmt, T, k)

            def forward(fused, m=m):
                m.MOE_FUSED = fused
                return m(x, idx, wts)

            fns = {"fused": lambda: forward(True), "dense": lambda: forward(False),
                   "glu": lambda: ops.mx_moe_gemm_glu(*common, bias=m.gate_up_bias, alpha=m.alpha, limit=m.limit, out=h),
                   "silu": lambda: ops.mx_moe_gemm(*common, out=h), "silu2": lambda: ops.mx_moe_gemm(*common, out=h)}
            if act == ACTS[0]:  # the float reference does not depend on the activation format: timed once per T
                fns["bf16"] = lambda: hf(x, idx, wts)
            with torch.no_grad():
                t = _alternating(fns, reps, flush)
            m.MOE_FUSED = True
            if act == ACTS[0]:
                t_bf16 = t["bf16"]
            rows = T * k / E
            points.append((rows, t["fused"] <= t["dense"], shape, act))
            say(f"{act:>9} {T:>5} {rows:>7.2f} {active:>6} {t['fused']:>9.1f} {t['dense']:>9.1f} {t_bf16:>9.1f} {t['dense'] / t['fused']:>7.2f}x "
                f"{t_bf16 / t['fused']:>6.2f}x | {t['glu']:>8.1f} {t['silu']:>8.1f} {t['silu2']:>8.1f} {t['glu'] / t['silu']:>6.3f} "
                f"{t['silu2'] / t['silu']:>6.3f}")
    return points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20b,120b")
    ap.add_argument("--ts", default="1,16,64,1024")
    ap.add_argument("--log", default=None)
    ap.add_argument("--child", default=None, help="internal: run this one shape and print POINT lines")
    args = ap.parse_args()
    ts = [int(t) for t in args.ts.split(",")]
    if args.child:
        for rows, ok, shape, act in run_shape(args.child, ts, lambda line: print(line, flush=True)):
            print(f"POINT {rows!r} {int(ok)} {shape} {act}", flush=True)
        return
    log = open(args.log, "w") if args.log else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    say(f"medians in us, device events, weights cold ({FLUSH_BYTES >> 20} MiB rewritten before every call); A/B = glu / silu, "
        f"A/A = silu^ / silu (the same launch timed twice)")
    points = []
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--ts", args.ts]
        try:
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            say(f"gpt-oss-{shape}: not measured (the step ran past its limit of {STEP_LIMIT} s); nothing more is started")
            break
        for line in out.stdout.splitlines():
            if line.startswith("POINT "):
                _, rows, ok, sh, act = line.split()
                points.append((float(rows), bool(int(ok)), sh, act))
            else:
                say(line)
        if out.returncode != 0:
            say(f"gpt-oss-{shape}: the step failed with status {out.returncode}; nothing more is started\n{out.stderr[-2000:]}")
            break
    best = None
    for r in sorted({p[0] for p in points}):
        if all(ok for rows, ok, _, _ in points if rows <= r):
            best = r
        else:
            break
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts

    lost = [(rows, shape, act) for rows, ok, shape, act in points if not ok]
    say(f"points where the dense route is faster: {lost if lost else 'none'}")
    say(f"rule: MOE_MAX_ROWS = {best if best is None else format(best, 'g')} (largest measured rows-per-expert average up to which fused <= dense "
        f"on the measured shapes and both activation formats); shipped MXGptOssExperts.MOE_MAX_ROWS = {MXGptOssExperts.MOE_MAX_ROWS}")
    if log:
        log.close()


if __name__ == "__main__":
    main()
