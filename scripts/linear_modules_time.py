"""Host-side cost of the forward of the five quantised linear classes in two trees: the kernels are the same library, so what can move
between two versions of the Python around them (torch/algorithms/quant_linear.py) is the time the host takes to issue a forward.

  shapes   the Llama-2-13B linears (N, K) = (5120, 5120) and (13824, 5120), fp16, no bias
  M = 1    decode: the host clock around a run of forwards that ends in a device synchronise, after a warm-up run; microseconds per
           forward, the median over the runs
  M = 4096 prefill, one sanity point, measured the same way with shorter runs

The two group functions are timed too: fp8_linear_group / mx_linear_group on three members that share the activation (one decode
launch at M = 1, three GEMMs on the shared codes at M = 4096).

Every leg is a fresh child process that imports the package of one tree (--measure TREE).  The driver runs the legs parent, change,
parent one after the other, three times over; the difference between the two parent legs is the spread of the machine on the day, and a row
passes when the change's median is no further above the parent's than that.
The table goes to --out and nowhere else; what is said about it is in profiles/linear_frame/README.md.
usage: python scripts/linear_modules_time.py --parent PARENT_TREE [--change TREE] [--out profiles/linear_frame/timing.md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((5120, 5120), (13824, 5120))
POINTS = ((1, 2000, 9), (4096, 20, 5))  # rows, forwards per run, runs
ROUNDS = 3
LEG_SECONDS = 240


def measure(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch

    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear, FP8Linear, fp8_linear_group
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear, MXWeightOnlyLinear, mx_linear_group
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    dev = torch.device("cuda:0")
    for N, K in SHAPES:
        torch.manual_seed(0)
        lin = torch.nn.Linear(K, N, bias=False).half().to(dev)
        lo, hi = torch.full((K,), -4.0), torch.full((K,), 4.0)
        mods = {"W8A8Linear static": W8A8Linear.from_float(lin, lo, hi, device=dev),
                "W8A8Linear per_token": W8A8Linear.from_float(lin, device=dev, act_quant="per_token"),
                "FP8Linear": FP8Linear.from_float(lin, device=dev), "FP8BlockLinear": FP8BlockLinear.from_float(lin, device=dev),
                "MXLinear": MXLinear.from_float(lin, device=dev), "MXWeightOnlyLinear": MXWeightOnlyLinear.from_float(lin, device=dev)}
        groups = {"fp8_linear_group x 3": (fp8_linear_group, [FP8Linear.from_float(lin, device=dev) for _ in range(3)]),
                  "mx_linear_group x 3": (mx_linear_group, [MXLinear.from_float(lin, device=dev) for _ in range(3)])}
        mods.update({name: (lambda x, fn=fn, members=members: fn(x, members)) for name, (fn, members) in groups.items()})
        for M, calls, runs in POINTS:
            x = torch.randn(M, K, device=dev, dtype=torch.float16)
            with torch.no_grad():
                for name, m in mods.items():
                    times = []
                    for run in range(runs + 1):  # run 0 is the warm-up
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(calls):
                            m(x)
                        torch.cuda.synchronize()
                        times.append((time.perf_counter() - t0) / calls * 1e6)
                    print(json.dumps({"class": name, "N": N, "K": K, "M": M, "us": statistics.median(times[1:])}), flush=True)


def drive(a):
    legs = [("parent", a.parent), ("change", a.change), ("parent again", a.parent)] * ROUNDS
    rows = {}
    for leg, tree in legs:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", tree], capture_output=True, text=True,
                             timeout=LEG_SECONDS)
        if out.returncode != 0:  # nothing more is started on the device after a leg that failed
            sys.exit(f"leg '{leg}' ended with status {out.returncode}:\n{out.stderr[-2000:]}")
        for line in out.stdout.splitlines():
            r = json.loads(line)
            rows.setdefault((r["class"], r["N"], r["K"], r["M"]), {}).setdefault(leg, []).append(r["us"])
        print(f"leg '{leg}' done", flush=True)
    lines = ["# Host-side forward time of the linear classes: parent tree against this tree", "",
             f"`python scripts/linear_modules_time.py --parent <checkout of the parent commit>` on an MI355X; microseconds per forward, "
             f"fp16 input, no bias, host clock around {POINTS[0][1]} (M = 1) / {POINTS[1][1]} (M = 4096) forwards ending in a synchronise, "
             f"median of the runs of a leg and then of the {ROUNDS} rounds.  Legs alternate parent, change, parent in fresh processes.  spread = "
             "|parent - parent again|; a row passes when change - parent <= spread.", "",
             "| class | N | K | M | parent | change | parent again | change - parent | spread | |", "|---|---|---|---|---|---|---|---|---|---|"]
    failed = 0
    for (name, N, K, M), legs_us in rows.items():
        print(name, N, K, M, {leg: [round(v, 1) for v in us] for leg, us in legs_us.items()}, flush=True)
        p, c, p2 = (statistics.median(legs_us[leg]) for leg in ("parent", "change", "parent again"))
        ok = c - p <= abs(p - p2)
        failed += not ok
        lines.append(f"| {name} | {N} | {K} | {M} | {p:.1f} | {c:.1f} | {p2:.1f} | {c - p:+.1f} | {abs(p - p2):.1f} | {'ok' if ok else 'ABOVE'} |")
    lines += ["", f"{failed} of {len(rows)} rows above the spread."]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", help="run one leg on this tree and print one JSON line per row")
    ap.add_argument("--parent")
    ap.add_argument("--change", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_frame", "timing.md"))
    a = ap.parse_args()
    measure(a.measure) if a.measure else drive(a)
