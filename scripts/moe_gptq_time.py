"""Routed Hessian launch (inc_gptq_hessian_accum_routed) against the per-expert loop it replaces, on MoE expert shapes.

Per shape and token count, both Hessians of one experts module (gate_up: K = H, gathered rows of x; down: K = I, sorted rows of h):
  routed : one call per Hessian, no host wait
  loop   : offsets to the host (.cpu()), a torch gather of x into sorted order (gate_up), one inc_gptq_hessian_accum per hit expert
Device events around each form, median of --reps after --warmup; fraction of the bf16 MFMA peak by K5's 2*T*K^2 convention summed
over experts (= 2 * routed rows * K^2).  Random routing (uniform over experts), random bf16 data.

    python scripts/moe_gptq_time.py [--shapes mixtral,qwen3] [--tokens 16384,65536] [--reps 5]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neural_compressor_amd import ops  # noqa: E402

SHAPES = {"mixtral": dict(E=8, k=2, H=4096, I=14336), "qwen3": dict(E=128, k=8, H=2048, I=768)}
PEAK_BF16 = 2.5e15  # dense bf16 MFMA peak, FLOP/s


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mixtral,qwen3")
    ap.add_argument("--tokens", default="16384,65536")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; median (min) ms of {args.reps} after {args.warmup} warm-up calls")
    for name in args.shapes.split(","):
        s = SHAPES[name]
        E, k, H, I = s["E"], s["k"], s["H"], s["I"]
        for T in [int(t) for t in args.tokens.split(",")]:
            g = torch.Generator().manual_seed(T)
            S = T * k
            idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(dev)
            x = (torch.randn(T, H, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            h = (torch.randn(S, I, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            route = ops.moe_route(idx, E)
            for tag, K, a, sorted_rows in (("gate_up", H, x, False), ("down", I, h, True)):
                Hs = torch.zeros((E, K, K), dtype=torch.float32, device=dev)
                rows = torch.ones(E, dtype=torch.int64, device=dev)  # beta != 0: the read-modify-write of H is part of both forms

                def routed():
                    assert ops.gptq_hessian_accum_routed(Hs, rows, a, route, T, k, sorted_rows=sorted_rows)

                def loop():
                    offs = route[1:E + 2].cpu().tolist()
                    if sorted_rows:
                        xs = a
                    else:
                        xs = a[torch.div(route[E + 2:E + 2 + offs[E]].long(), k, rounding_mode="floor")]
                    for e in range(E):
                        if offs[e + 1] > offs[e]:
                            ops.gptq_hessian_accum(Hs[e], xs[offs[e]:offs[e + 1]], 0.5, 1e-4)

                r_med, r_min = timed(routed, args.warmup, args.reps)
                l_med, l_min = timed(loop, args.warmup, args.reps)
                flop = 2.0 * S * K * K
                print(f"{name:8s} T={T:6d} {tag:8s} K={K:6d} rows/expert={S // E:6d}  routed {r_med:9.3f} ({r_min:9.3f}) ms "
                      f"{flop / r_med / 1e9 / (PEAK_BF16 / 1e12) :6.3f} of peak | loop {l_med:9.3f} ({l_min:9.3f}) ms "
                      f"{flop / l_med / 1e9 / (PEAK_BF16 / 1e12):6.3f} of peak | loop / routed {l_med / r_med:5.2f}x", flush=True)
                del Hs
            del x, h


if __name__ == "__main__":
    main()
