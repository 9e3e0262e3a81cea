"""One-launch decode groups on the Llama-2-7B shapes (INT4 g128, bf16, M = 1 and 16), each next to the form it replaces, in one process:

  qkv       act_order q + k + v (3 x 4096 x 4096): woq_linear_group (ONE inc_woq_gemm_multi_perm launch) against three prepared
            inc_woq_gemm_perm calls;
  gate_up   act_order gate + up (2 x 11008 x 4096): likewise, against two calls;
  gated     woq_gated_pair (ONE inc_woq_gemm_gated launch) against woq_linear_group + F.silu + mul (three launches), on modules
            without a g_idx and on act_order modules.

Cold weights: every row cycles through a ring of groups of distinct modules with >= 512 MiB of packed weights, so the words come from
HBM.  A figure is device time per group from a captured graph that holds one call of every group of the ring (no host in it), the
median over `reps` repeats of `passes` replays; the two forms of a row alternate, so whatever else the machine does hits both alike.
The outputs of the two forms are compared at the timed sizes before anything is timed.
usage: python scripts/decode_group_time.py [--reps R] [--passes P]"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd.torch.algorithms.weight_only import modules as W  # noqa: E402

dev = torch.device("cuda:0")
RING_BYTES = 512 << 20
GS = 128


def module(N, K, seed, act_order):
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = W.MI355XWeightOnlyLinear(K, N, bits=4, group_size=GS, zp=True, g_idx=act_order, device=dev)
    codes = torch.randint(0, 16, (N, K), generator=gen, device=dev, dtype=torch.int32)
    zp = torch.randint(1, 16, (N, K // GS), generator=gen, device=dev, dtype=torch.int32)
    m.pack(codes, torch.rand(N, K // GS, generator=gen, device=dev) * 0.02 + 1e-3, zp, None,
           g_idx=torch.randperm(K, generator=gen, device=dev) if act_order else None)
    m.bias = None
    assert m._forward_plan() == ("fused_act_order" if act_order else "fused")
    return m


def ring(n_members, N, K, act_order):
    groups = -(-RING_BYTES // (n_members * N * K // 2))
    return [[module(N, K, 100000 * act_order + 10 * g + i, act_order) for i in range(n_members)] for g in range(groups)]


def captured(fn, groups, side):
    with torch.cuda.stream(side):
        for _ in range(2):
            for grp in groups:
                fn(grp)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):  # the stream the warm-up ran on: its (device, stream) workspace exists already
            for grp in groups:
                fn(grp)
    torch.cuda.synchronize()
    return g


def timed(graph, groups, passes):
    """us per group: `passes` replays of the ring between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(passes):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (passes * groups) * 1e3


def row(name, groups, x, new, old, reps, passes, side, close):
    with torch.cuda.stream(side):  # both forms once before either is captured: the stream's workspace has its final size from here on
        a, b = new(groups[0]), old(groups[0])
    torch.cuda.synchronize()
    a, b = (a if isinstance(a, list) else [a]), (b if isinstance(b, list) else [b])
    worst = max(float(((p.float() - q.float()).abs() / (q.float().abs() + close)).max()) for p, q in zip(a, b))
    assert worst <= 2.0 ** -4, f"{name}: the two forms differ by {worst}"  # a guard against gross error only (the tests carry the bounds):
    # the forms differ by a few bf16 roundings of 2^-8 each, which silu stretches by up to |g| where g is negative
    g_new, g_old = captured(new, groups, side), captured(old, groups, side)
    t_new, t_old = [], []
    for _ in range(reps):
        t_new.append(timed(g_new, len(groups), passes))
        t_old.append(timed(g_old, len(groups), passes))
    m_new, m_old = statistics.median(t_new), statistics.median(t_old)
    print(f"{name} M={x.shape[0]:2d} ring of {len(groups)}: one launch {m_new:6.2f} us ({min(t_new):.2f}-{max(t_new):.2f}) | "
          f"parent form {m_old:6.2f} us ({min(t_old):.2f}-{max(t_old):.2f}) | {m_old / m_new:4.2f} x   "
          f"[outputs: worst relative distance {worst:.1e}]", flush=True)


def main(reps, passes):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    H, I = 4096, 11008
    for what, n, N, act_order in (("qkv", 3, H, True), ("gate_up", 2, I, True), ("gated_plain", 2, I, False)):
        groups = ring(n, N, H, act_order)
        for M in (1, 16):
            x = torch.randn(M, H, device=dev, dtype=torch.bfloat16)
            singles = lambda grp: [m(x) for m in grp]                      # noqa: E731
            grouped = lambda grp: W.woq_linear_group(x, grp)               # noqa: E731
            gated = lambda grp: W.woq_gated_pair(x, grp[0], grp[1])        # noqa: E731

            def unfused(grp):
                g, u = W.woq_linear_group(x, grp)
                return F.silu(g) * u

            if what != "gated_plain":
                grouped(groups[0])
                assert groups[0][0].__dict__["_group_calls"], "the group did not take the one-launch path"
                row(f"act_order {what} {n} x {N}x{H}: group vs single calls", groups, x, grouped, singles, reps, passes, side, 0.05)
            if n == 2:
                gated(groups[0])
                assert groups[0][0].__dict__.get("_gated_calls"), "the pair did not take the one-launch path"
                row(f"{'act_order' if act_order else 'plain'} gate/up {N}x{H}: gated pair vs group + silu + mul", groups, x, gated, unfused, reps, passes,
                    side, 0.01)
        del groups
        torch.cuda.empty_cache()


if __name__ == "__main__":
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d  # noqa: E731
    main(arg("--reps", 9), arg("--passes", 40))
