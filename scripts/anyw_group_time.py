"""Decode of 3-bit weight-only modules (group 128, bf16) on the Llama-2-7B shapes at M = 1 and 16: the gathered launch of act_order
modules and the one-launch groups, each next to the forms it replaces.

  act_order  one act_order 4096 x 4096 module: `gathered` = MI355XWeightOnlyLinear.forward through inc_woq_gemv_anyw_perm (one launch),
             `select` = x.index_select(1, k_order) + inc_woq_gemv_anyw on the K-sorted words (two launches), `dense` = the same module
             with ODD_WIDTH_DECODE = False: HIP recover() + the library GEMM (the route before the gathered kernel existed);
  qkv        q + k + v (3 x 4096 x 4096): woq_linear_group (ONE inc_woq_gemv_anyw_multi launch) against three single launches;
  gate_up    gate + up (2 x 11008 x 4096): likewise, against two;
  qkv_act_order, gate_up_act_order: the two group rows with act_order members (every member gathers through its own order), and
             `n x select`: the single calls with x.index_select in front of the plain kernel (2 n launches).
  The act_order rows also run M = 4 and 8: ODD_WIDTH_GATHER_MAX_MN, the outputs (M x N) up to which the gather happens inside the
  kernel, is read off them (the script sets the attribute itself, so every form is timed at every M).

Cold weights: every row cycles through a ring of distinct modules (groups) with >= 512 MiB of packed weights, so the words come from
HBM.  A figure is device time per module (group) from a captured graph that holds one call of every element of the ring (no host in
it), the median over `reps` repeats of `passes` replays; the forms of a row alternate, so whatever else the machine does hits all
alike.  The outputs of the forms are compared at the timed sizes before anything is timed.

Without --row the script runs every row in a fresh child process of its own under a time limit and stops at the first that fails.
usage: python scripts/anyw_group_time.py [--row NAME] [--reps R] [--passes P] [--limit SECONDS]"""
import os
import statistics
import subprocess
import sys

ROWS = ("act_order", "qkv", "gate_up", "qkv_act_order", "gate_up_act_order")
RING_BYTES = 512 << 20
GS, BITS = 128, 3


def drive(reps, passes, limit):
    for row in ROWS:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--reps", str(reps), "--passes", str(passes)]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{row}: not measured (no result within {limit} s); stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{row}: not measured (exit status {rc}); stopping", flush=True)
            return rc
    return 0


def run_row(row, reps, passes):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only import modules as W

    dev = torch.device("cuda:0")

    def module(N, K, seed, act_order):
        gen = torch.Generator(device=dev).manual_seed(seed)
        m = W.MI355XWeightOnlyLinear(K, N, bits=BITS, group_size=GS, zp=True, g_idx=act_order, device=dev)
        codes = torch.randint(0, 1 << BITS, (N, K), generator=gen, device=dev, dtype=torch.int32)
        zp = torch.randint(0, 1 << BITS, (N, K // GS), generator=gen, device=dev, dtype=torch.int32)
        m.pack(codes, torch.rand(N, K // GS, generator=gen, device=dev) * 0.02 + 1e-3, zp, None,
               g_idx=torch.randperm(K, generator=gen, device=dev) if act_order else None)
        m.bias = None
        assert m._forward_plan() == "dense" and (m._decode_anyw_perm if act_order else m._decode_anyw)
        return m

    def packed_bytes(m):
        return sum(t.numel() * t.element_size() for t in (m.qweight, m.scales, m.qzeros))

    def ring(n_members, N, K, act_order):
        first = [module(N, K, 7 + i, act_order) for i in range(n_members)]
        groups = -(-RING_BYTES // (n_members * packed_bytes(first[0])))
        return [first] + [[module(N, K, 100 * g + 7 + i, act_order) for i in range(n_members)] for g in range(1, groups)]

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

    def timed(graph, n, passes):
        """us per element of the ring: `passes` replays between two device events."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(passes):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (passes * n) * 1e3

    def report(name, M, groups, forms, side, note):
        graphs = [captured(fn, groups, side) for _, fn in forms]
        t = [[] for _ in forms]
        for _ in range(reps):
            for i, g in enumerate(graphs):
                t[i].append(timed(g, len(groups), passes))
        med = [statistics.median(v) for v in t]
        cols = " | ".join(f"{label} {m:6.2f} us ({min(v):.2f}-{max(v):.2f})" for (label, _), m, v in zip(forms, med, t))
        ratios = ", ".join(f"{label} / {forms[0][0]} = {m / med[0]:.2f} x" for (label, _), m in list(zip(forms, med))[1:])
        print(f"{name:18s} M={M:2d} ring of {len(groups)}: {cols} | {ratios}   [{note}]", flush=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    act_order = row.endswith("act_order")
    if row == "act_order":
        mods = [g[0] for g in ring(1, 4096, 4096, True)]
        plain = {}
        for M in (1, 4, 8, 16):
            x = torch.randn(M, 4096, device=dev, dtype=torch.bfloat16)

            def gathered(m):
                m.ODD_WIDTH_DECODE, m.ODD_WIDTH_GATHER_MAX_MN = True, 1 << 30
                return m(x)

            def select(m):
                call = plain.get(id(m))
                if call is None:
                    call = plain[id(m)] = ops.WoqGemvAnywCall(m._qweight_sorted, m.scales, m.qzeros, None, 4096, 4096, GS, BITS, x.dtype)
                return call(x.index_select(1, m._k_order))

            def dense(m):
                m.ODD_WIDTH_DECODE = False
                return m(x)

            with torch.cuda.stream(side):
                a, b, c = gathered(mods[0]), select(mods[0]), dense(mods[0])
                assert mods[0].__dict__.get("_call") is None
                gathered(mods[0])
                call = mods[0].__dict__["_call"]
                assert isinstance(call, ops.WoqGemvAnywCall) and call.gathers(M), "the module did not take the gathered kernel"
            torch.cuda.synchronize()
            assert torch.equal(a, b), "gathered and select differ"
            worst = float(((a.float() - c.float()).abs() / (c.float().abs() + 0.05)).max())
            assert worst <= 2.0 ** -4, f"gathered and dense differ by {worst}"  # a guard against gross error only (the tests carry the bounds)
            report("act_order 4096x4096", M, mods, (("gathered", gathered), ("select", select), ("dense", dense)), side,
                   f"gathered == select bit for bit; worst relative distance to dense {worst:.1e}")
        return
    n, N, K = (3, 4096, 4096) if row.startswith("qkv") else (2, 11008, 4096)
    groups = ring(n, N, K, act_order)
    for M in (1, 4, 8, 16) if act_order else (1, 16):
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)

        def one(grp):
            for m in grp:
                m.ODD_WIDTH_GATHER_MAX_MN = 1 << 30
            return W.woq_linear_group(x, grp)

        def singles(grp):
            for m in grp:
                m.ODD_WIDTH_GATHER_MAX_MN = 1 << 30
            return [m(x) for m in grp]

        def select(grp):  # act_order members: x.index_select + the plain kernel per member, 2 n launches
            for m in grp:
                m.ODD_WIDTH_GATHER_MAX_MN = 0
            return [m(x) for m in grp]

        with torch.cuda.stream(side):
            c = select(groups[0]) if act_order else None
            assert not act_order or not any(m.__dict__["_call"].gathers(M) for m in groups[0])
            b, a = singles(groups[0]), one(groups[0])
            call = next(iter(groups[0][0].__dict__["_group_calls"].values()))
            assert isinstance(call, ops.WoqGemvAnywGroupCall) and (call.ko is not None) == act_order, "the group did not take the one launch"
            assert all(isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall) for m in groups[0])
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(a, b)), "the one launch and the single launches differ"
        assert c is None or all(torch.equal(p, q) for p, q in zip(a, c)), "the one launch and the select form differ"
        forms = (("one launch", one), (f"{n} launches", singles)) + (((f"{n} x select", select),) if act_order else ())
        report(f"{row} {n}x{N}x{K}", M, groups, forms, side, "outputs equal bit for bit")


if __name__ == "__main__":
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d  # noqa: E731
    if "--row" in sys.argv:
        run_row(sys.argv[sys.argv.index("--row") + 1], arg("--reps", 9), arg("--passes", 20))
    else:
        sys.exit(drive(arg("--reps", 9), arg("--passes", 20), arg("--limit", 420)))
