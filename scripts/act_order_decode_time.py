"""Decode forward (M = 1, 4, 16, 64) of act_order (HF desc_act) INT4 g128 modules, bf16, with MI355XWeightOnlyLinear.ACT_ORDER_FUSED_GATHER
False (x.index_select + ops.woq_gemm: two launches, the un-prepared host path) and True (one inc_woq_gemm_perm launch through the
prepared call), alternating in one process, next to the module of the same shape without a g_idx.  Every row cycles through a ring of
distinct modules of >= 512 MiB of packed weights so that the weights come from HBM.

Two figures per row, medians over the repeats, both from device events:
  graph   one call, replayed from a captured graph that holds one call of every module of the ring (device time: no host in it);
  eager   one call, issued from Python one after the other (what a decode loop without graphs pays: the slower of host and device).
usage: python scripts/act_order_decode_time.py [--reps R]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear  # noqa: E402

dev = torch.device("cuda:0")
RING_BYTES = 512 << 20
GS = 128


def module(N, K, seed, act_order):
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = MI355XWeightOnlyLinear(K, N, bits=4, group_size=GS, zp=True, g_idx=act_order, device=dev)
    codes = torch.randint(0, 16, (N, K), generator=gen, device=dev, dtype=torch.int32)
    zp = torch.randint(1, 16, (N, K // GS), generator=gen, device=dev, dtype=torch.int32)
    m.pack(codes, torch.rand(N, K // GS, generator=gen, device=dev) * 0.02 + 1e-3, zp, None,
           g_idx=torch.randperm(K, generator=gen, device=dev) if act_order else None)
    assert m._forward_plan() == ("fused_act_order" if act_order else "fused")
    return m


def ring(N, K, act_order):
    n = -(-RING_BYTES // (N * K // 2))
    return [module(N, K, 1000 * act_order + i, act_order) for i in range(n)]


def captured(mods, x, side):
    with torch.cuda.stream(side):
        for _ in range(2):
            for m in mods:
                m(x)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):  # the stream the warm-up ran on: its (device, stream) workspace exists already
            for m in mods:
                m(x)
    torch.cuda.synchronize()
    return g


def timed(fn, calls, passes=8):
    """us per call: `passes` passes over the ring between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(passes):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (passes * calls) * 1e3


def main(reps):
    cls = MI355XWeightOnlyLinear
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for N, K in ((4096, 4096), (11008, 4096)):
        ao, plain = ring(N, K, True), ring(N, K, False)
        for M in (1, 4, 16, 64):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            graphs = {}
            for flag in (False, True):
                cls.ACT_ORDER_FUSED_GATHER = flag
                graphs[flag] = captured(ao, x, side)
                if flag:
                    assert all(m.__dict__["_call"] is not None for m in ao)
            cls.ACT_ORDER_FUSED_GATHER = False
            want = ao[0](x)
            cls.ACT_ORDER_FUSED_GATHER = True
            assert torch.equal(ao[0](x), want), "the two forms differ"
            graphs["plain"] = captured(plain, x, side)

            def eager(mods):
                for m in mods:
                    m(x)

            t = {k: [] for k in ("g_false", "g_true", "g_plain", "e_false", "e_true", "e_plain")}
            for _ in range(reps):  # alternating: whatever else the machine does hits every column alike
                for flag, name in ((False, "false"), (True, "true")):
                    cls.ACT_ORDER_FUSED_GATHER = flag
                    eager(ao)  # (the first pass after a switch rebuilds or drops the prepared calls)
                    t["g_" + name].append(timed(graphs[flag].replay, len(ao)))
                    t["e_" + name].append(timed(lambda: eager(ao), len(ao)))
                t["g_plain"].append(timed(graphs["plain"].replay, len(plain)))
                t["e_plain"].append(timed(lambda: eager(plain), len(plain)))
            md = {k: statistics.median(v) for k, v in t.items()}
            print(f"int4 g128 act_order {N}x{K} bf16 M={M:2d} ring of {len(ao)}: graph  two-launch {md['g_false']:6.2f} us | fused gather {md['g_true']:6.2f} us "
                  f"({md['g_false'] / md['g_true']:4.2f} x) | no g_idx {md['g_plain']:6.2f} us", flush=True)
            print(f"int4 g128 act_order {N}x{K} bf16 M={M:2d} ring of {len(ao)}: eager  two-launch {md['e_false']:6.2f} us | fused gather {md['e_true']:6.2f} us "
                  f"({md['e_false'] / md['e_true']:4.2f} x) | no g_idx {md['e_plain']:6.2f} us   (min / max of the graph figures: "
                  f"{min(t['g_false']):.2f}-{max(t['g_false']):.2f} | {min(t['g_true']):.2f}-{max(t['g_true']):.2f} | {min(t['g_plain']):.2f}-{max(t['g_plain']):.2f})",
                  flush=True)
            del graphs
        del ao, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9)
