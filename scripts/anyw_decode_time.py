"""Decode of 2- and 3-bit weight-only modules (group 128, bf16) on the Llama-2-7B shapes at M = 1, 4 and 16, three routes in one process:

  decode    MI355XWeightOnlyLinear.forward through inc_woq_gemv_anyw (ODD_WIDTH_DECODE = True): one launch over the packed words;
  parent    the same module with ODD_WIDTH_DECODE = False: HIP recover() into a transient dense weight + the library GEMM;
  4-bit     the 4-bit module of the same shape (inc_woq_gemm's decode kernels), the sibling the new kernel is measured against.

Cold weights: every row cycles through a ring of distinct modules with >= 512 MiB of packed weights, so the words come from HBM.  A
figure is device time per module from a captured graph that holds one call of every module of the ring (no host in it), the median
over `reps` repeats of `passes` replays; the routes of a row alternate, so whatever else the machine does hits all alike.  The decode
route's fraction of the HBM peak counts the packed bytes only (qweight + scales + qzeros).  The outputs of decode and parent are compared
before anything is timed.
usage: python scripts/anyw_decode_time.py [--reps R] [--passes P]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd import ops  # noqa: E402
from neural_compressor_amd.torch.algorithms.weight_only import modules as W  # noqa: E402

dev = torch.device("cuda:0")
RING_BYTES = 512 << 20
GS = 128
HBM_PEAK = 8.0e12  # bytes / s (MI355X, vendor figure)


def module(N, K, bits, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = W.MI355XWeightOnlyLinear(K, N, bits=bits, group_size=GS, zp=True, device=dev)
    codes = torch.randint(0, 1 << bits, (N, K), generator=gen, device=dev, dtype=torch.int32)
    zp = torch.randint(0, 1 << bits, (N, K // GS), generator=gen, device=dev, dtype=torch.int32)
    m.pack(codes, torch.rand(N, K // GS, generator=gen, device=dev) * 0.02 + 1e-3, zp, None)
    m.bias = None
    return m


def packed_bytes(m):
    return sum(t.numel() * t.element_size() for t in (m.qweight, m.scales, m.qzeros))


def ring(N, K, bits):
    first = module(N, K, bits, 1000 * bits)
    n = -(-RING_BYTES // packed_bytes(first))
    return [first] + [module(N, K, bits, 1000 * bits + i) for i in range(1, n)]


def captured(fn, mods, side):
    with torch.cuda.stream(side):
        for _ in range(2):
            for m in mods:
                fn(m)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):  # the stream the warm-up ran on: its (device, stream) workspace exists already
            for m in mods:
                fn(m)
    torch.cuda.synchronize()
    return g


def timed(graph, n, passes):
    """us per module: `passes` replays of the ring between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(passes):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (passes * n) * 1e3


def main(reps, passes):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for N, K in ((4096, 4096), (11008, 4096), (4096, 11008)):
        ring4 = ring(N, K, 4)
        for bits in (3, 2):
            mods = ring(N, K, bits)
            nbytes = packed_bytes(mods[0])
            for M in (1, 4, 16):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)

                def decode(m):
                    m.ODD_WIDTH_DECODE = True
                    return m(x)

                def parent(m):
                    m.ODD_WIDTH_DECODE = False
                    return m(x)

                def four(m):
                    return m(x)

                with torch.cuda.stream(side):
                    four(ring4[0])  # every route once before any is captured: the stream's workspace has its final size from here on
                    a, b = decode(mods[0]), parent(mods[0])
                    assert isinstance(mods[0].__dict__.get("_call"), type(None)) and mods[0]._plan == "dense"
                    decode(mods[0])
                    assert isinstance(mods[0].__dict__["_call"], ops.WoqGemvAnywCall), "the module did not take the decode kernel"
                torch.cuda.synchronize()
                worst = float(((a.float() - b.float()).abs() / (b.float().abs() + 0.05)).max())
                assert worst <= 2.0 ** -4, f"decode and parent differ by {worst}"  # a guard against gross error only (the tests carry the bounds)
                graphs = [captured(f, r, side) for f, r in ((decode, mods), (parent, mods), (four, ring4))]
                t = [[], [], []]
                for _ in range(reps):
                    for i, (g, r) in enumerate(zip(graphs, (mods, mods, ring4))):
                        t[i].append(timed(g, len(r), passes))
                med = [statistics.median(v) for v in t]
                frac = nbytes / (med[0] * 1e-6) / HBM_PEAK
                print(f"{bits}-bit {N}x{K} M={M:2d} ring of {len(mods)} ({nbytes / 1e6:.1f} MB packed): decode {med[0]:6.2f} us "
                      f"({min(t[0]):.2f}-{max(t[0]):.2f}, {100 * frac:4.1f} % of HBM peak) | parent {med[1]:6.2f} us ({min(t[1]):.2f}-{max(t[1]):.2f}) | "
                      f"{med[1] / med[0]:5.2f} x | 4-bit sibling {med[2]:6.2f} us ({min(t[2]):.2f}-{max(t[2]):.2f})   "
                      f"[outputs: worst relative distance {worst:.1e}]", flush=True)
                del graphs
            del mods
            torch.cuda.empty_cache()
        del ring4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d  # noqa: E731
    main(arg("--reps", 9), arg("--passes", 20))
