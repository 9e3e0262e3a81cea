"""NF4 (RTN's default: group 32, fp32 scales, non-optimum row-packed layout) forward through inc_woq_gemm_lut, per M, next to the dense
route of the same module (MI355XWeightOnlyLinear.LUT_FUSED = False: HIP recover + library GEMM) and to the INT4 optimum g128 module of the
same shape, all in one process.  Decode rows (M <= 64) cycle through a ring of distinct modules of >= 512 MiB so the weights come from
HBM; larger M reuse one module.  HBM fraction = (packed bytes + scale bytes) / time / 8 TB/s (fp32 scales at g32 add 25 % to the
packed bytes; the INT4 module's fp16 g128 scales and zero points 3 %).
usage: python scripts/lut_gemm_time.py            (CUDA-graph replay timings)
       python scripts/lut_gemm_time.py --prof     (a few eager calls per case, for rocprofv3 --kernel-trace --stats)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear  # noqa: E402

MI355XWeightOnlyLinear.LUT_MAX_M = 1 << 62  # time the kernel at every M: these rows are what the route rule (LUT_MAX_M) is set from
dev = torch.device("cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
RING_BYTES = 512 << 20
PEAK = 8e12


def graph_time(fns, reps=5):
    """Mean time of one call of fns[i] (cycled), replaying a graph that holds one call of each."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            for f in fns:
                f()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    calls = max(20, len(fns))
    with torch.cuda.graph(g, stream=side):  # the stream the warm-up ran on: its (device, stream) workspace exists already
        for i in range(calls):
            fns[i % len(fns)]()
    g.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * calls) * 1e3


def nf4_module(N, K, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = MI355XWeightOnlyLinear(K, N, dtype="nf4", bits=4, group_size=32, scale_dtype=torch.float32, use_optimum_format=False, device=dev)
    codes = torch.randint(-8, 8, (N, K), generator=gen, device=dev, dtype=torch.int32)
    m.pack(codes, torch.rand(N, K // 32, generator=gen, device=dev) * 0.02 + 1e-3, None, None)
    return m


def int4_module(N, K, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = MI355XWeightOnlyLinear(K, N, bits=4, group_size=128, device=dev)
    codes = torch.randint(-8, 8, (N, K), generator=gen, device=dev, dtype=torch.int32)
    m.pack(codes, torch.rand(N, K // 128, generator=gen, device=dev) * 0.02 + 1e-3, None, None)
    m.bias = None
    return m


def nbytes(m):
    return sum(t.numel() * t.element_size() for t in (m.qweight, m.scales, getattr(m, "qzeros", None)) if t is not None)


def ring(make, N, K):
    m0 = make(N, K, 0)
    return [m0] + [make(N, K, i) for i in range(1, -(-RING_BYTES // nbytes(m0)))]


def main(prof):
    Ms = (1, 64, 4096) if prof else (1, 16, 64, 256, 1024, 4096)
    shapes = ((4096, 4096),) if prof else ((4096, 4096), (11008, 4096), (4096, 11008))
    for N, K in shapes:
        nf4 = ring(nf4_module, N, K)
        i4 = ring(int4_module, N, K)
        for M in Ms:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            a, b = (nf4, i4) if M <= 64 else (nf4[:1], i4[:1])
            assert a[0]._forward_plan() == "fused_lut"
            if prof:
                for m in a[:4] + b[:4]:
                    for _ in range(5):
                        m(x)
                MI355XWeightOnlyLinear.LUT_FUSED = False
                for m in a[:4]:
                    for _ in range(5):
                        m(x)
                MI355XWeightOnlyLinear.LUT_FUSED = True
                torch.cuda.synchronize()
                continue
            ref = torch.nn.functional.linear(x.float(), a[0].recover(dtype=torch.bfloat16).float())
            err = float((a[0](x).float() - ref).norm() / ref.norm())
            t = graph_time([lambda m=m: m(x) for m in a])
            ti4 = graph_time([lambda m=m: m(x) for m in b])
            MI355XWeightOnlyLinear.LUT_FUSED = False
            try:
                assert a[0]._forward_plan() == "dense"
                td = graph_time([lambda m=m: m(x) for m in a])
            finally:
                MI355XWeightOnlyLinear.LUT_FUSED = True
            cold = f"ring of {len(a)}" if len(a) > 1 else "one module"
            print(f"nf4 g32 {N}x{K} M={M:5d}: fused {t:8.1f} us ({nbytes(a[0]) / (t * 1e-6) / PEAK:.3f} of HBM, "
                  f"{2.0 * M * N * K / t / 1e6:7.1f} TFLOP/s) | dense route {td:8.1f} us ({td / t:5.1f} x) | "
                  f"int4 g128 optimum {ti4:8.1f} us ({nbytes(b[0]) / (ti4 * 1e-6) / PEAK:.3f} of HBM; nf4 / int4 = {t / ti4:4.2f}) | "
                  f"rel err {err:.1e} | {cold}", flush=True)
        del nf4, i4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main("--prof" in sys.argv)
