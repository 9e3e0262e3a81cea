"""Times of the FP8 decode group launches (inc_fp8_gemv_multi, inc_fp8_gemv_gated, fp8_linear_group, fp8_gated_pair) next to the launches
they replace, on an MI355X: q + k + v as 3 x (5120, 5120) and gate + up as 2 x (13824, 5120), M = 1 and 16, bf16.

  launch   one inc_fp8_gemv_multi against n inc_fp8_gemv launches on the same operands, through the C entry points;
  group    fp8_linear_group against [m(x) for m in modules] (n quantiser launches + n products);
  gated    inc_fp8_gemv_gated against inc_fp8_gemv_multi + F.silu + mul (gate + up only);
  pair     fp8_gated_pair against its unfused form (GATED_FUSED = False: fp8_linear_group + F.silu + mul) and against the plain modules
           F.silu(gate(x)) * up(x).
The group and pair rows include the Python of the helper between their two events: where that takes longer than the kernels, they
measure the host.

Method: one device-event pair per call; 512 MiB are rewritten in front of every timed call, so weights, x and outputs come from HBM;
the variants of a row alternate in one loop with rotating order; the figure is the median.  Every section runs in a child process of
its own under `timeout`, and the first one that fails ends the run.  The last lines state what the rule gives: GATED_FUSED ships True
only if the fused form is not slower than the unfused one at every measured point.
usage: python scripts/fp8_group_time.py [--out profiles/fp8/fp8_group_time.log] [--iters 100]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = {"qkv": ("q+k+v 3 x 5120 x 5120", 3, 5120, 5120), "gate_up": ("gate+up 2 x 13824 x 5120", 2, 13824, 5120)}
MS = (1, 16)
FLUSH_BYTES = 512 << 20
SECTION_LIMIT = 240  # seconds for one child


def section(name, iters):
    import torch
    import torch.nn.functional as F

    from neural_compressor_amd import _lib, ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear, fp8_gated_pair, fp8_linear_group, fp8_quant

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    what, n, N, K = SECTIONS[name]
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    bf16 = torch.bfloat16

    def time_alternating(variants):
        names = list(variants)
        for k in names:
            variants[k]()
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in names}
        for it in range(iters):
            for j in range(len(names)):
                k = names[(it + j) % len(names)]
                flush.add_(1)
                a, b = ev[k][it]
                a.record()
                variants[k]()
                b.record()
        torch.cuda.synchronize()
        return {k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev[k]) for k in names}

    mods = []
    for i in range(n):
        m = FP8Linear(K, N, bias=False, device=dev, float_type=bf16)
        q = torch.randint(0, 256, (N, K), device=dev, dtype=torch.uint8)
        q[(q & 0x7F) == 0x7F] = 0
        m.qweight.copy_(q)
        m.w_scale.copy_(torch.rand(N, device=dev) * 1e-3 + 1e-4)
        mods.append(m)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    wq, al = arr([m.qweight for m in mods]), arr([m.w_scale for m in mods])
    Ns = (ctypes.c_int64 * n)(*[N] * n)
    FP8Linear.DECODE_GEMV, FP8Linear.DECODE_MAX_M = True, 16
    verdict = []
    for M in MS:
        x = torch.randn(M, K, device=dev, dtype=bf16)
        xq, rs = ops.fp8_quant_rows(x, None, K)
        ys = [torch.empty(M, N, dtype=bf16, device=dev) for _ in range(n)]
        yarr = arr(ys)
        h = torch.empty(M, N, dtype=bf16, device=dev)

        def multi():
            rc = _lib.lib.inc_fp8_gemv_multi(n, xq.data_ptr(), rs.data_ptr(), wq, al, None, yarr, _lib.INC_BF16, M, Ns, K, stream)
            assert rc == 0, rc

        def singles():
            for m, y in zip(mods, ys):
                rc = _lib.lib.inc_fp8_gemv(xq.data_ptr(), rs.data_ptr(), m.qweight.data_ptr(), m.w_scale.data_ptr(), None, y.data_ptr(),
                                           _lib.INC_BF16, M, N, K, stream)
                assert rc == 0, rc

        t = time_alternating({"multi": multi, "singles": singles})
        nbytes = n * N * K + M * K + 4 * (M + n * N) + 2 * M * N * n
        print(f"launch {what} M={M:2d}: multi {t['multi']:7.1f} us ({nbytes / (t['multi'] * 1e-6) / 8.0e12:5.3f} of 8.0 TB/s)  "
              f"{n} singles {t['singles']:7.1f} us  singles / multi {t['singles'] / t['multi']:5.2f}", flush=True)

        t = time_alternating({"group": lambda: fp8_linear_group(x, mods), "forwards": lambda: [m(x) for m in mods]})
        print(f"group  {what} M={M:2d}: fp8_linear_group {t['group']:7.1f} us  {n} forwards {t['forwards']:7.1f} us  "
              f"forwards / group {t['forwards'] / t['group']:5.2f}", flush=True)
        if name != "gate_up":
            continue
        g_, u_ = mods

        def gated():
            rc = _lib.lib.inc_fp8_gemv_gated(xq.data_ptr(), rs.data_ptr(), g_.qweight.data_ptr(), g_.w_scale.data_ptr(), None,
                                             u_.qweight.data_ptr(), u_.w_scale.data_ptr(), None, h.data_ptr(), _lib.INC_BF16, M, N, K, stream)
            assert rc == 0, rc

        def multi_silu_mul():
            multi()
            return F.silu(ys[0]) * ys[1]

        t = time_alternating({"gated": gated, "unfused": multi_silu_mul})
        verdict.append(t["gated"] <= t["unfused"])
        print(f"gated  {what} M={M:2d}: inc_fp8_gemv_gated {t['gated']:7.1f} us  multi + silu + mul {t['unfused']:7.1f} us  "
              f"unfused / gated {t['unfused'] / t['gated']:5.2f}", flush=True)

        def pair(on):
            def run():
                fp8_quant.GATED_FUSED = on
                return fp8_gated_pair(x, g_, u_)
            return run

        keep = fp8_quant.GATED_FUSED
        t = time_alternating({"fused": pair(True), "unfused": pair(False), "modules": lambda: F.silu(g_(x)) * u_(x)})
        fp8_quant.GATED_FUSED = keep
        verdict.append(t["fused"] <= t["unfused"])
        print(f"pair   {what} M={M:2d}: fp8_gated_pair fused {t['fused']:7.1f} us  unfused (group + silu + mul) {t['unfused']:7.1f} us  "
              f"plain modules {t['modules']:7.1f} us  unfused / fused {t['unfused'] / t['fused']:5.2f}  "
              f"modules / fused {t['modules'] / t['fused']:5.2f}", flush=True)
    if verdict:
        print("== rule of GATED_FUSED: the fused form not slower than the unfused one at every measured point: "
              + ("yes -> GATED_FUSED = True" if all(verdict) else "NO -> GATED_FUSED = False"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8", "fp8_group_time.log"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--section", choices=sorted(SECTIONS))
    a = ap.parse_args()
    if a.section:
        section(a.section, a.iters)
        return 0
    lines = ["FP8 decode groups (bf16 output, no bias; 512 MiB rewritten before every timed call, device events, variants alternating, "
             f"median of {a.iters}, us)"]
    print(lines[0], flush=True)
    rc = 0
    for name in ("qkv", "gate_up"):  # each GPU step in a process of its own under its own time limit; a failure ends the run
        p = subprocess.run(["timeout", "-k", "10", str(SECTION_LIMIT), sys.executable, os.path.abspath(__file__), "--section", name,
                            "--iters", str(a.iters)], stdout=subprocess.PIPE, text=True)
        print(p.stdout, end="", flush=True)
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"section {name} ended with status {p.returncode}: stopped")
            print(lines[-1], flush=True)
            rc = p.returncode
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
