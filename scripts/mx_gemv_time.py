"""Times of the MX decode route (inc_mx_gemv, inc_mx_gemv_multi) against the tile kernel it replaces at M <= 16, on an MI355X.

  kernel   inc_mx_gemv against inc_mx_gemm (the route of every batch before the GEMV existed: the yardstick) on the same operands, for
           (act, weight) = (fp8, fp8), (fp8, fp4), (fp4, fp4) on the Llama-2-13B shapes at M = 1, 4, 16, with the share of the HBM peak
           on the algorithmic bytes; inc_w8a8_gemm_rowscale (the int8 launch on the bytes of MXFP8) for orientation;
  launch   one inc_mx_gemv_multi against n inc_mx_gemv launches (q + k + v, gate + up) through the C entry points;
  module   MXLinear.forward (quantiser + product) with DECODE_GEMV on and off;
  group    mx_linear_group on q + k + v (3 x 5120^2) and gate + up (2 x 13824 x 5120) against the list of single forwards.  The module
           and group rows include the Python of the forward between their two events: where that takes longer than the kernels, they
           measure the host.

The method is scripts/mx_gemm_time.py's (its time_alternating and its cold rings): one device-event pair per call, the variants
alternating in one loop with rotating order, weights from a ring of >= 768 MiB of distinct buffers, the median over the loop.  The last
lines state what the rule of the defaults gives: DECODE_GEMV stays on only where the GEMV is faster than the tile kernel at every row.
usage: python scripts/mx_gemv_time.py [--out profiles/mx/mx_gemv_time.log]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_gemm_time as T  # noqa: E402  (puts the repository root on sys.path)
from neural_compressor_amd import _lib  # noqa: E402

FP8, FP4 = T.FP8, T.FP4
PAIRS = {"a8w8": (FP8, FP8), "a8w4": (FP8, FP4), "a4w4": (FP4, FP4)}
SHAPES = ((5120, 5120), (13824, 5120), (5120, 13824))
MS = (1, 4, 16)
dev, say = T.dev, T.say


def code_bytes(rows, K, fmt):
    return rows * K * (2 if fmt == FP8 else 1) // 2 + rows * K // 32


def kernel_section():
    """-> {(M, N, K, pair): (gemv us, gemm us)}"""
    say("== kernel: inc_mx_gemv against inc_mx_gemm, inc_w8a8_gemm_rowscale for orientation (bf16 output, no bias, cold weights, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for N, K in SHAPES:
        n8, n4 = T.ring_len(N * K), T.ring_len(N * K // 2)
        ring = {FP8: [T.codes(N, K, FP8) for _ in range(n8)], FP4: [T.codes(N, K, FP4) for _ in range(n4)]}
        wi = [torch.randint(-127, 128, (N, K), device=dev, dtype=torch.int8) for _ in range(n8)]
        alpha = torch.rand(N, device=dev) * 1e-4 + 1e-5
        for M in MS:
            x = {FP8: T.codes(M, K, FP8), FP4: T.codes(M, K, FP4)}
            xi = torch.randint(-127, 128, (M, K), device=dev, dtype=torch.int8)
            rs = torch.rand(M, device=dev) * 1e-2 + 1e-3
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            need = _lib.lib.inc_w8a8_gemm_workspace_bytes(M, N, K)
            wsp = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

            def mx(entry, xf, wf):
                fn, xq, w = getattr(_lib.lib, entry), x[xf], ring[wf]

                def run(i):
                    wq = w[i % len(w)]
                    rc = fn(xq[0].data_ptr(), xq[1].data_ptr(), xf, wq[0].data_ptr(), wq[1].data_ptr(), wf, None, y.data_ptr(), _lib.INC_BF16,
                            M, N, K, stream)
                    assert rc == 0, rc
                return run

            def int8(i):
                rc = _lib.lib.inc_w8a8_gemm_rowscale(xi.data_ptr(), wi[i % n8].data_ptr(), rs.data_ptr(), alpha.data_ptr(), None, y.data_ptr(),
                                                     _lib.INC_BF16, M, N, K, wsp.data_ptr(), need, stream)
                assert rc == 0, rc

            variants = {"int8": int8}
            for name, (xf, wf) in PAIRS.items():
                variants["gemv_" + name] = mx("inc_mx_gemv", xf, wf)
                variants["gemm_" + name] = mx("inc_mx_gemm", xf, wf)
            t = T.time_alternating(variants, 200)
            cells = []
            for name, (xf, wf) in PAIRS.items():
                gv, gm = t["gemv_" + name], t["gemm_" + name]
                out[(M, N, K, name)] = (gv, gm)
                nbytes = code_bytes(N, K, wf) + code_bytes(M, K, xf) + 2 * M * N
                cells.append(f"{name} gemv {gv:7.1f} us ({nbytes / (gv * 1e-6) / T.HBM_PEAK:5.3f} of HBM peak)  gemm {gm:7.1f} us  gemm / gemv {gm / gv:5.2f}")
            say(f"M={M:3d} N={N:5d} K={K:5d}: " + "   ".join(cells) + f"   int8 {t['int8']:7.1f} us")
        del ring, wi
    return out


GROUPS = (("q+k+v 3 x 5120 x 5120", 3, (5120, 5120)), ("gate+up 2 x 13824 x 5120", 2, (13824, 5120)))


def multi_section():
    import ctypes

    say()
    say("== launch: one inc_mx_gemv_multi against n inc_mx_gemv launches on the same operands (bf16 output, no bias, cold weights, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for what, n, (N, K) in GROUPS:
        for pair, (xf, wf) in PAIRS.items():
            one = N * K // (1 if wf == FP8 else 2)
            ring = [[T.codes(N, K, wf) for _ in range(n)] for _ in range(T.ring_len(n * one))]
            arrs = [((ctypes.c_void_p * n)(*[w[0].data_ptr() for w in grp]), (ctypes.c_void_p * n)(*[w[1].data_ptr() for w in grp])) for grp in ring]
            Ns = (ctypes.c_int64 * n)(*[N] * n)
            cells = []
            for M in (1, 16):
                x = T.codes(M, K, xf)
                ys = [torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(n)]
                yarr = (ctypes.c_void_p * n)(*[y.data_ptr() for y in ys])

                def multi(i):
                    wq, ws = arrs[i % len(arrs)]
                    rc = _lib.lib.inc_mx_gemv_multi(n, x[0].data_ptr(), x[1].data_ptr(), xf, wq, ws, wf, None, yarr, _lib.INC_BF16, M, Ns, K, stream)
                    assert rc == 0, rc

                def singles(i):
                    for (wq, ws), y in zip(ring[i % len(ring)], ys):
                        rc = _lib.lib.inc_mx_gemv(x[0].data_ptr(), x[1].data_ptr(), xf, wq.data_ptr(), ws.data_ptr(), wf, None, y.data_ptr(),
                                                  _lib.INC_BF16, M, N, K, stream)
                        assert rc == 0, rc

                t = T.time_alternating({"multi": multi, "singles": singles}, 200)
                nbytes = n * code_bytes(N, K, wf) + code_bytes(M, K, xf) + 2 * M * N * n
                cells.append(f"M={M:2d} multi {t['multi']:7.1f} us ({nbytes / (t['multi'] * 1e-6) / T.HBM_PEAK:5.3f} of HBM peak)  "
                             f"{n} singles {t['singles']:7.1f} us  singles / multi {t['singles'] / t['multi']:5.2f}")
            say(f"{what} {pair}: " + "   ".join(cells))
            del ring, arrs


def _modules(N, K, pair, count):
    """`count` MXLinear modules [N, K] of the pair, without weights of their own: bind() gives them buffers of a ring."""
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    xf, wf = PAIRS[pair]
    names = {FP8: "fp8_e4m3", FP4: "fp4"}
    return [MXLinear(K, N, bias=False, w_dtype=names[wf], act_dtype=names[xf], device=dev, float_type=torch.bfloat16) for _ in range(count)]


def bind(mods, ring, i):
    for j, m in enumerate(mods):
        m.qweight, m.w_scale = ring[(i * len(mods) + j) % len(ring)]


def module_section():
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    say()
    say("== module: MXLinear.forward (inc_mx_quant + product) with DECODE_GEMV on / off (bf16, cold weights, median us) ==")
    for N, K in SHAPES:
        for pair, (xf, wf) in PAIRS.items():
            ring = [T.codes(N, K, wf) for _ in range(T.ring_len(N * K // (1 if wf == FP8 else 2)))]
            mods = _modules(N, K, pair, 1)
            cells = []
            for M in (1, 16):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)

                def fwd(on):
                    def run(i):
                        MXLinear.DECODE_GEMV = on
                        bind(mods, ring, i)
                        mods[0](x)
                    return run

                keep = MXLinear.DECODE_GEMV, MXLinear.DECODE_MAX_M
                MXLinear.DECODE_MAX_M = 16
                t = T.time_alternating({"on": fwd(True), "off": fwd(False)}, 200)
                MXLinear.DECODE_GEMV, MXLinear.DECODE_MAX_M = keep
                cells.append(f"M={M:2d} on {t['on']:7.1f} us  off {t['off']:7.1f} us  off / on {t['off'] / t['on']:5.2f}")
            say(f"N={N:5d} K={K:5d} {pair}: " + "   ".join(cells))
            del ring


def group_section():
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear, mx_linear_group

    say()
    say("== group: mx_linear_group against [m(x) for m in modules] (bf16, cold weights, median us) ==")
    for what, count, (N, K) in GROUPS:
        for pair, (xf, wf) in PAIRS.items():
            one = N * K // (1 if wf == FP8 else 2)
            ring = [T.codes(N, K, wf) for _ in range(count * T.ring_len(count * one))]
            mods = _modules(N, K, pair, count)
            cells = []
            for M in (1, 16):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)

                def group(i):
                    bind(mods, ring, i)
                    mx_linear_group(x, mods)

                def singles(i):
                    bind(mods, ring, i)
                    [m(x) for m in mods]

                keep = MXLinear.DECODE_GEMV, MXLinear.DECODE_MAX_M
                MXLinear.DECODE_GEMV, MXLinear.DECODE_MAX_M = True, 16
                t = T.time_alternating({"group": group, "singles": singles}, 200)
                MXLinear.DECODE_GEMV, MXLinear.DECODE_MAX_M = keep
                cells.append(f"M={M:2d} group {t['group']:7.1f} us  singles {t['singles']:7.1f} us  singles / group {t['singles'] / t['group']:5.2f}")
            say(f"{what} {pair}: " + "   ".join(cells))
            del ring


def verdict(times):
    say()
    wins = {M: all(gv < gm for (m, _, _, _), (gv, gm) in times.items() if m == M) for M in MS}
    best = max((M for M in MS if all(wins[m] for m in MS if m <= M)), default=None)
    say("== rule of the defaults: the GEMV faster than inc_mx_gemm on all three shapes and all three pairs ==")
    say("   ".join(f"M={M}: {'yes' if wins[M] else 'NO'}" for M in MS))
    if best == MS[-1]:
        say("-> DECODE_GEMV = True, DECODE_MAX_M = 16")
    elif best is not None:
        say(f"-> DECODE_GEMV = True, DECODE_MAX_M = {best}")
    else:
        say("-> DECODE_GEMV = False")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "mx", "mx_gemv_time.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    say(f"device: {torch.cuda.get_device_name(0)}; HBM peak taken as {T.HBM_PEAK / 1e12:.1f} TB/s")
    times = kernel_section()
    multi_section()
    module_section()
    group_section()
    verdict(times)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(T.lines) + "\n")


if __name__ == "__main__":
    main()
