"""SHA-256 of the outputs of every kernel on the strip frame (csrc/strip_frame.hpp), one line per case: run it in two trees and diff
the listings to see whether a change of the kernels moved a bit.  The cases are the tests' own tables; a line hashes the outputs of a
case in bf16 and fp16 (and, where said, over its scale rules or row counts).  Where the tables' helpers draw random operands (sums that
depend on their order) those are used, the exact operands of the experts tables too:

  mx_gemv         tests/mx_gemv_cases.VCASES x the three format pairs on mx_cases.random_operands with a bias (inc_mx_gemv)
  mx_gemv_multi   the member lists of tests/test_gpu_mx_gemv.py x the three pairs, M = 1 and 16, a member without bias (inc_mx_gemv_multi)
  mx_moe          every case and mode of tests/mx_moe_cases.CASES x pairs (both scale rules in one line) on its exact operands, and the random case of
                  every mode x pairs (inc_mx_moe_gemm)
  fp8_gemv        fp8_cases GEMV_NS x GEMV_TILES (every GEMV_MS in one line) on random codes with Gaussian factors and a bias (inc_fp8_gemv)
  fp8_multi       fp8_group_cases MS x TILES x (3, 8 members) (inc_fp8_gemv_multi)
  fp8_gated       fp8_group_cases GATED_MS x GATED_NS x TILES on the random case and the exact case with both biases, one line (inc_fp8_gemv_gated)
  fp8_moe         every case and mode of fp8_moe_cases.CASES on its exact operands, the random case of every mode (inc_fp8_moe_gemm)
  fp8_gemm        fp8_cases GEMM_SHAPES (every GEMM_KPS in one line) on random codes: the 256 x 256 kernel, which is not on the frame -- a control

Every launch is made twice; the two outputs must agree before they enter the digest.  Outputs the experts kernels do not write (rows
past the valid positions) hold a sentinel.
usage: python scripts/strip_outputs_digest.py > listing.txt"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd import ops  # noqa: E402
from tests import fp8_cases as F  # noqa: E402
from tests import fp8_group_cases as G  # noqa: E402
from tests import fp8_moe_cases as FM  # noqa: E402
from tests import moe_stage_cases as S  # noqa: E402
from tests import mx_cases as C  # noqa: E402
from tests import mx_gemv_cases as V  # noqa: E402
from tests import mx_moe_cases as MM  # noqa: E402

dev = torch.device("cuda:0")
DTYPES = (torch.bfloat16, torch.float16)
MULTI_NS = [(33, 17, 260), (1, 1030), (5, 16, 17, 1, 33, 48, 2, 20)]  # tests/test_gpu_mx_gemv.py


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype is torch.float32 else torch.int16)


def emit(name, *fns):
    """One line for the outputs of all of fns (the variants of one case: output types, scale rules, row counts)."""
    h = hashlib.sha256()
    for fn in fns:
        outs = [fn(), fn()]
        torch.cuda.synchronize()
        outs = [o if isinstance(o, (list, tuple)) else [o] for o in outs]
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*outs)), f"{name}: a second call is not bit-identical"
        for o in outs[0]:
            h.update(bits(o).cpu().numpy().tobytes())
    print(f"{name} {h.hexdigest()}", flush=True)


def to(*ts):
    return [None if t is None else t.to(dev) for t in ts]


def moe_out(ro, N, mode, dtype):
    """A sentinel-filled `out`: rows past the valid positions are not written."""
    t = torch.full((ro["S"], N // 2 if mode == 0 else N), 0x7B5A if mode == 0 else 0x7B5A7B5A, dtype=torch.int16 if mode == 0 else torch.int32)
    return t.view(dtype if mode == 0 else torch.float32).to(dev)


def mx_gemv():
    for c in V.VCASES:
        for pair, pid in zip(C.PAIRS, C.PAIR_IDS):
            r = C.random_operands(c.M, c.N, c.Kp, pair[0], pair[1], seed=5)
            xq, xs, wq, ws = to(C.stored(r["xq"], pair[0]), r["xs"], C.stored(r["wq"], pair[1]), r["ws"])
            bias = torch.randn(c.N, generator=torch.Generator().manual_seed(9)) * 0.5
            emit(f"mx_gemv {pid} {c.name}",
                 *[lambda dt=dt: ops.mx_gemv(xq, xs, pair[0], wq, ws, pair[1], bias.to(dt).to(dev), dt) for dt in DTYPES])
    for Ns in MULTI_NS:
        for pair, pid in zip(C.PAIRS, C.PAIR_IDS):
            for M in (1, 16):
                r = C.random_operands(M, sum(Ns), 600, pair[0], pair[1], seed=21)
                xq, xs = to(C.stored(r["xq"], pair[0]), r["xs"])
                wqs = [w.contiguous().to(dev) for w in C.stored(r["wq"], pair[1]).split(list(Ns))]
                wss = [s.contiguous().to(dev) for s in r["ws"].split(list(Ns))]
                g = torch.Generator().manual_seed(22)
                biases = [None if i == 1 else torch.randn(N, generator=g) for i, N in enumerate(Ns)]
                emit(f"mx_gemv_multi {pid} n{len(Ns)}_{Ns[0]}_{Ns[1]} m{M}",
                     *[lambda dt=dt: ops.mx_gemv_multi(xq, xs, pair[0], wqs, wss, pair[1],
                                                       [None if b is None else b.to(dt).to(dev) for b in biases], dt) for dt in DTYPES])


def moe_calls(call, d, operands):
    """The launches of one experts case: both 16-bit types in mode 0, fp32 otherwise.  call(mode, *operands, route, T, k, rw, out)."""
    ro, mode = d["ro"], d["mode"]
    route = S.route_buffer(ro, fill=-1).to(dev)
    operands = to(*operands)
    rw = d["rw"].float().to(dev) if mode == 1 else None
    return [lambda dt=dt: call(mode, *operands, route, ro["T"], ro["k"], rw, moe_out(ro, d["N"], mode, dt))
            for dt in (DTYPES if mode == 0 else (torch.float32,))]


def mx_moe():
    for pair, pid in zip(C.PAIRS, C.PAIR_IDS):
        def call(mode, aq, as_, wq, ws, route, T, k, rw, out):
            return ops.mx_moe_gemm(mode, aq, as_, pair[0], route, wq, ws, pair[1], T, k, rw, out=out)

        for c, mode in MM.CASE_MODES:
            calls = []
            for rule in MM.RULES:
                d = MM.exact_case(c, mode, rule)
                calls += moe_calls(call, d, MM.stored_operands(d, pair[0], pair[1], poison=True))
            emit(f"mx_moe {pid} {c.name} mode{mode}", *calls)
        for mode in (2, 1, 0):
            d = MM.random_case(mode, pair[0], pair[1])
            emit(f"mx_moe {pid} random mode{mode}", *moe_calls(call, d, (d["aq"], d["as_"], d["wq"], d["ws"])))


def fp8_gemv():
    for N in F.GEMV_NS:
        for tiles in F.GEMV_TILES:
            calls = []
            for M in F.GEMV_MS:
                r = F.random_codes(M, N, 128 * tiles, seed=77)
                rs, al, bias = F.gaussian_factors(M, N, 78)
                xq, wq, rs, al = to(r["xq"], r["wq"], rs, al)
                calls += [lambda xq=xq, rs=rs, wq=wq, al=al, bias=bias, dt=dt: ops.fp8_gemv(xq, rs, wq, al, bias.to(dt).to(dev), dt)
                          for dt in DTYPES]
            emit(f"fp8_gemv n{N} k{tiles}tiles", *calls)


def fp8_group():
    for M in G.MS:
        for tiles in G.TILES:
            for Ns in (G.MULTI_NS, G.MULTI_NS8):
                d = G.multi_case(M, Ns, 128 * tiles)
                xq, rs = to(d["xq"], d["rs"])
                wqs, als = to(*d["wqs"]), to(*d["als"])
                emit(f"fp8_multi m{M} k{tiles}tiles n{len(Ns)}",
                     *[lambda dt=dt: ops.fp8_gemv_multi(xq, rs, wqs, als, [None if b is None else b.to(dt).to(dev) for b in d["biases"]], dt)
                       for dt in DTYPES])
    for M in G.GATED_MS:
        for N in G.GATED_NS:
            for tiles in G.TILES:
                d = G.gated_random_case(M, N, 128 * tiles)
                xq, wg, wu, rs, ag, au = to(*(d[k] for k in ("xq", "wg", "wu", "rs", "ag", "au")))
                e = G.gated_exact_case(M, N, 128 * tiles, "both")
                exq, ewg, ewu = to(*G.gated_stored(e))
                ers, eag, eau = to(e["rs"], e["ag"], e["au"])
                emit(f"fp8_gated m{M} n{N} k{tiles}tiles",
                     *[lambda dt=dt: ops.fp8_gemv_gated(xq, rs, wg, ag, None, wu, au, None, dt) for dt in DTYPES],
                     *[lambda dt=dt: ops.fp8_gemv_gated(exq, ers, ewg, eag, e["bg"].to(dt).to(dev), ewu, eau, e["bu"].to(dt).to(dev), dt)
                       for dt in DTYPES])


def fp8_moe():
    def call(mode, aq, rs, wq, al, route, T, k, rw, out):
        return ops.fp8_moe_gemm(mode, aq, rs, route, wq, al, T, k, rw, out=out)

    for c, mode in FM.CASE_MODES:
        d = FM.exact_case(c, mode)
        emit(f"fp8_moe {c.name} mode{mode}", *moe_calls(call, d, FM.stored_operands(d, poison=True)))
    for mode in (2, 1, 0):
        d = FM.random_case(mode, small=mode == 0)
        emit(f"fp8_moe random mode{mode}", *moe_calls(call, d, (d["aq"], d["rs"], d["wq"].contiguous(), d["al"])))


def fp8_gemm():
    for M, N in F.GEMM_SHAPES:
        calls = []
        for Kp in F.GEMM_KPS:
            r = F.random_codes(M, N, Kp, seed=79)
            rs, al, bias = F.gaussian_factors(M, N, 80)
            xq, wq, rs, al = to(r["xq"], r["wq"], rs, al)
            calls += [lambda xq=xq, rs=rs, wq=wq, al=al, bias=bias, dt=dt: ops.fp8_gemm(xq, rs, wq, al, bias.to(dt).to(dev), dt) for dt in DTYPES]
        emit(f"fp8_gemm m{M} n{N}", *calls)


if __name__ == "__main__":
    with torch.no_grad():
        for part in (mx_gemv, mx_moe, fp8_gemv, fp8_group, fp8_moe, fp8_gemm):
            part()
