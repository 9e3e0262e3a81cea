"""CPU: the FP8 decode group launches without a GPU -- the argument validation of inc_fp8_gemv_multi / inc_fp8_gemv_gated (it runs before
any HIP call), the helpers' fallback on members that are not FP8Linear, the exports, and the gated oracle's own check: it passes on
its own output and rejects each wrong read."""

import ctypes

import pytest
import torch

from tests import fp8_group_cases as G

P = 4096  # a non-null, 16-byte aligned "pointer"


def _arr(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _multi(n=3, xq=P, rs=P, wq=None, alpha=None, bias=None, y=None, ydtype=None, M=1, N=None, Kp=128, arrays=(True,) * 5):
    """One call of inc_fp8_gemv_multi on fake pointers; `arrays`: which of (wq, alpha, bias, y, N) are passed at all."""
    from neural_compressor_amd import _lib

    m = max(n, 1)
    wq = [P] * m if wq is None else wq
    alpha = [P] * m if alpha is None else alpha
    bias = [None] * m if bias is None else bias
    y = [P] * m if y is None else y
    N = [4] * m if N is None else N
    a = [_arr(wq), _arr(alpha), _arr(bias), _arr(y), (ctypes.c_int64 * m)(*N)]
    a = [v if keep else None for v, keep in zip(a, arrays)]
    return _lib.lib.inc_fp8_gemv_multi(n, xq, rs, a[0], a[1], a[2], a[3], _lib.INC_BF16 if ydtype is None else ydtype, M, a[4], Kp, None)


def test_multi_validates_its_arguments():
    from neural_compressor_amd import _lib

    assert _multi(xq=None) == -1 and _multi(rs=None) == -1
    for i in (0, 1, 3, 4):                                            # the host arrays themselves; bias (2) may be NULL
        assert _multi(arrays=tuple(j != i for j in range(5))) == -1, i
    for hole in range(3):                                             # a NULL entry of wq / alpha / y of any member
        for which in ("wq", "alpha", "y"):
            vals = [P] * 3
            vals[hole] = None
            assert _multi(**{which: vals}) == -1, (which, hole)
    assert _multi(n=1) == -2 and _multi(n=9) == -2 and _multi(n=0) == -2
    assert _multi(M=17) == -2 and _multi(M=0) == -1
    assert _multi(Kp=192) == -2 and _multi(Kp=0) == -1
    assert _multi(ydtype=_lib.INC_F32) == -2
    assert _multi(N=[4, 0, 4]) == -1 and _multi(N=[4, 4, -1]) == -1
    assert _multi(xq=P + 8) == -1                                     # codes not 16-byte aligned
    assert _multi(wq=[P, P + 8, P]) == -1
    assert _multi(alpha=[P, P, P + 2]) == -1 and _multi(rs=P + 2) == -1


def test_gated_validates_its_arguments():
    """(xq, row_scale, wq_gate, alpha_gate, bias_gate, wq_up, alpha_up, bias_up, h, ydtype, M, N, Kp, stream)"""
    from neural_compressor_amd import _lib

    fn = _lib.lib.inc_fp8_gemv_gated
    BF16, F16, F32 = _lib.INC_BF16, _lib.INC_F16, _lib.INC_F32
    ok = [P, P, P, P, None, P, P, None, P]
    for hole in range(9):
        if hole in (4, 7):
            continue  # a bias may be NULL
        args = list(ok)
        args[hole] = None
        assert fn(*args, BF16, 1, 4, 128, None) == -1, hole
    assert fn(*ok, BF16, 0, 4, 128, None) == -1
    assert fn(*ok, BF16, 1, 0, 128, None) == -1 and fn(*ok, BF16, 1, -4, 128, None) == -1
    assert fn(*ok, BF16, 1, 4, 0, None) == -1
    assert fn(*ok, BF16, 17, 4, 128, None) == -2
    assert fn(*ok, F16, 1, 4, 192, None) == -2
    assert fn(*ok, F32, 1, 4, 128, None) == -2
    for hole in (0, 2, 5):                                            # codes not 16-byte aligned
        args = list(ok)
        args[hole] = P + 8
        assert fn(*args, F16, 1, 4, 128, None) == -1, hole
    for hole in (1, 3, 6):                                            # factors not 4-byte aligned
        args = list(ok)
        args[hole] = P + 2
        assert fn(*args, F16, 1, 4, 128, None) == -1, hole


def test_exports():
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms import fp8_quant
    from neural_compressor_amd.torch.algorithms.fp8_quant import fp8_gated_pair, fp8_linear_group  # noqa: F401

    assert ops.FP8_GEMV_MAX_MEMBERS == 8 == G.MAX_MEMBERS
    assert callable(ops.fp8_gemv_multi) and callable(ops.fp8_gemv_gated)
    assert sorted(fp8_quant.__all__) == ["FP8Linear", "FP8Quantizer", "load", "save"]
    assert fp8_quant.fp8_quant.GATED_FUSED in (True, False)


def test_ops_refuse_a_cpu_device():
    from neural_compressor_amd import ops

    z8, zf = torch.zeros(2, 128, dtype=torch.uint8), torch.ones(2)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.fp8_gemv_multi(z8, zf, [z8, z8], [zf, zf], [None, None], torch.bfloat16)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.fp8_gemv_gated(z8, zf, z8, zf, None, z8, zf, None, torch.bfloat16)


def test_helpers_on_plain_linears_are_the_single_forwards():
    from neural_compressor_amd.torch.algorithms.fp8_quant import fp8_gated_pair, fp8_linear_group

    torch.manual_seed(3)
    mods = [torch.nn.Linear(24, n, bias=b) for n, b in ((8, True), (5, False), (8, True))]
    x = torch.randn(2, 3, 24)
    with torch.no_grad():
        want = [m(x) for m in mods]
        got = fp8_linear_group(x, mods)
        assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))
        gate, up = mods[0], mods[2]
        assert torch.equal(fp8_gated_pair(x, gate, up), torch.nn.functional.silu(want[0]) * want[2])
        for act in (torch.nn.SiLU(), torch.nn.GELU(), torch.tanh):
            assert torch.equal(fp8_gated_pair(x, gate, up, act), act(want[0]) * want[2])


# ---- the gated oracle ---------------------------------------------------------------------------------------------------------------
ORACLE_CASES = [(5, 20, 1152, "both"), (16, 7, 128, "both"), (5, 260, 4224, "gate")]


@pytest.mark.parametrize("shape", ORACLE_CASES, ids=lambda s: "-".join(map(str, s)))
def test_gated_oracle_passes_on_itself_and_rejects_each_wrong_read(shape):
    d = G.gated_exact_case(*shape)
    min_g, shares = G.assert_gated_exact_condition(d)
    print(f"min g {min_g}, comparable shares {shares}")
    for dtype in G.OUT_DTYPES:
        why = G.gated_check(d, G.gated_oracle_output(d, dtype), dtype)
        assert why is None, why
        for mutate in G.MUTATIONS:
            if mutate == "bias_of_the_other_member" and shape[3] != "both":
                continue
            wrong = G.gated_oracle_output(d, dtype, mutate)
            assert G.gated_check(d, wrong, dtype) is not None, (mutate, dtype)          # the wrong read is past the bound ...
            assert G.gated_check(d, wrong, dtype, mutate) is None, (mutate, dtype)      # ... and is what that mutation's reference says


def test_gated_exact_cases_of_the_gpu_tests_hold_their_conditions():
    for M_ in (1, 16):
        for N in (7, 260):
            for tiles in G.TILES:
                for bias in ("both", "gate"):
                    G.assert_gated_exact_condition(G.gated_exact_case(M_, N, 128 * tiles, bias))


def test_gated_random_cases_stay_inside_fp16():
    for M_ in G.GATED_MS:
        for N in G.GATED_NS:
            for tiles in G.TILES:
                d = G.gated_random_case(M_, N, 128 * tiles)
                ref = G.S.silu64(d["g"]) * d["u"]
                assert float(ref.abs().max()) < float(torch.finfo(torch.float16).max) / 2
                assert float((ref.abs() > 2.0 ** -14).double().mean()) >= 0.9         # and are not lost in its subnormals
