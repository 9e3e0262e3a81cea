"""CPU: the argument checks of ops.woq_gemm_perm / inc_woq_gemm_perm (everything they reject is rejected on the host, before a HIP
call) and a self-test of the cases of tests/act_order_cases.py: the comparator must tell a missing or wrong gather from a correct
one.  No GPU call anywhere in this file."""

import numpy as np
import pytest
import torch

from tests import act_order_cases as A
from tests import gemm_route_cases as R

FAKE_X, FAKE_Y, FAKE_KO, FAKE_W, FAKE_WS = 0x7F0000010000, 0x7F0000200000, 0x7F0000400000, 0x7F0000600000, 0x7F0000800000  # never dereferenced
INC_ERR_BAD_ARG, INC_ERR_UNSUPPORTED = -1, -2


def test_perm_cases_sit_on_the_three_decode_routes():
    for c, M in A.PARAMS:
        assert A.route_case(c, M).route in A.PERM_ROUTES
    assert {A.route_case(c, M).route for c, M in A.PARAMS} == set(A.PERM_ROUTES)
    variants = {(A.route_case(c, M).route, A.route_case(c, M).row_blocks, A.route_case(c, M).steps) for c, M in A.PARAMS}
    assert variants >= {("STREAM_W4", 1, 4), ("STREAM_W4", 2, 4), ("STREAM_W4", 4, 4), ("STREAM_W4", 1, 8),
                        ("STREAM_W8", 1, 4), ("STREAM_W8", 2, 4), ("STREAM_W8", 4, 4)}
    assert len(set(A.PARAM_IDS)) == len(A.PARAM_IDS)


def test_ops_woq_gemm_perm_rejects_a_bad_k_order_before_the_library(monkeypatch):
    from neural_compressor_amd import _lib, ops

    def boom(*a):
        raise AssertionError("the library was called")

    class Lib:  # every entry point raises
        def __getattr__(self, name):
            return boom

    monkeypatch.setattr(ops, "lib", Lib())
    N, K = 64, 128
    x = torch.zeros(2, K, dtype=torch.bfloat16)
    qw, sc, qz = torch.zeros(K // 8, N, dtype=torch.int32), torch.zeros(1, N, dtype=torch.float16), torch.zeros(1, N // 8, dtype=torch.int32)
    with pytest.raises(TypeError, match="int32"):
        ops.woq_gemm_perm(x, torch.arange(K), qw, sc, qz, None, N, K, 128, 4)                              # int64
    with pytest.raises(ValueError, match="K = 128"):
        ops.woq_gemm_perm(x, torch.arange(K - 1, dtype=torch.int32), qw, sc, qz, None, N, K, 128, 4)       # wrong length
    with pytest.raises(RuntimeError, match="different devices"):
        ops.woq_gemm_perm(x, torch.empty(K, dtype=torch.int32, device="meta"), qw, sc, qz, None, N, K, 128, 4)
    with pytest.raises(RuntimeError, match="HBM"):                                                        # and there is no CPU path
        ops.woq_gemm_perm(x, torch.arange(K, dtype=torch.int32), qw, sc, qz, None, N, K, 128, 4)
    assert _lib.SIGNATURES["inc_woq_gemm_perm"][1] == _lib.SIGNATURES["inc_woq_gemm"][1]  # same shape of call, k_order first


def test_prepared_call_rejects_a_bad_k_order():
    from neural_compressor_amd import ops

    N, K = 64, 128
    meta = dict(device="meta")
    qw, sc, qz = torch.empty(K // 8, N, dtype=torch.int32, **meta), torch.empty(1, N, dtype=torch.float16, **meta), torch.empty(1, N // 8, dtype=torch.int32, **meta)
    with pytest.raises(TypeError, match="int32"):
        ops.WoqGemmCall(qw, sc, qz, None, N, K, 128, 4, torch.bfloat16, k_order=torch.empty(K, dtype=torch.int64, **meta))
    with pytest.raises(ValueError, match="K = 128"):
        ops.WoqGemmCall(qw, sc, qz, None, N, K, 128, 4, torch.bfloat16, k_order=torch.empty(K + 1, dtype=torch.int32, **meta))
    with pytest.raises(ValueError, match="no g_idx"):
        ops.WoqGemmCall(qw, sc, qz, None, N, K, 128, 4, torch.bfloat16, g_idx=torch.empty(K, dtype=torch.int32, **meta),
                        k_order=torch.empty(K, dtype=torch.int32, **meta))
    with pytest.raises(RuntimeError, match="HBM"):  # ... and then the usual residency check
        ops.WoqGemmCall(qw, sc, qz, None, N, K, 128, 4, torch.bfloat16, k_order=torch.empty(K, dtype=torch.int32, **meta))


def _classify_oracle(g, K, gs):
    """numpy: (kind, order) as modules._classify_g_idx defines them."""
    gs_eff = K if (gs == -1 or gs >= K) else gs
    contiguous = np.arange(K) // gs_eff
    if np.array_equal(g, contiguous):
        return "contiguous", None
    order = np.argsort(g, kind="stable")
    return ("permuted", order) if np.array_equal(g[order], contiguous) else ("irregular", None)


def _g_idx_inputs():
    K, gs = 96, 32
    contiguous = np.arange(K) // gs
    yield "contiguous", K, gs, contiguous, "contiguous"
    for kind in A.PERM_KINDS:  # whole elements permuted (the identity leaves the contiguous index)
        yield kind, K, gs, contiguous[A.perm(K, kind)], "contiguous" if kind == "identity" else "permuted"
    moved = contiguous.copy()
    moved[gs - 1] = 1  # 31 elements in group 0, 33 in group 1
    yield "moved", K, gs, moved, "irregular"
    yield "ragged", 80, 32, (np.arange(80) // 32)[A.perm(80, "random")], "permuted"  # last group of 16
    for one in (128, -1):  # one group per row
        yield f"one_group_{one}", K, one, np.zeros(K, dtype=np.int64), "contiguous"
        yield f"one_group_{one}_plus", K, one, (np.arange(K) == 5).astype(np.int64), "irregular"


@pytest.mark.parametrize("name,K,gs,g,want", list(_g_idx_inputs()), ids=[t[0] for t in _g_idx_inputs()])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_classify_g_idx(name, K, gs, g, want, dtype):
    """One classification serves every plan: contiguous / a permutation of whole groups (with the stable argsort) / irregular."""
    from neural_compressor_amd.torch.algorithms.weight_only.modules import _classify_g_idx

    kind, order = _classify_g_idx(torch.from_numpy(g).to(dtype), K, gs)
    okind, oorder = _classify_oracle(g, K, gs)
    assert kind == okind == want
    if kind == "permuted":
        assert order.dtype is torch.int64 and np.array_equal(order.numpy(), oorder)
    else:
        assert order is None and oorder is None


def test_entry_point_rejects_on_the_host():
    """M > 64, a route without a gathering form, a misaligned k_order: INC_ERR_UNSUPPORTED before anything is launched (the
    pointers are never dereferenced)."""
    from neural_compressor_amd import _lib

    f, bf = _lib.lib.inc_woq_gemm_perm, _lib.INC_BF16
    ws = _lib.lib.inc_woq_gemm_workspace_bytes

    def call(M, N, K, gs, bits, ko=FAKE_KO, x=FAKE_X):
        return f(x, bf, ko, FAKE_W, FAKE_W, FAKE_W, None, FAKE_Y, M, N, K, max(1, K // gs), gs, bits, FAKE_WS, ws(M, N, K), None)

    assert f(None, bf, None, None, None, None, None, None, 1, 1, 1, 1, 1, 4, None, 0, None) == INC_ERR_BAD_ARG
    assert call(5, 200, 416, 32, 4, x=FAKE_X + 1) == INC_ERR_BAD_ARG            # x must hold 16-bit values
    assert call(65, 200, 416, 32, 4) == INC_ERR_UNSUPPORTED                      # STRIP
    assert call(65, 200, 512, 128, 8) == INC_ERR_UNSUPPORTED                     # 3A2B_W8
    assert call(16, 60, 256, 128, 4) == INC_ERR_UNSUPPORTED                      # SMALL (N < 64)
    assert call(40, 70, 200, 40, 4) == INC_ERR_UNSUPPORTED                       # TILE (groups of 40)
    assert call(40, 70, 192, 64, 3) == INC_ERR_UNSUPPORTED                       # TILE_ANYW
    for off in (4, 8, 12):
        assert call(5, 200, 416, 32, 4, ko=FAKE_KO + off) == INC_ERR_UNSUPPORTED
    assert call(5, 200, 416, 32, 9) == INC_ERR_UNSUPPORTED
    # a streaming route without its workspace: inc_woq_gemm's answer
    assert f(FAKE_X, bf, FAKE_KO, FAKE_W, FAKE_W, FAKE_W, None, FAKE_Y, 5, 200, 416, 13, 32, 4, None, 0, None) == R.INC_ERR_WORKSPACE


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("c,M", A.PARAMS, ids=A.PARAM_IDS)
def test_comparator_tells_a_wrong_gather_from_a_right_one(c, M, dtype):
    """Against the reference of a permutation, the exactly computed and once-rounded result of that permutation passes; the result of
    the same permutation with two entries exchanged fails, and so does the result without any gather (the identity).

    One exchanged pair moves an output by one product |dx| |dw|.  The bound grows with K (2 (K + 4) 2^-24 S, S = sum |x| |w|): at
    K = 33280 that term alone is 4e-3 S, more than any single product of the sum, so there a single exchange is inside the bound by
    construction and only the missing gather is asked for (the GPU file compares bit for bit with the gathered x on top)."""
    for kind in ("random", "reversal"):
        x, bias, ref, S = A.reference(c, M, dtype, kind)
        p = A.perm(c.K, kind)
        assert R.worst_ratio(A.exact_result(c, x, p, bias, dtype), ref, S, c.K, dtype)[0] <= 1.0
        if c.K <= 2048:
            assert R.worst_ratio(A.exact_result(c, x, A.swapped(p, x[0]), bias, dtype), ref, S, c.K, dtype)[0] > 1.0, "two swapped entries pass"
        assert R.worst_ratio(A.exact_result(c, x, A.perm(c.K, "identity"), bias, dtype), ref, S, c.K, dtype)[0] > 1.0, "no gather passes"
