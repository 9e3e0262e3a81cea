"""CPU: the entry points of the one-launch decode groups (inc_woq_gemm_multi_perm, inc_woq_gemm_gated) validate before any HIP call, the
ops wrappers raise on host / meta tensors before the library is reached, and the comparators of tests/decode_group_cases.py reject
what they are there to reject (an exact float64 result rounded once passes; exchanging gate and up, gathering through an order with
two entries exchanged, or dropping the SiLU does not)."""

import ctypes

import numpy as np
import pytest
import torch

from tests import act_order_cases as A
from tests import decode_group_cases as D
from tests import gemm_route_cases as R
from tests import moe_stage_cases as MS

INC_ERR_BAD_ARG, INC_ERR_UNSUPPORTED = -1, -2


def _host_arrays(n, K, Ns):
    """Host arrays of non-NULL addresses (never dereferenced: every call below is rejected before a launch)."""
    bufs = [np.zeros(64, dtype=np.int32) for _ in range(n)]
    ptrs = (ctypes.c_void_p * n)(*[(b.ctypes.data & ~15) + 16 for b in bufs])  # 16-byte aligned, inside the buffer
    return bufs, ptrs, (ctypes.c_int64 * n)(*Ns)


def test_multi_perm_validates_before_any_hip_call():
    from neural_compressor_amd import _lib

    L = _lib.lib
    n, K = 2, 416
    bufs, ptrs, narr = _host_arrays(n, K, (200, 264))
    x = ptrs[0]
    call = lambda n_=n, x_=x, ko=ptrs, bits=4, N=narr: L.inc_woq_gemm_multi_perm(  # noqa: E731
        n_, x_, 2, ko, ptrs, ptrs, ptrs, None, ptrs, 5, N, K, 32, bits, None, 0, None)
    assert L.inc_woq_gemm_multi_perm(2, None, 2, None, None, None, None, None, None, 5, None, K, 32, 4, None, 0, None) == INC_ERR_BAD_ARG
    assert call(ko=None) == INC_ERR_BAD_ARG                      # no array of orders
    assert call(bits=3) == INC_ERR_UNSUPPORTED                   # as inc_woq_gemm_multi
    assert call(n_=1) == INC_ERR_UNSUPPORTED
    with_null = (ctypes.c_void_p * n)(ptrs[0], None)
    assert call(ko=with_null) == INC_ERR_BAD_ARG                 # a NULL member of k_order
    assert call(x_=x + 1) == INC_ERR_BAD_ARG                     # x is read 2 bytes at a time
    off4 = (ctypes.c_void_p * n)(ptrs[0], ptrs[1] + 4)
    assert call(ko=off4) == INC_ERR_UNSUPPORTED                  # an order that is not 16-byte aligned
    # and inc_woq_gemm_multi itself still declines the same way
    assert L.inc_woq_gemm_multi(1, x, 2, ptrs, ptrs, ptrs, None, ptrs, 5, narr, K, 32, 4, None, 0, None) == INC_ERR_UNSUPPORTED


def test_gated_validates_before_any_hip_call():
    from neural_compressor_amd import _lib

    L = _lib.lib
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data & ~15
    p += 16

    def call(x=p, kg=None, ku=None, gq=p, M=5, N=200, K=416, gs=32, bits=4, act=0):
        return L.inc_woq_gemm_gated(x, 2, kg, ku, gq, p, p, p, p, p, p, M, N, K, gs, bits, act, None, 0, None)

    assert call(x=None) == INC_ERR_BAD_ARG and call(gq=None) == INC_ERR_BAD_ARG and call(M=0) == INC_ERR_BAD_ARG
    assert call(kg=p) == INC_ERR_BAD_ARG and call(ku=p) == INC_ERR_BAD_ARG       # both orders, or neither
    assert call(bits=3) == INC_ERR_UNSUPPORTED and call(bits=8) == INC_ERR_UNSUPPORTED
    assert call(act=1) == INC_ERR_UNSUPPORTED
    assert call(M=D.GATED_MAX_M + 1) == INC_ERR_UNSUPPORTED
    assert call(N=202) == INC_ERR_UNSUPPORTED and call(K=400) == INC_ERR_UNSUPPORTED and call(gs=48) == INC_ERR_UNSUPPORTED
    assert call(x=p + 2) == INC_ERR_UNSUPPORTED                                   # no orders: 16-byte loads of x
    assert call(kg=p, ku=p + 4) == INC_ERR_UNSUPPORTED                            # a misaligned order
    assert call() == -4                                                           # eligible, no workspace: INC_ERR_WORKSPACE, nothing launched
    assert call(x=p + 2, kg=p, ku=p) == -4                                        # gathered: x needs only 2-byte alignment
    assert L.inc_woq_gemm_gated_workspace_bytes(1, 4096, 4096) == D.COUNTER_BYTES + 8 * 1 * 2 * 4096 * 4
    for bad in ((0, 4096, 4096), (1, 0, 4096), (1, 4096, -1)):
        assert L.inc_woq_gemm_gated_workspace_bytes(*bad) == 0


def _part(N, K, G, device="cpu", bias=False):
    return (torch.zeros(K // 8, N, dtype=torch.int32, device=device), torch.zeros(G, N, dtype=torch.float16, device=device),
            torch.zeros(G, N // 8, dtype=torch.int32, device=device), torch.zeros(N, dtype=torch.float16, device=device) if bias else None, N)


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_ops_wrappers_raise_before_the_library(device):
    from neural_compressor_amd import ops

    K, G = 416, 13
    parts = [_part(200, K, G, device), _part(264, K, G, device)]
    good = torch.zeros(K, dtype=torch.int32, device=device)
    for make in (lambda ko: ops.WoqGemmGroupCall(parts, K, 32, 4, torch.bfloat16, k_orders=ko),
                 lambda ko: ops.WoqGatedCall(parts[0], parts[0], K, 32, 4, torch.bfloat16, k_orders=ko)):
        with pytest.raises(TypeError, match="k_order must be int32"):
            make([good.long(), None])
        with pytest.raises(ValueError, match=f"K = {K}"):
            make([good[:-1], good])
        with pytest.raises(ValueError, match=f"K = {K}"):
            make([None, good.view(1, K)])
        with pytest.raises(RuntimeError, match="HBM"):  # host / meta tensors: no CPU path
            make([good, None])
        with pytest.raises(RuntimeError, match="HBM"):
            make(None)
    with pytest.raises(ValueError, match="one entry per part"):
        ops.WoqGemmGroupCall(parts, K, 32, 4, torch.bfloat16, k_orders=[good])
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.WoqGatedCall(parts[0], parts[0], K, 32, 4, torch.float32)
    with pytest.raises(ValueError, match="same N"):
        ops.WoqGatedCall(parts[0], parts[1], K, 32, 4, torch.bfloat16)
    with pytest.raises(ValueError, match="bias"):
        ops.WoqGatedCall(_part(200, K, G, device, bias=True), parts[0], K, 32, 4, torch.bfloat16)


def test_cases_sit_on_their_rungs():
    """Host only: the route query and the workspace size pin every case (the GPU tests assert the same before they launch)."""
    for dtype in D.DTYPES:
        for c, M in D.PARAMS:
            D.assert_on_rung(c, M, dtype)
        for c, M in D.GATED_PARAMS:
            D.assert_on_rung(c, M, dtype, D.gated_ns(c))
    assert {D.row_blocks(M) for M in D.case("ragged").Ms} == {1, 2, 4}
    assert D.case("one_group").group_size >= D.case("one_group").K and D.case("eight_steps").plan.steps == 8


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
def test_group_comparator_rejects_a_wrong_order_and_a_wrong_member(dtype):
    c, M = D.case("ragged"), 5
    x, biases, outs = D.group_reference(c, M, dtype)
    Ls, ps = D.layers(c), D.orders(c)
    for i, (L, p, b, (ref, S)) in enumerate(zip(Ls, ps, biases, outs)):
        exact = ref.to(dtype)
        assert R.worst_ratio(exact, ref, S, c.K, dtype)[0] <= 1.0
        q = A.swapped(p, x[0])
        wrong = R.reference(D.gathered(x, q), D.dense64(L, dtype), b)[0].to(dtype)
        with pytest.raises(AssertionError, match="off by"):
            R.assert_elementwise(wrong, ref, S, c.K, dtype, "two entries of the order exchanged")
        other = ps[1 - i]  # the sibling's order
        wrong = R.reference(D.gathered(x, other), D.dense64(L, dtype), b)[0].to(dtype)
        with pytest.raises(AssertionError, match="off by"):
            R.assert_elementwise(wrong, ref, S, c.K, dtype, "the sibling's order")
    # members of equal shape differ: the one_group case has two 200-column members
    a, b = D.layers(D.case("one_group"))
    assert not np.array_equal(a["qweight"], b["qweight"]) and not np.array_equal(a["scales"], b["scales"])


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
@pytest.mark.parametrize("name", ["ragged", "slices"])
def test_gated_comparator_rejects_the_mutants(name, dtype):
    c, M = D.case(name), 5
    ps = tuple(D.orders(c, n=2))
    for orders in ((None, None), ps):
        x, ref, tol = D.gated_reference(c, M, dtype, orders)
        assert MS.worst_ratio(ref.to(dtype), ref, tol)[0] <= 1.0, "an exact result rounded once must pass"
        swapped_gu = D.gated_oracle(c, x, dtype, orders, swap=True)[0].to(dtype)
        no_silu = D.gated_oracle(c, x, dtype, orders, act=False)[0].to(dtype)
        base = orders[0] if orders[0] is not None else np.arange(c.K, dtype=np.int32)
        q = A.swapped(base, x[0])
        wrong_gather = D.gated_oracle(c, x, dtype, (q, orders[1]))[0].to(dtype)
        for what, y in (("gate and up exchanged", swapped_gu), ("the SiLU dropped", no_silu), ("two entries of gate's order exchanged", wrong_gather)):
            with pytest.raises(AssertionError, match="off by"):
                MS.assert_elementwise(y, ref, tol, what)
