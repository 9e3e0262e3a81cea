"""CPU: inc_woq_gemv_anyw_perm and inc_woq_gemv_anyw_multi validate before any HIP call, the workspace of the batched launch follows
its formula, ops.sort_packed_k reorders the fields of a packed weight of any width (K % n_pack != 0 included), and the comparator of
the GPU perm cases rejects a gather through an order with two entries exchanged."""

import ctypes

import numpy as np
import pytest
import torch

from oracle import woq_oracle as O
from tests import act_order_cases as P
from tests import anyw_decode_cases as A
from tests import anyw_group_cases as G
from tests import gemm_route_cases as R

INC_ERR_BAD_ARG, INC_ERR_UNSUPPORTED, INC_ERR_WORKSPACE = -1, -2, -4


def _aligned():
    """(keep-alive buffer, a 16-byte aligned non-NULL address inside it); never dereferenced: every call below is rejected before a launch."""
    buf = np.zeros(64, dtype=np.int32)
    return buf, (buf.ctypes.data & ~15) + 16


def test_perm_validates_before_any_hip_call():
    from neural_compressor_amd import _lib

    L = _lib.lib
    buf, p = _aligned()

    def call(x=p, ko=p, qw=p, sc=p, y=p, M=5, N=68, K=96, Gn=3, gs=32, bits=3, ws=None, wsb=0, dt=2):
        return L.inc_woq_gemv_anyw_perm(x, dt, ko, qw, sc, p, None, y, M, N, K, Gn, gs, bits, ws, wsb, None)

    assert call(x=None) == INC_ERR_BAD_ARG and call(ko=None) == INC_ERR_BAD_ARG and call(qw=None) == INC_ERR_BAD_ARG
    assert call(y=None) == INC_ERR_BAD_ARG and call(Gn=4) == INC_ERR_BAD_ARG
    assert call(x=p + 1) == INC_ERR_BAD_ARG                          # x is read 2 bytes at a time
    assert call(bits=4) == INC_ERR_UNSUPPORTED and call(bits=8) == INC_ERR_UNSUPPORTED
    assert call(M=17) == INC_ERR_UNSUPPORTED and call(M=0) == INC_ERR_UNSUPPORTED
    assert call(N=60) == INC_ERR_UNSUPPORTED and call(N=66) == INC_ERR_UNSUPPORTED
    assert call(K=100, Gn=4) == INC_ERR_UNSUPPORTED and call(gs=48, Gn=2) == INC_ERR_UNSUPPORTED
    assert call(dt=0) == INC_ERR_UNSUPPORTED
    assert call(ko=p + 4) == INC_ERR_UNSUPPORTED                     # a misaligned order
    assert call(qw=p + 4) == INC_ERR_UNSUPPORTED and call(sc=p + 4) == INC_ERR_UNSUPPORTED
    assert call(M=16, K=1 << 27, Gn=1 << 22) == INC_ERR_UNSUPPORTED  # M * K = 2^31 (x by 32-bit byte offsets; the slice limit declines it too)
    assert call(M=4, N=64, K=2080, Gn=17, gs=128) == INC_ERR_WORKSPACE   # eligible, four slices, no workspace: nothing launched
    assert call(x=p + 2, M=4, N=64, K=2080, Gn=17, gs=128) == INC_ERR_WORKSPACE  # an x 2 bytes off: allowed here ...
    plain = L.inc_woq_gemv_anyw(p + 2, 2, p, p, p, None, p, 4, 64, 2080, 17, 128, 3, None, 0, None)
    assert plain == INC_ERR_UNSUPPORTED                              # ... and still declined by the plain entry


def test_multi_validates_before_any_hip_call():
    from neural_compressor_amd import _lib

    L = _lib.lib
    buf, p = _aligned()
    arr = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    ns = lambda *v: (ctypes.c_int64 * len(v))(*v)    # noqa: E731
    ptrs, narr = arr(p, p, p), ns(64, 68, 204)

    def call(n=3, x=p, ko=None, qw=ptrs, y=ptrs, M=5, N=narr, K=96, gs=32, bits=3):
        return L.inc_woq_gemv_anyw_multi(n, x, 2, ko, qw, ptrs, ptrs, None, y, M, N, K, gs, bits, None, 0, None)

    assert L.inc_woq_gemv_anyw_multi(3, None, 2, None, None, None, None, None, None, 5, None, 96, 32, 3, None, 0, None) == INC_ERR_BAD_ARG
    assert call(x=None) == INC_ERR_BAD_ARG and call(qw=None) == INC_ERR_BAD_ARG and call(N=None) == INC_ERR_BAD_ARG
    assert call(qw=arr(p, None, p)) == INC_ERR_BAD_ARG and call(y=arr(p, p, None)) == INC_ERR_BAD_ARG
    assert call(bits=4) == INC_ERR_UNSUPPORTED and call(bits=8) == INC_ERR_UNSUPPORTED
    assert call(M=17) == INC_ERR_UNSUPPORTED
    assert call(n=1) == INC_ERR_UNSUPPORTED
    nine = arr(*([p] * 9))
    assert L.inc_woq_gemv_anyw_multi(9, p, 2, None, nine, nine, nine, None, nine, 5, ns(*([64] * 9)), 96, 32, 3, None, 0, None) == INC_ERR_UNSUPPORTED
    assert call(N=ns(64, 60, 204)) == INC_ERR_UNSUPPORTED and call(N=ns(64, 68, 66)) == INC_ERR_UNSUPPORTED
    assert call(N=ns(64, 68, (1 << 18) + 4)) == INC_ERR_UNSUPPORTED
    assert call(K=100) == INC_ERR_UNSUPPORTED and call(gs=48) == INC_ERR_UNSUPPORTED
    assert call(x=p + 2) == INC_ERR_UNSUPPORTED                      # no orders: 16-byte loads of x
    assert call(x=p + 1, ko=ptrs) == INC_ERR_BAD_ARG                 # with orders x is read 2 bytes at a time
    assert call(ko=arr(p, p + 4, p)) == INC_ERR_UNSUPPORTED          # a misaligned order
    assert call(ko=arr(p, None, p)) == INC_ERR_BAD_ARG               # a NULL entry: the caller hands the identity
    assert call(qw=arr(p, p + 4, p)) == INC_ERR_UNSUPPORTED
    # all strips' counters must fit the 16 KiB block: 4096 strips do, 4097 do not (one slice, so the eligible batch would launch: only
    # the declined one is called)
    big = ns(1 << 17, 1 << 17, 64)
    assert call(N=big) == INC_ERR_UNSUPPORTED
    # eligible with four slices and no workspace: INC_ERR_WORKSPACE, nothing launched -- with and without orders, x 2 bytes off with them
    two = ns(264, 64)
    assert call(n=2, N=two, K=2080, gs=128, M=16) == INC_ERR_WORKSPACE
    assert call(n=2, N=two, K=2080, gs=128, M=16, ko=ptrs, x=p + 2) == INC_ERR_WORKSPACE


def test_multi_workspace_formula():
    from neural_compressor_amd import _lib

    L = _lib.lib
    for c in G.GROUP_CASES:
        narr = (ctypes.c_int64 * len(c.Ns))(*c.Ns)
        for M in (1, c.M, 16):
            got = L.inc_woq_gemv_anyw_multi_workspace_bytes(len(c.Ns), M, narr, c.K, c.bits)
            assert got == G.multi_workspace_bytes(M, c.Ns, c.K, c.bits), (c.name, M)
            singles = [L.inc_woq_gemv_anyw_slices(M, N, c.K, c.bits) for N in c.Ns]
            assert singles == [G.slices(c.K, c.bits)] * len(c.Ns)   # a member's slices are the single launch's
    one = G.GROUP_CASES[0]
    assert G.slices(one.K, one.bits) == 1 and G.multi_workspace_bytes(5, one.Ns, one.K, one.bits) == 0
    four = G.GROUP_CASES[1]
    assert G.slices(four.K, four.bits) == 4
    assert G.multi_workspace_bytes(16, four.Ns, four.K, four.bits) == 16384 + 4 * 16 * 328 * 4
    narr = (ctypes.c_int64 * 2)(264, 64)
    for bad in ((1, 16, 2080, 3), (2, 17, 2080, 3), (2, 16, 2080, 4), (2, 16, 2081, 3)):
        assert L.inc_woq_gemv_anyw_multi_workspace_bytes(bad[0], bad[1], narr, bad[2], bad[3]) == 0
    assert L.inc_woq_gemv_anyw_multi_workspace_bytes(2, 16, None, 2080, 3) == 0


@pytest.mark.parametrize("K", [96, 2080])
@pytest.mark.parametrize("bits", A.BITS + (4, 8))  # (4 / 8 bits: the act_order plan of the whole-word widths sorts through it too)
def test_sort_packed_k(bits, K):
    from neural_compressor_amd import ops

    N, npk = 8, 32 // bits
    rng = np.random.default_rng(31 * bits + K)
    iw = rng.integers(0, 1 << bits, size=(N, K))
    scales, zp = np.full((N, 1), 0.01, dtype=np.float32), rng.integers(0, 1 << bits, size=(N, 1))
    qweight, qzeros, _ = O.woq_pack_optimum(iw, scales, zp, bits)
    rows = -(-K // npk)
    assert qweight.shape == (rows, N)
    src = G.fields_of(qweight, bits)
    assert (src[K:] == 0).all()
    qw = torch.from_numpy(qweight)
    for kind in G.PERM_KINDS:
        order = P.perm(K, kind)
        out = ops.sort_packed_k(qw, torch.from_numpy(order), K, bits)
        assert out.dtype is torch.int32 and tuple(out.shape) == (rows, N) and out.is_contiguous()
        got = G.fields_of(out.numpy(), bits)
        assert np.array_equal(got[:K], src[order]), f"{bits} bits, K = {K}, {kind}: a field is not the source's at order[k]"
        assert (got[K:] == 0).all(), "a padding field is not zero"
        if kind == "identity":
            assert torch.equal(out, qw)
        w, _ = O.woq_unpack_optimum(out.numpy(), qzeros, N, K, 1, bits)
        assert np.array_equal(w.astype(np.int64), iw[:, order])
    # int64 orders are taken too; wrong shapes are refused
    assert torch.equal(ops.sort_packed_k(qw, torch.from_numpy(P.perm(K, "reversal")).long(), K, bits),
                       ops.sort_packed_k(qw, torch.from_numpy(P.perm(K, "reversal")), K, bits))
    with pytest.raises(ValueError, match="order must hold"):
        ops.sort_packed_k(qw, torch.arange(K - 1), K, bits)
    with pytest.raises(ValueError, match="qweight must be int32"):
        ops.sort_packed_k(qw[:-1], torch.arange(K), K, bits)


def test_perm_cases_hold_their_edges():
    """The rows of anyw_decode_cases this file borrows still hold what the issue picked them for."""
    by = {c.name: c for c in G.PERM_CASES}
    assert [c.name for c in G.PERM_CASES] == list(G.PERM_CASE_NAMES)
    assert by["b3_g32_straddle"].pins.straddle_words > 0 and by["b3_g32_straddle"].pins.strip_tail > 0
    c = by["b3_long_m16"]
    assert G.slices(c.K, c.bits) == 4 and c.pins.ragged_group and c.M == 16
    assert by["b6_tail4"].pins.padding > 0
    for c in G.PERM_CASES:
        assert A.pins_of(c) == c.pins, c.name
        assert c.K % 8 == 0


@pytest.mark.parametrize("kind", G.PERM_KINDS)
@pytest.mark.parametrize("c", G.PERM_CASES, ids=G.PERM_CASE_NAMES)
def test_comparator_rejects_an_order_with_two_entries_exchanged(c, kind):
    """Selectivity: a gather through swapped(p, x[0]) misses the bound of p's reference somewhere, so a wrong gather cannot pass."""
    for dtype in G.DTYPES:
        x, bias, p, ref, S = G.perm_reference(c, dtype, kind)
        assert R.worst_ratio(ref.to(dtype), ref, S, c.K, dtype)[0] <= 1.0, "the exact result rounded once must pass"
        q = P.swapped(p, x[0])
        assert sorted(q.tolist()) == list(range(c.K)) and (q != p).sum() == 2
        wrong = R.reference(x[:, torch.from_numpy(q).long()], R.dense_weight64(A.layer_of(c), dtype), bias)[0]
        assert float(((wrong - ref).abs() / R.tolerance(ref, S, c.K, dtype)).max()) > 1.0
        with pytest.raises(AssertionError, match="off by"):
            R.assert_elementwise(wrong.to(dtype), ref, S, c.K, dtype, "two entries of the order exchanged")


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_ops_wrappers_raise_before_the_library(device):
    from neural_compressor_amd import ops

    K, gs, bits, N = 96, 32, 3, 68
    part = (torch.zeros(10, N, dtype=torch.int32, device=device), torch.zeros(3, N, dtype=torch.float16, device=device),
            torch.zeros(3, 7, dtype=torch.int32, device=device), None, N)
    with pytest.raises(ValueError, match="HBM"):  # host / meta tensors: no CPU path
        ops.WoqGemvAnywCall(*part[:4], N, K, gs, bits, torch.bfloat16, k_order=torch.zeros(K, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="HBM"):
        ops.WoqGemvAnywGroupCall([part, part], K, gs, bits, torch.bfloat16)
    with pytest.raises(ValueError, match="bits=4"):
        ops.WoqGemvAnywGroupCall([part, part], K, gs, 4, torch.bfloat16)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        ops.WoqGemvAnywGroupCall([part, part], K, gs, bits, torch.float32)
