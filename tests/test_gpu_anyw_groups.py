"""-m gpu: the gathered and the batched decode GEMV of the 1 / 2 / 3 / 5 / 6 / 7-bit modules (inc_woq_gemv_anyw_perm,
inc_woq_gemv_anyw_multi) on the cases of tests/anyw_group_cases.py, bf16 and fp16.

  C1  inc_woq_gemv_anyw_perm(x, p, W) == inc_woq_gemv_anyw(x.index_select(1, p), W), bit for bit;
  C2  output i of inc_woq_gemv_anyw_multi == the single entry (plain or gathered) on member i, bit for bit;
  C3  every output within the element-wise bound of tests/gemm_route_cases.py of the float64 product on the oracle's dense weight;
  C4  repeated calls are bit-identical, and a single call after a group launch on the same workspace is correct (counters re-armed);
  C5  the module route on one-hot rows returns columns of the module's own recover(dtype), bit for bit.
"""

import ctypes

import pytest
import torch

from tests import anyw_decode_cases as A
from tests import anyw_group_cases as G
from tests import gemm_route_cases as R

pytestmark = pytest.mark.gpu

WS_SENTINEL, WS_TAIL = 0xA5, 4096
_dev = {}


def _layer_tensors(hip, L):
    key = (L["N"], L["K"], L["group_size"], L["bits"])
    if key not in _dev:
        _dev[key] = tuple(torch.from_numpy(L[k]).to(hip) for k in ("qweight", "scales", "qzeros"))
    return _dev[key]


def _single(ops, hip, L, bias, dtype, order=None):
    qw, sc, qz = _layer_tensors(hip, L)
    return ops.WoqGemvAnywCall(qw, sc, qz, bias, L["N"], L["K"], L["group_size"], L["bits"], dtype, k_order=order)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the gathered launch
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
@pytest.mark.parametrize("kind", G.PERM_KINDS)
@pytest.mark.parametrize("c", G.PERM_CASES, ids=G.PERM_CASE_NAMES)
def test_perm_is_the_plain_kernel_on_the_gathered_x(hip, c, kind, dtype):
    from neural_compressor_amd import ops

    x, bias, p, ref, S = G.perm_reference(c, dtype, kind)
    L = A.layer_of(c)
    xd, bd, pd = x.to(hip), bias.to(hip), torch.from_numpy(p).to(hip)
    call = _single(ops, hip, L, bd, dtype, order=pd)
    assert call.ko is not None
    y = call(xd, checked=False)
    assert y.shape == (c.M, c.N) and y.dtype is dtype
    R.assert_elementwise(y, ref, S, c.K, dtype, f"{c.name} {kind}")                               # C3
    plain = _single(ops, hip, L, bd, dtype)
    assert torch.equal(y, plain(xd.index_select(1, pd.long()), checked=False)), "C1: not the plain kernel on x[:, p]"
    if kind == "identity":
        assert torch.equal(y, plain(xd, checked=False))
    assert torch.equal(call(xd, checked=False), y), "C4: a second call is not bit-identical"
    # x 2 bytes off a 16-byte boundary: the same bits
    buf = torch.zeros(8 + x.numel() + 8, dtype=dtype, device=hip)
    off = buf[9:9 + x.numel()].view(x.shape)
    off.copy_(xd)
    assert off.data_ptr() % 16 == 2
    assert torch.equal(call(off, checked=False), y), "an x that is only 2-byte aligned changed the result"


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
@pytest.mark.parametrize("name", ["b3_long_m16", "b6_tail4"])
def test_perm_clamps_entries_outside_the_row(hip, name, dtype):
    """A k_order holding -1 and K gives the bits of the same order with 0 and K - 1."""
    from neural_compressor_amd import ops

    c = next(c for c in G.PERM_CASES if c.name == name)
    x, bias, p, _, _ = G.perm_reference(c, dtype, "random")
    L = A.layer_of(c)
    xd, bd = x.to(hip), bias.to(hip)
    bad, good = p.copy(), p.copy()
    bad[3], good[3] = -1, 0
    bad[c.K - 2], good[c.K - 2] = c.K, c.K - 1
    yb = _single(ops, hip, L, bd, dtype, order=torch.from_numpy(bad).to(hip))(xd, checked=False)
    yg = _single(ops, hip, L, bd, dtype, order=torch.from_numpy(good).to(hip))(xd, checked=False)
    assert torch.equal(yb, yg)
    ref, S = R.reference(x[:, torch.from_numpy(good).long()], R.dense_weight64(L, dtype), bias)
    R.assert_elementwise(yg, ref, S, c.K, dtype, f"{name} clamped order")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the batched launch
# ---------------------------------------------------------------------------------------------------------------------------------------
def _entry_multi(hip, c, xd, dtype, tensors, biases, orders, ws):
    """inc_woq_gemv_anyw_multi on a workspace the test owns -> the outputs."""
    from neural_compressor_amd import _lib

    n = len(c.Ns)
    arr = lambda v: (ctypes.c_void_p * n)(*v)  # noqa: E731
    ys = [torch.empty(c.M, N, dtype=dtype, device=hip) for N in c.Ns]
    rc = _lib.lib.inc_woq_gemv_anyw_multi(
        n, xd.data_ptr(), _lib.INC_BF16 if dtype is torch.bfloat16 else _lib.INC_F16, None if orders is None else arr([o.data_ptr() for o in orders]),
        arr([t[0].data_ptr() for t in tensors]), arr([t[1].data_ptr() for t in tensors]), arr([t[2].data_ptr() for t in tensors]),
        arr([None if b is None else b.data_ptr() for b in biases]), arr([y.data_ptr() for y in ys]), c.M, (ctypes.c_int64 * n)(*c.Ns), c.K,
        c.group_size, c.bits, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() - WS_TAIL, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return ys


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
@pytest.mark.parametrize("mode", G.ORDER_MODES)
@pytest.mark.parametrize("c", G.GROUP_CASES, ids=G.GROUP_IDS)
def test_group_equals_the_single_launches(hip, c, mode, dtype):
    from neural_compressor_amd import _lib, ops

    x, biases, orders, outs = G.group_reference(c, dtype, mode)
    Ls = G.group_layers(c)
    xd = x.to(hip)
    bd = [None if b is None else b.to(hip) for b in biases]
    od = [None if p is None else torch.from_numpy(p).to(hip) for p in orders]
    tensors = [_layer_tensors(hip, L) for L in Ls]
    parts = [(t[0], t[1], t[2], b, N) for t, b, N in zip(tensors, bd, c.Ns)]
    call = ops.WoqGemvAnywGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=None if mode == "plain" else od)
    assert (call.ko is None) == (mode == "plain")
    ys = call(xd)
    assert isinstance(ys, list) and len(ys) == len(c.Ns), "the library declined the group"
    singles = [_single(ops, hip, L, b, dtype, order=o)(xd, checked=False) for L, b, o in zip(Ls, bd, od)]
    for i, (y, s, (ref, S)) in enumerate(zip(ys, singles, outs)):
        assert y.shape == (c.M, c.Ns[i]) and y.dtype is dtype
        assert torch.equal(y, s), f"C2: member {i} is not its single launch"
        R.assert_elementwise(y, ref, S, c.K, dtype, f"{c.name} {mode} member {i}")                # C3
    assert all(torch.equal(a, b) for a, b in zip(call(xd), ys)), "C4: a second call is not bit-identical"
    # the entry point on a workspace of exactly the declared size: counters back to zero, nothing written past it; then a single
    # launch on the same workspace gives its usual result
    need = _lib.lib.inc_woq_gemv_anyw_multi_workspace_bytes(len(c.Ns), c.M, (ctypes.c_int64 * len(c.Ns))(*c.Ns), c.K, c.bits)
    assert need == G.multi_workspace_bytes(c.M, c.Ns, c.K, c.bits)
    ws = None
    if need:
        ws = torch.full((need + WS_TAIL,), WS_SENTINEL, dtype=torch.uint8, device=hip)
        ws[:G.COUNTER_BYTES] = 0
    ident = torch.arange(c.K, dtype=torch.int32, device=hip)
    eo = None if mode == "plain" else [ident if o is None else o for o in od]
    for _ in range(2):
        ye = _entry_multi(hip, c, xd, dtype, tensors, bd, eo, ws)
        assert all(torch.equal(a, b) for a, b in zip(ye, ys))
        if ws is not None:
            assert bool((ws[:G.COUNTER_BYTES] == 0).all()), "the arrival counters did not return to zero"
            assert bool((ws[need:] == WS_SENTINEL).all()), "the workspace was written past inc_woq_gemv_anyw_multi_workspace_bytes"
    if ws is not None:
        i = len(c.Ns) - 1
        y1 = torch.empty(c.M, c.Ns[i], dtype=dtype, device=hip)
        qw, sc, qz = tensors[i]
        rc = _lib.lib.inc_woq_gemv_anyw(xd.data_ptr(), _lib.INC_BF16 if dtype is torch.bfloat16 else _lib.INC_F16, qw.data_ptr(), sc.data_ptr(),
                                        qz.data_ptr(), None if bd[i] is None else bd[i].data_ptr(), y1.data_ptr(), c.M, c.Ns[i], c.K, sc.shape[0],
                                        c.group_size, c.bits, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(y1, _single(ops, hip, Ls[i], bd[i], dtype)(xd, checked=False)), "C4: a single call after the group launch"
        assert bool((ws[:G.COUNTER_BYTES] == 0).all())


def test_group_call_declines_and_tracks_its_tensors(hip):
    from neural_compressor_amd import ops

    c, dtype = G.GROUP_CASES[1], torch.bfloat16
    tensors = [_layer_tensors(hip, L) for L in G.group_layers(c)]
    parts = [(t[0], t[1], t[2], None, N) for t, N in zip(tensors, c.Ns)]
    od = [torch.from_numpy(p).to(hip) for p in G.group_orders(c, "orders")]
    call = ops.WoqGemvAnywGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=od)
    assert call(R.make_x(17, c.K, dtype).to(hip)) is None                         # more than 16 rows: nothing launched
    assert call.current(parts, od) and not call.current(parts, None) and not call.current(parts, [od[1], od[0]])
    with pytest.raises(ValueError, match="bits=4"):
        ops.WoqGemvAnywGroupCall(parts, c.K, c.group_size, 4, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------------
MK, MGS, MBITS = 2080, 128, 3


def _module(hip, N, seed, act_order=True, bias=True, bits=MBITS):
    """An asymmetric g128 MI355XWeightOnlyLinear of `bits` bits, K = 2080 (a ragged last group); act_order: its g_idx permutes whole
    groups (a random permutation of K)."""
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    g = torch.Generator().manual_seed(seed)
    Gn = -(-MK // MGS)
    iw = torch.randint(0, 1 << bits, (N, MK), generator=g, dtype=torch.int32)
    sc = torch.rand(N, Gn, generator=g) * 0.02 + 0.002
    zp = torch.randint(1, 1 << bits, (N, Gn), generator=g, dtype=torch.int32)
    b = torch.randn(N, generator=g) if bias else None
    m = MI355XWeightOnlyLinear(MK, N, bits=bits, group_size=MGS, zp=True, bias=bias, g_idx=act_order, device=hip)
    m.pack(iw.to(hip), sc.to(hip), zp.to(hip), None if b is None else b.to(hip),
           g_idx=torch.randperm(MK, generator=g).to(hip) if act_order else None)
    if not bias:
        m.bias = None
    return m


def _module_oracle(m, x, dtype):
    """(ref, S) in float64 of the module's forward on x: the oracle's dense weight of the module's packed arrays and g_idx."""
    from oracle import woq_oracle as O

    gi = None if m.g_idx is None else m.g_idx.cpu().numpy()
    w = O.woq_dense_weight(m.qweight.cpu().numpy(), m.scales.cpu().numpy(), m.qzeros.cpu().numpy(), m.out_features, m.in_features, m.bits,
                           m.group_size, compute_dtype=dtype, g_idx=gi).double()
    b = torch.zeros(m.out_features, dtype=dtype) if m.bias is None else m.bias.to(dtype).cpu()
    return R.reference(x.cpu(), w, b)


def _no_recover(*a, **k):
    raise AssertionError("recover() ran on the decode path")


def _parent_route(m, x):
    """What forward computed before the decode kernel existed: HIP recover() + the library GEMM."""
    b = None if m.bias is None else m.bias.to(x.dtype)
    return torch.nn.functional.linear(x, m.recover(dtype=x.dtype), b)


def _whole_group_g_idx(hip, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.argsort(torch.randperm(MK, generator=g)) // MGS).to(torch.int32).to(hip)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
def test_act_order_module_decodes_without_recover(hip, dtype, monkeypatch):
    from neural_compressor_amd import ops

    m = _module(hip, 264, 71)
    assert m.ODD_WIDTH_DECODE is True and m.ACT_ORDER_FUSED_GATHER is True and m.ODD_WIDTH_FUSED is False
    monkeypatch.setattr(m, "recover", _no_recover)
    for M in (1, 16):
        x = R.make_x(M, MK, dtype)
        ref, S = _module_oracle(m, x, dtype)
        for _ in range(2):  # the call that builds the prepared call, then the fast path at the top of forward
            y = m(x.to(hip))
            R.assert_elementwise(y, ref, S, MK, dtype, f"module M = {M}")
            call = m.__dict__["_call"]
            assert isinstance(call, ops.WoqGemvAnywCall) and call.ko is not None
            assert call.gathers(1) and call.gathers(M) == (M * 264 <= m.ODD_WIDTH_GATHER_MAX_MN)
        y3 = m(x.to(hip).view(1, M, MK))
        assert y3.shape == (1, M, 264) and torch.equal(y3.view(M, 264), y)
    assert m._plan == "dense" and m._decode_anyw is False and m._decode_anyw_perm is True
    assert torch.equal(m._qweight_sorted, ops.sort_packed_k(m.qweight, m._k_order, MK, MBITS))


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
def test_act_order_module_one_hot_rows_equal_its_recover(hip, dtype):
    """C5: m(x) on one-hot rows is m.recover(dtype)[:, k], bit for bit (no bias)."""
    from neural_compressor_amd import ops

    m = _module(hip, 264, 72, bias=False)
    w = m.recover(dtype)
    ks = [0, 9, 10, 127, 128, 639, 640, 2047, 2048, MK - 1]
    x = torch.zeros(len(ks), MK, dtype=dtype)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    y = m(x.to(hip))
    assert isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall) and m.__dict__["_call"].ko is not None
    for i, k in enumerate(ks):
        assert torch.equal(y[i], w[:, k]), f"row for k = {k} is not recover()'s column"


def test_act_order_module_keeps_the_parent_route_elsewhere(hip):
    from neural_compressor_amd import ops

    dtype = torch.bfloat16
    m = _module(hip, 264, 73)
    x1 = R.make_x(1, MK, dtype).to(hip)
    y_decode = m(x1)
    assert isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall)
    xb = R.make_x(17, MK, dtype).to(hip)  # one row over the limit, right after a decode call
    assert torch.equal(m(xb), _parent_route(m, xb))
    assert m.__dict__.get("_call") is None
    for switch in ("ODD_WIDTH_DECODE", "ACT_ORDER_FUSED_GATHER"):
        m(x1)
        assert m.__dict__["_call"] is not None
        setattr(m, switch, False)
        assert torch.equal(m(x1), _parent_route(m, x1)), f"{switch} = False is not the parent's route"
        m(x1)
        assert m.__dict__.get("_call") is None
        setattr(m, switch, True)
        assert torch.equal(m(x1), y_decode)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
def test_gather_row_limit_changes_the_launches_not_the_bits(hip, dtype):
    """Up to ODD_WIDTH_GATHER_MAX_MN outputs (M x N) the kernel gathers; above, x.index_select + the plain kernel: bit-identical (C1)."""
    m = _module(hip, 264, 75)
    assert m.ODD_WIDTH_GATHER_MAX_MN >= 4096  # one row of a 4096-column module at the least
    x = R.make_x(5, MK, dtype).to(hip)
    outs, calls = [], [None]
    for limit in (5 * 264, 5 * 264 - 1, 5 * 264):
        m.ODD_WIDTH_GATHER_MAX_MN = limit
        for again in (False, True):  # the building call, then the fast path
            outs.append(m(x))
            call = m.__dict__["_call"]
            assert (call is calls[-1]) == again, "a new limit rebuilds the prepared call, the same limit keeps it"
            calls.append(call)
            assert call.ko is not None and call.gather_max_mn == limit and call.gathers(5) == (limit == 5 * 264) and call.gathers(4)
    assert all(torch.equal(o, outs[0]) for o in outs)
    ref, S = _module_oracle(m, x.cpu(), dtype)
    R.assert_elementwise(outs[0], ref, S, MK, dtype, "module M = 5")


def test_rewritten_g_idx_rebuilds_the_sorted_words_and_the_call(hip):
    dtype = torch.float16
    m = _module(hip, 264, 74)
    x = R.make_x(4, MK, dtype)
    y_old = m(x.to(hip))
    call_old, sorted_old = m.__dict__["_call"], m._qweight_sorted
    m.g_idx.copy_(_whole_group_g_idx(hip, 5))
    y_new = m(x.to(hip))
    assert m.__dict__["_call"] is not call_old and m._qweight_sorted is not sorted_old and m._decode_anyw_perm
    assert not torch.equal(y_new, y_old)
    ref, S = _module_oracle(m, x, dtype)
    R.assert_elementwise(y_new, ref, S, MK, dtype, "after g_idx was rewritten")
    # groups of uneven size: the dense route
    g = m.g_idx.clone()
    g[g == 1] = 0
    m.g_idx.copy_(g)
    y = m(x.to(hip))
    assert m._decode_anyw_perm is False and m._plan == "dense" and m.__dict__.get("_call") is None
    assert torch.equal(y, _parent_route(m, x.to(hip)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# woq_linear_group
# ---------------------------------------------------------------------------------------------------------------------------------------
def _parts_of(mods):
    return ([(m._qweight_sorted if m._decode_anyw_perm else m.qweight, m.scales, m.qzeros, m.bias, m.out_features) for m in mods],
            [m._k_order32 if m._decode_anyw_perm else None for m in mods])


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
def test_woq_linear_group_takes_odd_width_members_in_one_launch(hip, dtype):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only import modules as W

    mods = [_module(hip, 264, 81), _module(hip, 64, 82, act_order=False), _module(hip, 204, 83, bias=False)]
    states = [{k: v.clone() for k, v in m.state_dict().items()} for m in mods]
    rows = 5
    assert 16 * 264 <= W.MI355XWeightOnlyLinear.ODD_WIDTH_GATHER_MAX_MN  # the kernel gathers for every row count at these widths
    x = R.make_x(rows, MK, dtype).to(hip)
    ys = W.woq_linear_group(x, mods)
    key = tuple(id(m) for m in mods[1:]) + (dtype,)
    call = mods[0].__dict__["_group_calls"][key]
    assert isinstance(call, ops.WoqGemvAnywGroupCall) and call.ko is not None
    parts, orders = _parts_of(mods)
    assert orders[1] is None and orders[0] is not None and orders[2] is not None
    direct = ops.WoqGemvAnywGroupCall(parts, MK, MGS, MBITS, dtype, k_orders=orders)(x)
    assert isinstance(direct, list) and all(torch.equal(a, b) for a, b in zip(ys, direct))
    assert all(torch.equal(a, m(x)) for a, m in zip(ys, mods)), "a grouped output is not the single call's"
    for i, (m, y) in enumerate(zip(mods, ys)):
        ref, S = _module_oracle(m, x, dtype)
        R.assert_elementwise(y, ref, S, MK, dtype, f"member {i}")
    assert all(torch.equal(a, b) for a, b in zip(W.woq_linear_group(x, mods), ys))
    assert mods[0].__dict__["_group_calls"][key] is call, "the prepared call was rebuilt"
    y3 = W.woq_linear_group(x.view(1, rows, MK), mods)
    assert all(a.shape == (1, rows, m.out_features) and torch.equal(a.view(rows, -1), b) for a, b, m in zip(y3, ys, mods))
    # 16 rows: one launch while the widest member's outputs are within ODD_WIDTH_GATHER_MAX_MN, the single calls (index_select in
    # front of the plain kernel) beyond -- the same bits
    x16 = R.make_x(16, MK, dtype).to(hip)
    y16 = W.woq_linear_group(x16, mods)
    direct16 = ops.WoqGemvAnywGroupCall(parts, MK, MGS, MBITS, dtype, k_orders=orders)(x16)
    assert all(torch.equal(a, b) for a, b in zip(y16, direct16)) and all(torch.equal(a, m(x16)) for a, m in zip(y16, mods))
    mods[0].ODD_WIDTH_GATHER_MAX_MN = 16 * 264 - 1
    mods[0].__dict__.pop("_group_calls")
    y16b = W.woq_linear_group(x16, mods)
    assert "_group_calls" not in mods[0].__dict__, "a group beyond the gather limit took the one launch"
    assert not mods[0].__dict__["_call"].gathers(16) and mods[2].__dict__["_call"].gathers(16)
    assert all(torch.equal(a, b) for a, b in zip(y16b, y16))
    del mods[0].ODD_WIDTH_GATHER_MAX_MN
    W.woq_linear_group(x, mods)
    plain_only = [mods[1], _module(hip, 68, 85, act_order=False)]
    yp = W.woq_linear_group(x16, plain_only)  # no act_order member: the gather limit does not apply
    assert isinstance(plain_only[0].__dict__["_group_calls"][(id(plain_only[1]), dtype)], ops.WoqGemvAnywGroupCall)
    assert all(torch.equal(a, m(x16)) for a, m in zip(yp, plain_only))
    for m, st in zip(mods, states):
        now = m.state_dict()
        assert set(now) == set(st) and all(torch.equal(now[k], st[k]) for k in st)
    # more rows than the kernel takes, and a switch off: the single calls
    xb = R.make_x(17, MK, dtype).to(hip)
    assert all(torch.equal(a, m(xb)) for a, m in zip(W.woq_linear_group(xb, mods), mods))
    cls = W.MI355XWeightOnlyLinear
    cls.ACT_ORDER_FUSED_GATHER = False
    try:
        off = W.woq_linear_group(x, mods)
        assert all(torch.equal(a, m(x)) for a, m in zip(off, mods))
        assert torch.equal(off[0], _parent_route(mods[0], x)) and torch.equal(off[1], ys[1])
    finally:
        cls.ACT_ORDER_FUSED_GATHER = True
    # a 4-bit member in the list: single calls
    four = _module(hip, 64, 84, act_order=False, bits=4)
    mixed = [mods[0], four]
    mods[0].__dict__.pop("_group_calls")
    ym = W.woq_linear_group(x, mixed)
    assert "_group_calls" not in mods[0].__dict__
    assert torch.equal(ym[0], ys[0]) and torch.equal(ym[1], four(x))


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
def test_woq_gated_pair_of_odd_width_members_uses_the_group_launch(hip, dtype):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only import modules as W

    gate, up = _module(hip, 264, 91, bias=False), _module(hip, 264, 92, bias=False)
    x = R.make_x(4, MK, dtype).to(hip)
    h = W.woq_gated_pair(x, gate, up)
    assert isinstance(gate.__dict__["_group_calls"][(id(up), dtype)], ops.WoqGemvAnywGroupCall)
    assert torch.equal(h, torch.nn.functional.silu(gate(x)) * up(x))


# ---------------------------------------------------------------------------------------------------------------------------------------
# a model
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_tiny_llama_3bit_act_order_one_token_logits(hip, monkeypatch):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear
    from neural_compressor_amd.torch.quantization import RTNConfig, quantize
    from tests.model_zoo import calib_ids, tiny_llama

    q = quantize(tiny_llama(), RTNConfig(bits=3, group_size=32, use_sym=False, use_layer_wise=False))
    mods = [m for m in q.modules() if isinstance(m, MI355XWeightOnlyLinear)]
    assert len(mods) == 14
    g = torch.Generator().manual_seed(11)
    for m in mods:  # a whole-group g_idx per module, the same for both runs
        m.g_idx = (torch.argsort(torch.randperm(m.in_features, generator=g)) // 32).to(torch.int32).to(m.qweight.device)
    ids = calib_ids()[0][:, :1].to("cuda")
    with torch.no_grad():
        on = q(ids).logits.float().cpu()
        took = sum(isinstance(m.__dict__.get("_call"), ops.WoqGemvAnywCall) and m.__dict__["_call"].ko is not None for m in mods)
        monkeypatch.setattr(MI355XWeightOnlyLinear, "ODD_WIDTH_DECODE", False)
        off = q(ids).logits.float().cpu()
    assert took == 14, f"only {took} of 14 modules hold a gathered call"
    assert all(m.__dict__.get("_call") is None for m in mods)
    assert torch.isfinite(on).all() and float((on - off).norm() / off.norm()) <= 2e-3
