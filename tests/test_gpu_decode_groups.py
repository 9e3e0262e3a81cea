"""-m gpu: the one-launch decode groups -- act_order members in the batched launch (inc_woq_gemm_multi_perm) and gate / up with the SiLU
product in the same launch (inc_woq_gemm_gated, built in form (i): the strips of gate and up share a ticket, the last arriver forms the
product from the two fixed-order fp32 sums).  Cases, inputs, references and bounds: tests/decode_group_cases.py.

Part A, every case x M, bf16 and fp16, with bias:
  identity  output i of the gathered group call is torch.equal to output i of the plain group call on x.index_select(1, p_i) -- orders
            that differ per member, and a group whose last member has no order (the identity) -- and a second call is bit-identical;
  oracle    every output element within gemm_route_cases.tolerance of float64 x[:, p_i] @ W_i^T + b_i;
  modules   woq_linear_group on three act_order MI355XWeightOnlyLinear takes the one-launch path, agrees with the single calls within
            the oracle's bound, equals them bit for bit with ACT_ORDER_FUSED_GATHER off, follows a rewritten g_idx, leaves the state
            dicts alone.
Part B, every 4-bit case with two equal members, M <= 16:
  oracle    h within moe_stage_cases.mode0_tolerance of float64 silu(g) u;
  repeat    two calls are torch.equal, and a plain group call on the same cached workspace still returns its earlier bits (the shared
            counters were re-armed);
  gathered  one order shared by gate and up: torch.equal to the un-gathered entry on x.index_select; two orders (each member through its
            own): within the oracle's bound for g = x[:, p_g] . Wg, u = x[:, p_u] . Wu;
  helper    woq_gated_pair: fused within the bound, every fallback torch.equal to the unfused expression.
Before a launch every case is asserted to sit on the rung it was written for (decode_group_cases.assert_on_rung).
"""

import copy

import pytest
import torch
import torch.nn.functional as F

from tests import decode_group_cases as D
from tests import gemm_route_cases as R
from tests import moe_stage_cases as MS

pytestmark = pytest.mark.gpu

_dev_layers = {}


def _part(hip, L, bias=None):
    key = (L["N"], L["K"], L["group_size"], L["bits"], L["member"])
    if key not in _dev_layers:
        _dev_layers[key] = tuple(torch.from_numpy(L[k]).to(hip) for k in ("qweight", "scales", "qzeros"))
    return (*_dev_layers[key], None if bias is None else bias.to(hip), L["N"])


def _order_tensors(hip, ps):
    out = [None if p is None else torch.from_numpy(p).to(hip) for p in ps]
    assert all(t is None or (t.dtype is torch.int32 and t.data_ptr() % 16 == 0) for t in out)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# part A: the entry through ops.WoqGemmGroupCall
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
@pytest.mark.parametrize("c,M", D.PARAMS, ids=D.PARAM_IDS)
def test_group_perm_is_the_plain_group_on_the_gathered_x_and_within_the_oracle_bound(hip, c, M, dtype):
    from neural_compressor_amd import ops

    D.assert_on_rung(c, M, dtype)
    Ls = D.layers(c)
    for mixed in (False, True):
        x_cpu, biases, outs = D.group_reference(c, M, dtype, mixed)
        x = x_cpu.to(hip)
        parts = [_part(hip, L, b) for L, b in zip(Ls, biases)]
        ps = _order_tensors(hip, D.orders(c, mixed))
        plain = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype)
        call = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=ps)
        assert call.ko is not None and plain.ko is None
        ys = call(x)
        assert ys is not None, "the library declined an eligible act_order group"
        again = call(x)
        for i, (p, (ref, S)) in enumerate(zip(ps, outs)):
            assert torch.equal(again[i], ys[i]), f"member {i}: a second call is not bit-identical"
            want = plain(x if p is None else x.index_select(1, p))[i]
            assert torch.equal(ys[i], want), f"member {i} (mixed = {mixed}): differs from the plain group call on the gathered x"
            r = R.assert_elementwise(ys[i], ref, S, c.K, dtype, f"{c.name} M = {M} member {i} mixed = {mixed}")
            print(f"\n[decode group A] {c.name} m{M} {str(dtype)[6:]} member {i} mixed={mixed}: worst err / tol {r:.3f}")
        assert call.current(parts, ps) and not call.current(parts, None) and not plain.current(parts, ps)


def test_group_perm_declines_and_tracks_its_orders(hip):
    from neural_compressor_amd import ops

    c, dtype = D.case("ragged"), torch.bfloat16
    parts = [_part(hip, L) for L in D.layers(c)]
    ps = _order_tensors(hip, D.orders(c))
    call = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=ps)
    assert call(R.make_x(65, c.K, dtype).to(hip)) is None            # as inc_woq_gemm_multi: more than 64 rows, nothing launched
    x = R.make_x(5, c.K, dtype).to(hip)
    buf = torch.zeros(c.K + 4, dtype=torch.int32, device=hip)
    off = buf[1:1 + c.K]
    off.copy_(ps[0])
    assert off.data_ptr() % 16 == 4
    assert ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=[off, ps[1]])(x) is None  # a misaligned order
    # entries outside [0, K-1] are clamped, never followed
    bad, clamped = ps[0].clone(), ps[0].clone()
    bad[3], clamped[3] = -1, 0
    bad[c.K - 5], clamped[c.K - 5] = c.K, c.K - 1
    y_bad = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=[bad, ps[1]])(x)
    y_ok = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=[clamped, ps[1]])(x)
    assert bool(torch.isfinite(y_bad[0].float()).all()) and all(torch.equal(a, b) for a, b in zip(y_bad, y_ok))
    # current(): the order tensors by identity and version
    assert call.current(parts, ps)
    assert not call.current(parts, [ps[0].clone(), ps[1]])
    ps[1][0:2] = ps[1][[1, 0]]
    assert not call.current(parts, ps)


# ---------------------------------------------------------------------------------------------------------------------------------------
# part A: modules
# ---------------------------------------------------------------------------------------------------------------------------------------
MK, MGS = 1024, 128


def _module(hip, N, seed, act_order=True, bias=True):
    """An asymmetric INT4 g128 MI355XWeightOnlyLinear; act_order: its g_idx permutes whole groups (a random permutation of K)."""
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    g = torch.Generator().manual_seed(seed)
    iw = torch.randint(0, 16, (N, MK), generator=g, dtype=torch.int32)
    sc = torch.rand(N, MK // MGS, generator=g) * 0.02 + 0.002
    zp = torch.randint(1, 16, (N, MK // MGS), generator=g, dtype=torch.int32)
    b = torch.randn(N, generator=g) if bias else None
    m = MI355XWeightOnlyLinear(MK, N, bits=4, group_size=MGS, zp=True, bias=bias, g_idx=act_order, device=hip)
    m.pack(iw.to(hip), sc.to(hip), zp.to(hip), None if b is None else b.to(hip),
           g_idx=torch.randperm(MK, generator=g).to(hip) if act_order else None)
    if not bias:
        m.bias = None
    assert m._forward_plan() == ("fused_act_order" if act_order else "fused")
    return m


def _module_oracle(m, x, dtype):
    """(ref, S) in float64 of the module's forward on x, from its own recover() in the compute dtype."""
    w = m.recover(dtype=dtype).double().cpu()
    b = torch.zeros(m.out_features, dtype=dtype) if m.bias is None else m.bias.to(dtype).cpu()
    return R.reference(x.cpu(), w, b)


def _sorted_parts(mods):
    return ([(m._qweight_sorted if m._k_order32 is not None else m.qweight, m.scales, m.qzeros, m.bias, m.out_features) for m in mods],
            [m._k_order32 for m in mods])


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
def test_woq_linear_group_takes_act_order_modules_in_one_launch(hip, dtype):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only import modules as W

    mods = [_module(hip, N, 41 + i) for i, N in enumerate((264, 64, 328))]
    states = [{k: v.clone() for k, v in m.state_dict().items()} for m in mods]
    x = R.make_x(5, MK, dtype).to(hip)

    def check(ys, what):
        for i, (m, y) in enumerate(zip(mods, ys)):
            ref, S = _module_oracle(m, x, dtype)
            R.assert_elementwise(y, ref, S, MK, dtype, f"{what}, member {i}")

    ys = W.woq_linear_group(x, mods)
    parts, orders = _sorted_parts(mods)
    direct = ops.WoqGemmGroupCall(parts, MK, MGS, 4, dtype, k_orders=orders)(x)
    assert isinstance(direct, list), "the library declined an act_order group"
    assert all(torch.equal(a, b) for a, b in zip(ys, direct)), "woq_linear_group did not take the one-launch path"
    call = mods[0].__dict__["_group_calls"][tuple(id(m) for m in mods[1:]) + (dtype,)]
    assert call.ko is not None
    assert all(torch.equal(a, b) for a, b in zip(W.woq_linear_group(x, mods), ys))
    assert mods[0].__dict__["_group_calls"][tuple(id(m) for m in mods[1:]) + (dtype,)] is call, "the prepared call was rebuilt"
    check(ys, "one launch")
    check([m(x) for m in mods], "single calls")
    y3 = W.woq_linear_group(x.view(1, 5, MK), mods)
    assert all(a.shape == (1, 5, m.out_features) and torch.equal(a.view(5, -1), b) for a, b, m in zip(y3, ys, mods))
    # switched off: the single calls, bit for bit
    cls = W.MI355XWeightOnlyLinear
    assert cls.ACT_ORDER_FUSED_GATHER is True
    cls.ACT_ORDER_FUSED_GATHER = False
    try:
        off = W.woq_linear_group(x, mods)
        assert all(torch.equal(a, m(x)) for a, m in zip(off, mods))
    finally:
        cls.ACT_ORDER_FUSED_GATHER = True
    # a plain member in the group: the identity order
    plain = _module(hip, 200, 47, act_order=False)
    mixed = [mods[0], plain, mods[2]]
    ym = W.woq_linear_group(x, mixed)
    parts_m, orders_m = _sorted_parts(mixed)
    assert orders_m[1] is None
    dm = ops.WoqGemmGroupCall(parts_m, MK, MGS, 4, dtype, k_orders=orders_m)(x)
    assert isinstance(dm, list) and all(torch.equal(a, b) for a, b in zip(ym, dm))
    assert torch.equal(ym[0], ys[0]) and torch.equal(ym[2], ys[2])
    ref, S = _module_oracle(plain, x, dtype)
    R.assert_elementwise(ym[1], ref, S, MK, dtype, "the plain member of a mixed group")
    # the state dicts are untouched
    for m, st in zip(mods, states):
        now = m.state_dict()
        assert set(now) == set(st) and all(torch.equal(now[k], st[k]) for k in st)
    # another permutation of whole groups written into one member's g_idx: the result follows the new order
    g = torch.Generator().manual_seed(5)
    mods[1].g_idx.copy_((torch.argsort(torch.randperm(MK, generator=g)) // MGS).to(torch.int32).to(hip))
    y2 = W.woq_linear_group(x, mods)
    assert mods[1]._plan == "fused_act_order"
    assert mods[0].__dict__["_group_calls"][tuple(id(m) for m in mods[1:]) + (dtype,)] is not call
    assert torch.equal(y2[0], ys[0]) and torch.equal(y2[2], ys[2]) and not torch.equal(y2[1], ys[1])
    check(y2, "after g_idx was rewritten")
    parts2, orders2 = _sorted_parts(mods)
    d2 = ops.WoqGemmGroupCall(parts2, MK, MGS, 4, dtype, k_orders=orders2)(x)
    assert all(torch.equal(a, b) for a, b in zip(y2, d2))


def test_woq_linear_group_guards_device_and_width(hip):
    """x of another width reaches the modules' own error instead of a reshape of the wrong size."""
    from neural_compressor_amd.torch.algorithms.weight_only import modules as W

    mods = [_module(hip, 64, 61, act_order=False), _module(hip, 64, 62, act_order=False)]
    x = R.make_x(4, MK // 2, torch.bfloat16).to(hip)  # 4 x 512 elements reshape to 2 x 1024 without the guard
    with pytest.raises(Exception):
        W.woq_linear_group(x, mods)
    assert "_group_calls" not in mods[0].__dict__


# ---------------------------------------------------------------------------------------------------------------------------------------
# part B: the entry through ops.WoqGatedCall
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
@pytest.mark.parametrize("c,M", D.GATED_PARAMS, ids=D.GATED_PARAM_IDS)
def test_gated_within_the_oracle_bound_repeatable_and_gathered(hip, c, M, dtype):
    from neural_compressor_amd import ops

    Ns = D.gated_ns(c)
    D.assert_on_rung(c, M, dtype, Ns)
    Lg, Lu = D.layers(c, Ns)
    gp, up = _part(hip, Lg), _part(hip, Lu)
    x_cpu, ref, tol = D.gated_reference(c, M, dtype)
    x = x_cpu.to(hip)
    group = ops.WoqGemmGroupCall([gp, up], c.K, c.group_size, 4, dtype)
    gu0 = group(x)
    assert gu0 is not None
    call = ops.WoqGatedCall(gp, up, c.K, c.group_size, 4, dtype)
    h = call(x)
    assert h is not None, "the library declined an eligible pair"
    r = MS.assert_elementwise(h, ref, tol, f"{c.name} M = {M}")
    print(f"\n[decode group B] {c.name} m{M} {str(dtype)[6:]}: worst err / tol {r:.3f}")
    assert torch.equal(call(x), h), "a second call is not bit-identical"
    # the same cached (device, stream) workspace: the shared counters are back at zero, the plain group call returns its earlier bits
    ws = ops._ws_cache[(x.device.index, torch.cuda.current_stream().cuda_stream)]
    assert not bool(ws[:D.COUNTER_BYTES].any()), "arrival counters are not back at zero"
    gu1 = group(x)
    assert all(torch.equal(a, b) for a, b in zip(gu0, gu1))
    assert torch.equal(call(x), h)
    # the unfused product of the rounded g and u is within a few output roundings of h: the same sums went in
    u_out = MS.out_rounding(dtype)[0]
    unfused = (F.silu(gu0[0].float()) * gu0[1].float())
    assert bool(((h.float() - unfused).abs() <= 4 * u_out * (unfused.abs() + gu0[0].float().abs() * gu0[1].float().abs()) + 1e-6).all())
    # gathered, one order shared: bit-identical to the un-gathered entry on the gathered x
    p0, p1 = _order_tensors(hip, D.orders(c, n=2))
    shared = ops.WoqGatedCall(gp, up, c.K, c.group_size, 4, dtype, k_orders=[p0, p0])
    hs = shared(x)
    assert hs is not None and torch.equal(hs, call(x.index_select(1, p0))), "shared order: differs from the entry on the gathered x"
    # gathered, each member through its own order; and a pair of which only gate has one
    for ps in (D.orders(c, n=2), [D.orders(c, n=2)[0], None]):
        _, ref2, tol2 = D.gated_reference(c, M, dtype, tuple(ps))
        two = ops.WoqGatedCall(gp, up, c.K, c.group_size, 4, dtype, k_orders=_order_tensors(hip, ps))
        h2 = two(x)
        assert h2 is not None and torch.equal(two(x), h2)
        MS.assert_elementwise(h2, ref2, tol2, f"{c.name} M = {M}, orders {'gate and up' if ps[1] is not None else 'gate only'}")
    assert not bool(ws[:D.COUNTER_BYTES].any())


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
def test_gated_declines_above_its_row_limit(hip, dtype):
    from neural_compressor_amd import ops

    c = D.case("ragged")
    Lg, Lu = D.layers(c, D.gated_ns(c))
    call = ops.WoqGatedCall(_part(hip, Lg), _part(hip, Lu), c.K, c.group_size, 4, dtype)
    assert ops.WoqGatedCall.MAX_M == D.GATED_MAX_M
    assert call(R.make_x(D.GATED_OVER_M, c.K, dtype).to(hip)) is None
    assert call(R.make_x(D.GATED_MAX_M, c.K, dtype).to(hip)) is not None


# ---------------------------------------------------------------------------------------------------------------------------------------
# part B: the helper
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pair_oracle(gate, up, x, dtype):
    xc = x.cpu().double()
    wg, wu = gate.recover(dtype=dtype).double().cpu(), up.recover(dtype=dtype).double().cpu()
    g, u = xc @ wg.t(), xc @ wu.t()
    return MS.mode0_tolerance(g, u, MS.accum_bound(MK, xc.abs() @ wg.abs().t()), MS.accum_bound(MK, xc.abs() @ wu.abs().t()), dtype)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
def test_woq_gated_pair_fused_and_every_fallback(hip, dtype):
    """Rows: 5 and 16 fused, 17 above the limit.  (From 5 rows on a single call of these layers takes the streaming kernel with the
    plan of the group, so the fallbacks can be compared with the single calls bit for bit.)"""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only import modules as W

    N = 264
    gate, up = _module(hip, N, 71, act_order=False, bias=False), _module(hip, N, 72, act_order=False, bias=False)
    keys = set(gate.state_dict())
    assert W.GATED_FUSED is True
    for M in (5, 16):
        x = R.make_x(M, MK, dtype).to(hip)
        h = W.woq_gated_pair(x, gate, up)
        call = gate.__dict__["_gated_calls"][(id(up), dtype)]
        assert isinstance(call, ops.WoqGatedCall) and torch.equal(call(x), h), "the fused path did not run"
        ref, tol = _pair_oracle(gate, up, x, dtype)
        MS.assert_elementwise(h, ref, tol, f"woq_gated_pair M = {M}")
        assert torch.equal(W.woq_gated_pair(x, gate, up, act_fn=torch.nn.SiLU()), h)
        assert gate.__dict__["_gated_calls"][(id(up), dtype)] is call, "the prepared call was rebuilt"
        unfused = F.silu(gate(x)) * up(x)
        W.GATED_FUSED = False
        try:
            assert torch.equal(W.woq_gated_pair(x, gate, up), unfused)
        finally:
            W.GATED_FUSED = True
        # leading dimensions are kept
        h3 = W.woq_gated_pair(x.view(1, M, MK), gate, up)
        assert h3.shape == (1, M, N) and torch.equal(h3.view(M, N), h)
    assert set(gate.state_dict()) == keys
    clone = copy.deepcopy(gate)
    assert not any(clone.__dict__.get("_gated_calls", {}).values()), "a copy carries the prepared call"
    x = R.make_x(5, MK, dtype).to(hip)
    h = W.woq_gated_pair(x, gate, up)
    assert torch.equal(W.woq_gated_pair(x, clone, up), h)
    # fallbacks: exactly the unfused expression
    gelu = torch.nn.GELU()
    assert torch.equal(W.woq_gated_pair(x, gate, up, act_fn=gelu), gelu(gate(x)) * up(x))
    x17 = R.make_x(D.GATED_OVER_M, MK, dtype).to(hip)
    assert torch.equal(W.woq_gated_pair(x17, gate, up), F.silu(gate(x17)) * up(x17))
    x32 = x.float()
    y32 = W.woq_gated_pair(x32, gate, up)
    assert y32.dtype is torch.float32 and torch.equal(y32, F.silu(gate(x32)) * up(x32))
    biased = _module(hip, N, 73, act_order=False, bias=True)
    assert torch.equal(W.woq_gated_pair(x, biased, up), F.silu(biased(x)) * up(x))
    assert "_gated_calls" not in biased.__dict__
    # a replaced buffer rebuilds the prepared call
    other = _module(hip, N, 74, act_order=False, bias=False)
    call = gate.__dict__["_gated_calls"][(id(up), dtype)]
    up.qweight, up.scales, up.qzeros = other.qweight.clone(), other.scales.clone(), other.qzeros.clone()
    h_new = W.woq_gated_pair(x, gate, up)
    assert gate.__dict__["_gated_calls"][(id(up), dtype)] is not call and not torch.equal(h_new, h)
    ref, tol = _pair_oracle(gate, up, x, dtype)
    MS.assert_elementwise(h_new, ref, tol, "after up's buffers were replaced")


@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.DTYPE_IDS)
def test_woq_gated_pair_act_order_members_gather_through_their_own_orders(hip, dtype):
    from neural_compressor_amd.torch.algorithms.weight_only import modules as W

    N = 264
    gate, up = _module(hip, N, 81, bias=False), _module(hip, N, 82, bias=False)
    assert not torch.equal(gate._k_order32, up._k_order32)
    x = R.make_x(5, MK, dtype).to(hip)
    h = W.woq_gated_pair(x, gate, up)
    call = gate.__dict__["_gated_calls"][(id(up), dtype)]
    assert call.ko[0] == gate._k_order32.data_ptr() and call.ko[1] == up._k_order32.data_ptr()
    ref, tol = _pair_oracle(gate, up, x, dtype)
    MS.assert_elementwise(h, ref, tol, "act_order pair")
    cls = W.MI355XWeightOnlyLinear
    cls.ACT_ORDER_FUSED_GATHER = False
    try:
        assert torch.equal(W.woq_gated_pair(x, gate, up), F.silu(gate(x)) * up(x))
    finally:
        cls.ACT_ORDER_FUSED_GATHER = True
