"""-m gpu: the routed MX GEMM of the fused MoE experts (inc_mx_moe_gemm) and MXExperts against the oracle of tests/mx_moe_cases.py.

  exact     every case of the table x three pairs (mode 0: bf16 and fp16; mode 1: fp32 and bf16 routing weights) x both scale rules:
            modes 2 / 1 bit-equal to the float64 result, mode 0 within the rounding of the output plus a few fp32 ulp.  `out` sits in a
            sentinel window, rows past the valid positions and the guards stay untouched, source rows no valid position names hold 0xFF
            codes and 0xFF scale bytes, repeated calls are bit-identical, and the route buffer comes from the oracle, not the route kernel;
  random    Gaussian operands through the oracle quantiser, within the bound of an fp32 chain in any order (worst ratio printed);
  one expert  mode 2 on one expert that holds every row == inc_mx_gemv (<= 16 rows) and inc_mx_gemm, bit for bit;
  rejections  each return code, with nothing written;
  module    the fused forward == the chain of the six ops calls bit for bit; both routes against a float64 emulation fed the fused
            route's own h; from_float / recover against the oracle quantiser;
  model     tiny_mixtral / tiny_qwen3_moe: every experts module becomes MXExperts, finite forward, save -> load bit-identical.
"""

import pytest
import torch

from tests import moe_models
from tests import moe_stage_cases as S
from tests import mx_cases as C
from tests import mx_moe_cases as M

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x7B5A, 0x7B5A7B5A
GUARD = 16                      # elements in front of the window (keeps it 16-byte aligned) and behind it
DTYPES16 = [torch.bfloat16, torch.float16]
DTYPE_IDS16 = ["bf16", "fp16"]
PIPE = 2.0 ** -8                # per-term allowance of the module-level emulation (_emulate_second_half)


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float32: _lib.INC_F32, torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


def _route_on(hip, ro):
    return S.route_buffer(ro, fill=-1).to(hip)


def _launch(hip, mode, aq, as_, afmt, route, wq, ws, wfmt, rw, odtype, T, k):
    """One call of inc_mx_moe_gemm with `out` inside sentinels -> (rc, the whole window as raw ints [S, Nout] on the CPU, guards ok)."""
    from neural_compressor_amd import _lib

    E, N = wq.shape[:2]
    Kp = ws.shape[2] * 32
    Sn, Nout = T * k, (N // 2 if mode == 0 else N)
    idt, sent = (torch.int16, SENT16) if mode == 0 else (torch.int32, SENT32)
    buf = torch.full((GUARD + Sn * Nout + GUARD,), sent, dtype=idt, device=hip)
    win = buf[GUARD:GUARD + Sn * Nout]
    assert win.data_ptr() % 16 == 0
    rc = _lib.lib.inc_mx_moe_gemm(mode, aq.data_ptr(), as_.data_ptr(), afmt, route.data_ptr(), wq.data_ptr(), ws.data_ptr(), wfmt,
                                  None if rw is None else rw.data_ptr(), _code(rw.dtype) if rw is not None else _lib.INC_F32,
                                  win.data_ptr(), _code(odtype), T, k, E, N, Kp, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    guards = bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + Sn * Nout:] == sent).all())
    return rc, win.cpu().view(Sn, Nout), guards


def _run_exact(hip, d, pair, odtype=None, wdtype=torch.float32):
    """The exact case d on the device -> the valid rows of the output (CPU, in its float type), every side condition asserted."""
    afmt, wfmt = pair
    mode, ro = d["mode"], d["ro"]
    aq, as_, wq, ws = (t.to(hip) for t in M.stored_operands(d, afmt, wfmt, poison=True))
    rw = d["rw"].to(wdtype).to(hip) if mode == 1 else None
    otype = odtype if mode == 0 else torch.float32
    args = (hip, mode, aq, as_, afmt, _route_on(hip, ro), wq, ws, wfmt, rw, otype, ro["T"], ro["k"])
    rc, raw, guards = _launch(*args)
    assert rc == 0, rc
    assert guards, "wrote around out"
    sent = SENT16 if mode == 0 else SENT32
    nv = ro["nvalid"]
    assert bool((raw[nv:] == sent).all()), "wrote a row past the valid positions"
    rc2, raw2, _ = _launch(*args)
    assert rc2 == 0 and torch.equal(raw, raw2), "repeated calls differ"
    return raw[:nv].contiguous().view(otype)


def _variants(mode):
    """(odtype, wdtype) a mode is run with."""
    if mode == 0:
        return [(dt, torch.float32) for dt in DTYPES16]
    if mode == 1:
        return [(None, torch.float32), (None, torch.bfloat16)]
    return [(None, torch.float32)]


# ---- the entry point on exact operands -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_exact_operands(hip, cm, pair):
    c, mode = cm
    for rule in M.RULES:
        d = M.exact_case(c, mode, rule)
        M.assert_exact_condition(d)
        for odtype, wdtype in _variants(mode):
            y = _run_exact(hip, d, pair, odtype, wdtype)
            why = M.check_output(d, y, odtype)
            assert why is None, f"{c.name} mode {mode} {rule} {odtype} {wdtype}: {why}"


def test_fp16_routing_weights(hip):
    d = M.exact_case(M.case("kW"), 1, "block")
    y = _run_exact(hip, d, C.PAIRS[0], None, torch.float16)
    assert M.check_output(d, y) is None


def test_poisoned_rows_do_not_change_valid_outputs(hip):
    """The same call with the unnamed source rows as ordinary data gives the same bits."""
    for name, mode in (("short_waves", 0), ("kW_plus1", 1), ("short_waves", 2)):
        d = M.exact_case(M.case(name), mode, "block")
        assert not bool(d["named"].all())
        afmt, wfmt = C.PAIRS[1]
        ro = d["ro"]
        outs = []
        for poison in (True, False):
            aq, as_, wq, ws = (t.to(hip) for t in M.stored_operands(d, afmt, wfmt, poison=poison))
            rw = d["rw"].float().to(hip) if mode == 1 else None
            rc, raw, _ = _launch(hip, mode, aq, as_, afmt, _route_on(hip, ro), wq, ws, wfmt, rw,
                                 torch.bfloat16 if mode == 0 else torch.float32, ro["T"], ro["k"])
            assert rc == 0
            outs.append(raw)
        assert torch.equal(*outs), (name, mode)


# ---- random operands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_random_operands_are_within_the_chain_bound(hip, mode, pair):
    afmt, wfmt = pair
    d = M.random_case(mode, afmt, wfmt)
    ro = d["ro"]
    rw = d["rw"].to(hip) if mode == 1 else None
    for odtype in (DTYPES16 if mode == 0 else [None]):
        otype = odtype if mode == 0 else torch.float32
        rc, raw, guards = _launch(hip, mode, d["aq"].to(hip), d["as_"].to(hip), afmt, _route_on(hip, ro), d["wq"].to(hip), d["ws"].to(hip),
                                  wfmt, rw, otype, ro["T"], ro["k"])
        assert rc == 0 and guards
        y = raw[:ro["nvalid"]].contiguous().view(otype)
        ref, tol, ok = M.random_gate(d, odtype)
        assert float(ok.double().mean()) >= 0.5, "too few comparable outputs"
        err = (y.double() - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)[ok]
        print(f"random mode {mode} {C.PAIR_IDS[C.PAIRS.index(pair)]} {odtype}: worst |y - ref| / bound = {float(ratio.max()):.4f} "
              f"over {int(ok.sum())} outputs")
        assert bool(torch.isfinite(y[ok].float()).all()) and float(ratio.max()) <= 1.0, f"worst ratio {float(ratio.max())}"


# ---- one expert that holds every row: the linears' own kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("rows", [5, 16, 70])
def test_one_expert_equals_the_linear_kernels(hip, pair, rows):
    from neural_compressor_amd import ops

    afmt, wfmt = pair
    c = C.GCase("moe_one_expert", rows, 260, 128 * (M.WAVES + 1), False)
    g = torch.Generator().manual_seed(91 + rows)
    x = torch.randint(-3, 4, (rows, c.Kp), generator=g)
    w = torch.randint(-3, 4, (c.N, c.Kp), generator=g)
    fx, fw = C.SCALE_RULES["block"]
    b = torch.arange(c.Kp // 32)[None, :]
    xs = fx(torch.arange(rows)[:, None], b).to(torch.uint8).to(hip)
    ws = fw(torch.arange(c.N)[:, None], b).to(torch.uint8).to(hip)
    xq = C.stored(C.encode_values(x, afmt), afmt).to(hip)
    wq = C.stored(C.encode_values(w, wfmt), wfmt).to(hip)
    ro = S.route_oracle(torch.zeros(rows, 1, dtype=torch.int64), 1)         # T = rows, k = 1, E = 1: position p is token p
    assert ro["order"].tolist() == list(range(rows))
    y = ops.mx_moe_gemm(2, xq, xs, afmt, _route_on(hip, ro), wq[None], ws[None], wfmt, rows, 1).cpu()
    for dtype in DTYPES16:                                                   # exact operands: the 16-bit outputs hold the fp32 sums
        want = [ops.mx_gemm(xq, xs, afmt, wq, ws, wfmt, None, dtype).cpu()]
        if rows <= ops.MX_GEMV_MAX_M:
            want.append(ops.mx_gemv(xq, xs, afmt, wq, ws, wfmt, None, dtype).cpu())
        for t in want:
            assert torch.equal(y.to(dtype).view(torch.int16), t.view(torch.int16))
    xd = M._scaled(x, xs.cpu())
    wd = M._scaled(w, ws.cpu())
    assert torch.equal(y.double(), xd @ wd.T)


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(hip):
    d = M.exact_case(M.case("one_slot"), 2, "block")
    ro = d["ro"]
    aq, as_, wq, ws = (t.to(hip) for t in M.stored_operands(d, C.FP8, C.FP8))
    aq4, _, wq4, _ = (t.to(hip) for t in M.stored_operands(d, C.FP4, C.FP4))
    route = _route_on(hip, ro)
    rw = d["rw"].float().to(hip)
    T, k = ro["T"], ro["k"]
    BAD, UNSUPPORTED = -1, -2

    def rc_of(mode=2, aq=aq, as_=as_, afmt=C.FP8, wq=wq, ws=ws, wfmt=C.FP8, rw=None, odtype=torch.float32, T=T, k=k):
        rc, raw, guards = _launch(hip, mode, aq, as_, afmt, route, wq, ws, wfmt, rw, odtype, T, k)
        assert guards and bool((raw == (SENT16 if mode == 0 else SENT32)).all()), "a rejected call wrote"
        return rc

    assert rc_of(afmt=C.FP4, aq=aq4) == UNSUPPORTED                          # (fp4, fp8) is not a pair
    assert rc_of(afmt=2) == UNSUPPORTED and rc_of(wfmt=3) == UNSUPPORTED     # fp6 / e5m2 codes
    assert rc_of(ws=ws[:, :, :6].contiguous()) == UNSUPPORTED                # Kp = 192
    assert rc_of(mode=0, wq=wq[:, :19].contiguous(), ws=ws[:, :19].contiguous(), odtype=torch.bfloat16) == UNSUPPORTED      # odd N
    assert rc_of(mode=0, odtype=torch.float32) == UNSUPPORTED and rc_of(odtype=torch.float16) == UNSUPPORTED
    assert rc_of(mode=1, rw=rw, odtype=torch.bfloat16) == UNSUPPORTED
    big = torch.zeros((513, 1, 256), dtype=torch.uint8, device=hip)
    assert rc_of(wq=big, ws=big[:, :, :8].contiguous()) == UNSUPPORTED       # E = 513
    assert rc_of(mode=1) == BAD                                              # mode 1 without routing weights
    assert rc_of(mode=3) == BAD and rc_of(T=0) == BAD and rc_of(k=0) == BAD


# ---- module --------------------------------------------------------------------------------------------------------------------------
def _float_experts(E, H, I, dtype, seed, act=None):
    class Experts(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.gate_up_proj = torch.nn.Parameter((torch.randn(E, 2 * I, H, generator=g) * 0.08).to(dtype))
            self.down_proj = torch.nn.Parameter((torch.randn(E, H, I, generator=g) * 0.08).to(dtype))
            self.act_fn = act if act is not None else torch.nn.SiLU()

    return Experts()


def _mx_experts(hip, pair, E=6, H=200, I=72, dtype=torch.bfloat16, seed=3):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts

    afmt, wfmt = pair
    fl = _float_experts(E, H, I, dtype, seed)
    return fl, MXExperts.from_float(fl, w_dtype=C.FMT_NAMES[wfmt], act_dtype=C.FMT_NAMES[afmt], device=hip)


def _inputs(hip, T, k, E, H, dtype, seed=0, invalid=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, H, generator=g) * 1.5).to(dtype)
    logits = torch.randn(T, E, generator=g)
    w, idx = torch.topk(torch.softmax(logits, -1), k, dim=-1)
    if invalid and T > 2:
        idx[1, 0], idx[2, k - 1] = -1, E                                     # "no expert" sentinels: contribute nothing
    return x.to(hip), idx.to(hip), w.to(hip)


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_from_float_and_recover_against_the_oracle_quantiser(hip, pair):
    afmt, wfmt = pair
    fl, m = _mx_experts(hip, pair)
    E = m.num_experts
    assert m.gate_up_qweight.dtype is torch.uint8 and tuple(m.gate_up_w_scale.shape) == (E, 144, 256 // 32)
    assert tuple(m.down_qweight.shape) == (E, 200, 128 if wfmt == C.FP8 else 64)
    for e in range(E):
        rec = m.recover(torch.float32, expert=e)
        for i, (prefix, p) in enumerate((("gate_up", fl.gate_up_proj), ("down", fl.down_proj))):
            q, s = C.quant_mx(p[e].detach(), wfmt)
            assert torch.equal(getattr(m, prefix + "_qweight")[e].cpu(), C.stored(q, wfmt)), (prefix, e)
            assert torch.equal(getattr(m, prefix + "_w_scale")[e].cpu(), s), (prefix, e)
            assert torch.equal(rec[i].cpu().double(), C.dequant_mx(q, s, wfmt)[:, :p.shape[2]]), (prefix, e)
    gu, dn = m.recover()
    assert gu.dtype is torch.bfloat16 and tuple(gu.shape) == (E, 144, 200) and tuple(dn.shape) == (E, 200, 72)
    assert torch.equal(gu[2].float(), m.recover(torch.float32, expert=2)[0].bfloat16().float())
    assert "w_dtype=" + C.FMT_NAMES[wfmt] in m.extra_repr() and "num_experts=6" in m.extra_repr()


def _six_calls(m, x, idx, w, cdt):
    from neural_compressor_amd import ops

    T, k = idx.shape
    route = ops.moe_route(idx, m.num_experts)
    xq, xs = ops.mx_quant(x, m.act_fmt, m.kp_h)
    h = ops.mx_moe_gemm(0, xq, xs, m.act_fmt, route, m.gate_up_qweight, m.gate_up_w_scale, m.w_fmt, T, k, out_dtype=cdt)
    hq, hs = ops.mx_quant(h, m.act_fmt, m.kp_i)
    y = ops.mx_moe_gemm(1, hq, hs, m.act_fmt, route, m.down_qweight, m.down_w_scale, m.w_fmt, T, k, routing_weights=w)
    return ops.moe_combine(y, route, T, k, m.num_experts, cdt), h, route


@pytest.mark.parametrize("xdtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_fused_forward_is_the_chain_of_the_six_calls(hip, pair, xdtype, monkeypatch):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts

    monkeypatch.setattr(MXExperts, "MOE_FUSED", True)
    monkeypatch.setattr(MXExperts, "MOE_MAX_ROWS", 64)
    ft = torch.float16 if xdtype is torch.float32 else xdtype
    _, m = _mx_experts(hip, pair, dtype=ft)
    for T, k in ((1, 2), (37, 2), (5, 1)):
        x, idx, w = _inputs(hip, T, k, m.num_experts, 200, xdtype, seed=T)

        def no_host_read(self, *a, **kw):
            raise AssertionError("host read in a fused forward")

        with monkeypatch.context() as mp:
            for name in ("item", "tolist", "cpu", "nonzero"):
                mp.setattr(torch.Tensor, name, no_host_read)
            y = m(x, idx, w)
        want, _, _ = _six_calls(m, x, idx, w, ft)
        assert y.dtype is xdtype and y.shape == x.shape
        assert torch.equal(y, want.to(xdtype)) and bool(torch.isfinite(y).all()), (T, k)
    assert tuple(m(x[:0], idx[:0], w[:0]).shape) == (0, 200)
    z = m(x, idx[:, :0], w[:, :0])
    assert z.shape == x.shape and not bool(z.any())


def _emulate_second_half(m, h, route_cpu, ro, w, cdt):
    """float64: y[p] = w[order[p]] * (dequant(quant(h[p])) . Wd[e]) on the fused route's own h, combined in slot order -> (ref, bound)
    [T, H].  The bound per product is PIPE * sum_k |a_k b_k|, then k fp32 additions and one rounding to cdt.
    PIPE = 2^-8 is half a unit in the last place of a product of two e4m3 elements (8 significant bits), allowed on every term.  The
    bound of an fp32 chain (Kp 2^-23 of the mass, the gate of the random-operand tests at Kp = 640) is NOT used here: the sum inside
    one v_mfma_scale instruction is not an fp32 chain.  With one K-tile (Kp = 128) and rows of h, whose elements span many binades
    inside a block, this kernel, inc_mx_gemv and inc_mx_gemm agree bit for bit and all three sit up to 2^-13.9 of the mass away from
    the float64 product (4.3 x the chain bound of 128 terms): OCP MX leaves the internal precision of the dot product to the
    implementation, and the format of the operands is the only thing a bound can be derived from."""
    T, k, nvalid = ro["T"], ro["k"], ro["nvalid"]
    afmt = m.act_fmt
    hq, hs = C.quant_mx(h[:nvalid].cpu(), afmt, m.kp_i)
    hd = C.dequant_mx(hq, hs, afmt)
    _, dn = m.recover(torch.float32)
    dn = torch.nn.functional.pad(dn.cpu().double(), (0, m.kp_i - m.intermediate_dim))
    y = torch.zeros(nvalid, m.hidden_dim, dtype=torch.float64)
    ty = torch.zeros_like(y)
    order = ro["order"].long()
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo < hi:
            wt = w.reshape(-1).double().cpu()[order[lo:hi]][:, None]
            y[lo:hi] = wt * (hd[lo:hi] @ dn[e].T)
            ty[lo:hi] = wt.abs() * PIPE * (hd[lo:hi].abs() @ dn[e].abs().T)
    pos = ro["pos"].long().view(T, k)
    ref = torch.zeros(T, m.hidden_dim, dtype=torch.float64)
    ea = torch.zeros_like(ref)
    mag = torch.zeros_like(ref)
    for s in range(k):
        p = pos[:, s]
        ok = p < nvalid
        ref[ok] += y[p[ok]]
        ea[ok] += ty[p[ok]]
        mag[ok] += y[p[ok]].abs() + ty[p[ok]]
    ea = ea + k * 2.0 ** -24 * mag
    u_out, tiny = S.out_rounding(cdt)
    return ref, ea + u_out * (ref.abs() + ea) + tiny


def _grid_step(h, fmt, Kp):
    """Per element of h (CPU, [rows, K]): the spacing of the MX grid its quantisation lands on, |scale| 2^(max(e, emin) - mb)."""
    f = C._F[fmt]
    q, sb = C.quant_mx(h, fmt, Kp)
    v = C.dequant_mx(q, torch.full_like(sb, 127), fmt).abs()                 # the element values before the block scale
    e = torch.where(v > 0, C._floor_log2(torch.where(v > 0, v, torch.ones_like(v))), torch.full_like(v, f["emin"], dtype=torch.int32))
    step = torch.ldexp(torch.ones_like(v), e.clamp(min=f["emin"]) - f["mb"])
    scale = torch.ldexp(torch.ones(sb.shape, dtype=torch.float64), sb.int() - 127)
    return (step.view(h.shape[0], Kp // 32, 32) * scale[:, :, None]).view(h.shape[0], Kp)


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_both_routes_against_the_emulation_fed_the_fused_h(hip, pair, monkeypatch):
    """The first half (h) is pinned by the exact and random GEMM tests; here the second half of both routes is checked against a
    float64 emulation that starts from the fused route's own h.

    The fused route is held to the emulation's own bound (PIPE per product term, k fp32 additions, one rounding).
    The dense route forms its own h from g and u ROUNDED to 16 bits, with act_fn and the product rounded again:
        |dh| <= 1.5 (1.1 |g| |u| u_out + 3 u_out |h|)      (|silu'| <= 1.1; three roundings on the product; 1.5 covers second order
                                                            and the fp32 chain difference between the tile kernel and the strip kernel)
    and quantises that h: an element moves by at most |dh| plus one step of the grid it lands on, two steps where the block's scale
    byte changes too:  |dhq| <= |dh| + 2 step.  Then y is rounded to 16 bits, multiplied by the routing weight and rounded, and added
    in 16 bits (k roundings): (k + 2) u_out sum_s |w_s| (|h| . |Wd|) on top."""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts

    cdt = torch.bfloat16
    _, m = _mx_experts(hip, pair, dtype=cdt)
    T, k = 37, 2
    x, idx, w = _inputs(hip, T, k, m.num_experts, 200, cdt, seed=5)
    monkeypatch.setattr(MXExperts, "MOE_FUSED", True)
    fused = m(x, idx, w)
    _, h, route = _six_calls(m, x, idx, w, cdt)
    ro = S.route_oracle(idx.cpu(), m.num_experts)
    S.assert_route(route.cpu(), ro)
    ref, tol = _emulate_second_half(m, h, route.cpu(), ro, w, cdt)
    r, (i, j) = S.worst_ratio(fused.cpu(), ref, tol)
    print(f"fused against the emulation {C.PAIR_IDS[C.PAIRS.index(pair)]}: worst ratio {r:.4f}")
    assert r <= 1.0, (r, i, j)

    monkeypatch.setattr(MXExperts, "MOE_FUSED", False)
    dense = m(x, idx, w)
    assert dense.dtype is cdt and dense.shape == x.shape
    nvalid, order, I = ro["nvalid"], ro["order"].long(), m.intermediate_dim
    u_out, _ = S.out_rounding(cdt)
    xq, xs = ops.mx_quant(x, m.act_fmt, m.kp_h)
    gu = ops.mx_moe_gemm(2, xq, xs, m.act_fmt, route, m.gate_up_qweight, m.gate_up_w_scale, m.w_fmt, T, k)[:nvalid].double().cpu()
    hf = h[:nvalid].double().cpu()
    dh = 1.5 * (1.1 * gu[:, :I].abs() * gu[:, I:].abs() * u_out + 3 * u_out * hf.abs())
    dhq = torch.nn.functional.pad(dh, (0, m.kp_i - I)) + 2 * _grid_step(h[:nvalid].cpu(), m.act_fmt, m.kp_i)
    habs = torch.nn.functional.pad(hf.abs(), (0, m.kp_i - I))
    _, dn = m.recover(torch.float32)
    dn = torch.nn.functional.pad(dn.cpu().double().abs(), (0, m.kp_i - I))
    extra = torch.zeros(nvalid, m.hidden_dim, dtype=torch.float64)
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo < hi:
            wt = w.reshape(-1).double().cpu()[order[lo:hi]][:, None].abs()
            extra[lo:hi] = wt * (dhq[lo:hi] @ dn[e].T + (k + 2) * u_out * (habs[lo:hi] @ dn[e].T))
    tol_dense = tol.clone()
    pos = ro["pos"].long().view(T, k)
    for s in range(k):
        p = pos[:, s]
        ok = p < nvalid
        tol_dense[ok] += extra[p[ok]]
    r, (i, j) = S.worst_ratio(dense.cpu(), ref, tol_dense)
    print(f"dense against the emulation {C.PAIR_IDS[C.PAIRS.index(pair)]}: worst ratio {r:.4f}")
    assert r <= 1.0, (r, i, j)


def test_rows_above_the_threshold_take_the_dense_route(hip, monkeypatch):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts

    _, m = _mx_experts(hip, C.PAIRS[0], E=2, H=128, I=64)
    monkeypatch.setattr(MXExperts, "MOE_FUSED", True)
    monkeypatch.setattr(MXExperts, "MOE_MAX_ROWS", 4)
    calls = []
    real = ops.mx_moe_gemm
    monkeypatch.setattr(ops, "mx_moe_gemm", lambda *a, **kw: (calls.append(a[0]), real(*a, **kw))[1])
    for T, fused in ((4, True), (5, False)):                                 # T * k <= 4 * E = 8
        del calls[:]
        x, idx, w = _inputs(hip, T, 2, 2, 128, torch.bfloat16, seed=T, invalid=False)
        y = m(x, idx, w)
        assert calls == ([0, 1] if fused else []) and bool(torch.isfinite(y).all()), (T, calls)


# ---- model ---------------------------------------------------------------------------------------------------------------------------
MODELS = [moe_models.tiny_mixtral, moe_models.tiny_qwen3_moe]
MODEL_IDS = ["mixtral", "qwen3_moe"]


def _ids(n=2, seq=12):
    return torch.randint(0, 128, (n, seq), generator=torch.Generator().manual_seed(0))


@pytest.mark.parametrize("build", MODELS, ids=MODEL_IDS)
def test_model_with_quant_experts(hip, build, tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts, MXLinear, load
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    float_model = build(dtype=torch.bfloat16)
    names = [n for n, _ in moe_models.experts_of(float_model)]
    linears = [n for n, mod in float_model.named_modules() if isinstance(mod, torch.nn.Linear) and n != "lm_head"]
    q = quantize(build(dtype=torch.bfloat16).to(hip), MXQuantConfig(quant_experts=True))
    assert names and all(isinstance(q.get_submodule(n), MXExperts) for n in names)
    assert all(isinstance(q.get_submodule(n), MXLinear) for n in linears) and isinstance(q.lm_head, torch.nn.Linear)
    ids = _ids().to(hip)
    with torch.no_grad():
        y = q(ids).logits
    assert bool(torch.isfinite(y).all())
    q.save(str(tmp_path))
    back = load(str(tmp_path), build(dtype=torch.bfloat16), device=hip)
    assert all(isinstance(back.get_submodule(n), MXExperts) for n in names)
    assert type(back.get_submodule(names[0]).act_fn) is type(float_model.get_submodule(names[0]).act_fn)
    sa, sb = q.state_dict(), back.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k_], sb[k_]) for k_ in sa)
    with torch.no_grad():
        assert torch.equal(back(ids).logits, y)


@pytest.mark.parametrize("build", MODELS, ids=MODEL_IDS)
def test_model_without_quant_experts_is_as_before(hip, build):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts, MXLinear
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    float_model = build(dtype=torch.bfloat16)
    names = [n for n, _ in moe_models.experts_of(float_model)]
    linears = [n for n, mod in float_model.named_modules() if isinstance(mod, torch.nn.Linear) and n != "lm_head"]
    want_keys = []
    for key in float_model.state_dict():
        owner = key.rsplit(".", 1)[0]
        want_keys += [owner + ".qweight", owner + ".w_scale"] if owner in linears and key.endswith(".weight") else [key]
    for cfg in (MXQuantConfig(), MXQuantConfig(quant_experts=False)):
        q = quantize(build(dtype=torch.bfloat16).to(hip), cfg)
        assert not any(isinstance(mod, MXExperts) for mod in q.modules())
        assert all(type(q.get_submodule(n)) is type(float_model.get_submodule(n)) for n in names)
        assert all(isinstance(q.get_submodule(n), MXLinear) for n in linears)
        assert sorted(q.state_dict()) == sorted(want_keys)


def test_set_local_leaves_one_experts_module_float(hip):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    model = moe_models.tiny_mixtral(dtype=torch.bfloat16)
    names = [n for n, _ in moe_models.experts_of(model)]
    cfg = MXQuantConfig(w_dtype="fp4", act_dtype="fp8_e4m3", quant_experts=True)
    cfg.set_local(names[0], MXQuantConfig(w_dtype="fp32"))
    q = quantize(model.to(hip), cfg)
    assert not isinstance(q.get_submodule(names[0]), MXExperts)
    assert isinstance(q.get_submodule(names[1]), MXExperts) and q.get_submodule(names[1]).w_dtype == "fp4"
    with torch.no_grad():
        assert bool(torch.isfinite(q(_ids().to(hip)).logits).all())


def test_unsupported_experts_stay_float(hip):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts, MXQuantizer
    from neural_compressor_amd.torch.utils.utility import is_fused_experts

    model = torch.nn.Module()
    model.gelu = _float_experts(2, 128, 64, torch.bfloat16, 1, act=torch.nn.GELU())
    model.silu = _float_experts(2, 128, 64, torch.bfloat16, 2)
    model.oss = moe_models.tiny_gpt_oss_experts()
    assert not is_fused_experts(model.oss)
    cfg = {"w_dtype": "fp8_e4m3", "act_dtype": "fp8_e4m3"}
    out = MXQuantizer(quant_config={"gelu": cfg, "silu": cfg, "oss": cfg}).convert(model)
    assert isinstance(out.silu, MXExperts) and not isinstance(out.gelu, MXExperts) and type(out.oss).__name__ == "GptOssExperts"
