"""-m gpu: the routed FP8 GEMM of the fused MoE experts (inc_fp8_moe_gemm) and FP8Experts against the oracle of tests/fp8_moe_cases.py.

  exact       every (case, mode) of the table: modes 2 / 1 bit-equal to the float64 result for fp32 / bf16 / fp16 routing weights, mode 0
              within the rounding of the output plus a few fp32 ulp in bf16 and fp16.  `out` sits in a sentinel window, rows past the
              valid positions and the guards stay untouched, source rows no valid position names hold code 0xFF and an a_scale of NaN,
              repeated calls are bit-identical, and the route buffer comes from the oracle, not the route kernel;
  unit scales all three modes bit-identical to inc_mx_moe_gemm (fp8, fp8) with every scale byte 127: the operand map and the K order;
  one expert  mode 2 on one expert that holds every row, rounded to 16 bits == inc_fp8_gemv (<= 16 rows) / inc_fp8_gemm (70 rows);
  gaussian    random codes, non-power-of-two factors: within 2^-8 of the mass per term plus three fp32 roundings (worst ratio printed);
  rejections  each return code, with nothing written;
  module      from_float / recover against the oracle quantiser; the fused forward == the chain of the six ops calls bit for bit; both
              routes against a float64 emulation fed the fused route's own h; the threshold between the routes;
  model       tiny_mixtral / tiny_qwen3_moe / tiny_olmoe under FP8Config(moe_experts=True): every experts module becomes FP8Experts,
              save -> load bit-identical, the error against the float logits printed next to the CPU emulation's; without the flag the
              conversion is what it was.
"""

import logging

import pytest
import torch

from tests import fp8_cases as F
from tests import fp8_moe_cases as M
from tests import moe_models
from tests import moe_stage_cases as S

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x7B5A, 0x7B5A7B5A
GUARD = 16                      # elements in front of the window (keeps it 16-byte aligned) and behind it
DTYPES16 = [torch.bfloat16, torch.float16]
PIPE = M.PIPE


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float32: _lib.INC_F32, torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


def _route_on(hip, ro):
    return S.route_buffer(ro, fill=-1).to(hip)


def _launch(hip, mode, aq, rs, route, wq, al, rw, odtype, T, k, Kp=None):
    """One call of inc_fp8_moe_gemm with `out` inside sentinels -> (rc, the whole window as raw ints [S, Nout] on the CPU, guards ok)."""
    from neural_compressor_amd import _lib

    E, N = wq.shape[:2]
    Kp = wq.shape[2] if Kp is None else Kp
    Sn, Nout = T * k, (N // 2 if mode == 0 else N)
    idt, sent = (torch.int16, SENT16) if mode == 0 else (torch.int32, SENT32)
    buf = torch.full((GUARD + Sn * Nout + GUARD,), sent, dtype=idt, device=hip)
    win = buf[GUARD:GUARD + Sn * Nout]
    assert win.data_ptr() % 16 == 0
    rc = _lib.lib.inc_fp8_moe_gemm(mode, aq.data_ptr(), rs.data_ptr(), route.data_ptr(), wq.data_ptr(), al.data_ptr(),
                                   None if rw is None else rw.data_ptr(), _code(rw.dtype) if rw is not None else _lib.INC_F32,
                                   win.data_ptr(), _code(odtype), T, k, E, N, Kp, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    guards = bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + Sn * Nout:] == sent).all())
    return rc, win.cpu().view(Sn, Nout), guards


def _run_exact(hip, d, odtype=None, wdtype=torch.float32):
    """The exact case d on the device -> the valid rows of the output (CPU, in its float type), every side condition asserted."""
    mode, ro = d["mode"], d["ro"]
    aq, rs, wq, al = (t.to(hip) for t in M.stored_operands(d, poison=True))
    rw = d["rw"].to(wdtype).to(hip) if mode == 1 else None
    otype = odtype if mode == 0 else torch.float32
    args = (hip, mode, aq, rs, _route_on(hip, ro), wq, al, rw, otype, ro["T"], ro["k"])
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
        return [(None, torch.float32), (None, torch.bfloat16), (None, torch.float16)]
    return [(None, torch.float32)]


# ---- the entry point on exact operands -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_exact_operands(hip, cm):
    c, mode = cm
    d = M.exact_case(c, mode)
    M.assert_exact_condition(d)
    for odtype, wdtype in _variants(mode):
        y = _run_exact(hip, d, odtype, wdtype)
        if c.name == "all_invalid":
            assert y.numel() == 0
        why = M.check_output(d, y, odtype)
        assert why is None, f"{c.name} mode {mode} {odtype} {wdtype}: {why}"


def test_poisoned_rows_do_not_change_valid_outputs(hip):
    """The same call with the unnamed source rows as ordinary data gives the same bits."""
    for name, mode in (("short_waves", 0), ("kW_plus1", 1), ("short_waves", 2)):
        d = M.exact_case(M.case(name), mode)
        assert not bool(d["named"].all())
        ro = d["ro"]
        outs = []
        for poison in (True, False):
            aq, rs, wq, al = (t.to(hip) for t in M.stored_operands(d, poison=poison))
            assert bool(torch.isnan(rs).any()) == poison
            rw = d["rw"].float().to(hip) if mode == 1 else None
            rc, raw, _ = _launch(hip, mode, aq, rs, _route_on(hip, ro), wq, al, rw, torch.bfloat16 if mode == 0 else torch.float32,
                                 ro["T"], ro["k"])
            assert rc == 0
            outs.append(raw)
        assert torch.equal(*outs), (name, mode)


# ---- unit factors: the accumulator of inc_mx_moe_gemm --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_unit_scales_equal_the_mx_kernel(hip, mode):
    """a_scale = alpha = 1 against inc_mx_moe_gemm (fp8, fp8) with every scale byte 127, on random codes: the same bits in all three
    modes.  In mode 0 the codes are the magnitudes below 1.0, so that silu(g) u stays inside fp16 (asserted on the float64 result)."""
    from neural_compressor_amd import ops

    d = M.random_case(mode, "edges3", 260, 640, small=(mode == 0), unit=True)
    ro = d["ro"]
    T, k, nv = ro["T"], ro["k"], ro["nvalid"]
    assert nv > 0
    aq, rs, wq, al = d["aq"].to(hip), d["rs"].to(hip), d["wq"].to(hip), d["al"].to(hip)
    as_ = torch.full((aq.shape[0], d["Kp"] // 32), 127, dtype=torch.uint8, device=hip)
    ws = torch.full((*wq.shape[:2], d["Kp"] // 32), 127, dtype=torch.uint8, device=hip)
    route = _route_on(hip, ro)
    rw = d["rw"].to(hip) if mode == 1 else None
    for odtype in (DTYPES16 if mode == 0 else [None]):
        if mode == 0:
            I = d["N"] // 2
            ref = S.silu64(d["val"][:, :I]) * d["val"][:, I:]
            assert float((ref.abs() < float(torch.finfo(odtype).max) / 2).double().mean()) >= M.MIN_SHARE
        got = ops.fp8_moe_gemm(mode, aq, rs, route, wq, al, T, k, routing_weights=rw, out_dtype=odtype)[:nv].cpu()
        want = ops.mx_moe_gemm(mode, aq, as_, F.FP8, route, wq, ws, F.FP8, T, k, routing_weights=rw, out_dtype=odtype)[:nv].cpu()
        idt = torch.int16 if mode == 0 else torch.int32
        assert bool(torch.isfinite(got.float()).all())
        assert torch.equal(got.view(idt), want.view(idt)), (mode, odtype)


# ---- one expert that holds every row: the linears' own kernels ---------------------------------------------------------------------
def _one_expert_route(hip, rows):
    ro = S.route_oracle(torch.zeros(rows, 1, dtype=torch.int64), 1)         # T = rows, k = 1, E = 1: position p is token p
    assert ro["order"].tolist() == list(range(rows))
    return _route_on(hip, ro)


@pytest.mark.parametrize("rows", [5, 16, 70])
def test_one_expert_equals_the_linear_kernels(hip, rows):
    """Exact operands: mode 2 rounded to the 16-bit type is inc_fp8_gemv's / inc_fp8_gemm's output without bias, as numbers (the linear
    kernels add a zero bias, so a zero's sign may differ)."""
    from neural_compressor_amd import ops

    ex = F.exact_case(rows, 260, 128 * (M.WAVES + 1))
    xq, wq, rs, al = ex["xq"].to(hip), ex["wq"].to(hip), ex["rs"].to(hip), ex["al"].to(hip)
    y = ops.fp8_moe_gemm(2, xq, rs, _one_expert_route(hip, rows), wq[None], al[None], rows, 1).cpu()
    assert torch.equal(y.double(), ex["y"])
    for dtype in DTYPES16:
        product = ops.fp8_gemv if rows <= ops.FP8_GEMV_MAX_M else ops.fp8_gemm
        assert torch.equal(y.to(dtype), product(xq, rs, wq, al, None, dtype).cpu()), (rows, dtype)


@pytest.mark.parametrize("rows", [5, 16])
def test_one_expert_equals_the_gemv_on_random_codes(hip, rows):
    """The same split over 8 waves and the same wave order: inc_fp8_gemv's sums bit for bit, on codes whose sums are not exact."""
    from neural_compressor_amd import ops

    N, Kp = 260, 128 * 26
    rc = F.random_codes(rows, N, Kp, 8100 + rows)
    rs, al, _ = F.gaussian_factors(rows, N, 8200 + rows)
    xq, wq, rs, al = rc["xq"].to(hip), rc["wq"].to(hip), rs.to(hip), al.to(hip)
    y = ops.fp8_moe_gemm(2, xq, rs, _one_expert_route(hip, rows), wq[None], al[None], rows, 1).cpu()
    for dtype in DTYPES16:
        want = ops.fp8_gemv(xq, rs, wq, al, None, dtype).cpu()
        assert bool(torch.isfinite(want.float()).all()) and torch.equal(y.to(dtype), want), (rows, dtype)


# ---- Gaussian factors on random codes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_gaussian_factors_on_random_codes(hip, mode):
    d = M.random_case(mode)
    ro = d["ro"]
    rw = d["rw"].to(hip) if mode == 1 else None
    for odtype in (DTYPES16 if mode == 0 else [None]):
        otype = odtype if mode == 0 else torch.float32
        rc, raw, guards = _launch(hip, mode, d["aq"].to(hip), d["rs"].to(hip), _route_on(hip, ro), d["wq"].to(hip), d["al"].to(hip), rw,
                                  otype, ro["T"], ro["k"])
        assert rc == 0 and guards
        y = raw[:ro["nvalid"]].contiguous().view(otype)
        ref, tol, ok = M.random_gate(d, odtype)
        assert float(ok.double().mean()) >= 0.5, "too few comparable outputs"
        err = (y.double() - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)[ok]
        print(f"gaussian factors mode {mode} {odtype}: worst |y - ref| / bound = {float(ratio.max()):.4f} over {int(ok.sum())} outputs")
        assert bool(torch.isfinite(y[ok].float()).all()) and float(ratio.max()) <= 1.0, f"worst ratio {float(ratio.max())}"


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(hip):
    d = M.exact_case(M.case("one_slot"), 2)
    ro = d["ro"]
    aq, rs, wq, al = (t.to(hip) for t in M.stored_operands(d))
    route = _route_on(hip, ro)
    rw = d["rw"].float().to(hip)
    T, k = ro["T"], ro["k"]
    BAD, UNSUPPORTED = -1, -2

    def rc_of(mode=2, aq=aq, rs=rs, wq=wq, al=al, rw=None, odtype=torch.float32, T=T, k=k, Kp=None):
        rc, raw, guards = _launch(hip, mode, aq, rs, route, wq, al, rw, odtype, T, k, Kp)
        assert guards and bool((raw == (SENT16 if mode == 0 else SENT32)).all()), "a rejected call wrote"
        return rc

    assert rc_of(Kp=192) == UNSUPPORTED
    assert rc_of(mode=0, wq=wq[:, :19].contiguous(), al=al[:, :19].contiguous(), odtype=torch.bfloat16) == UNSUPPORTED      # odd N
    assert rc_of(mode=0, odtype=torch.float32) == UNSUPPORTED and rc_of(odtype=torch.float16) == UNSUPPORTED
    assert rc_of(mode=1, rw=rw, odtype=torch.bfloat16) == UNSUPPORTED
    big = torch.zeros((513, 1, 256), dtype=torch.uint8, device=hip)
    assert rc_of(wq=big, al=torch.ones((513, 1), device=hip)) == UNSUPPORTED  # E = 513
    assert rc_of(mode=1) == BAD                                              # mode 1 without routing weights
    assert rc_of(mode=3) == BAD and rc_of(T=0) == BAD and rc_of(k=0) == BAD
    assert rc_of(aq=aq.view(-1)[8:8 + 128].view(1, 128)) == BAD               # codes not 16-byte aligned
    assert rc_of(al=al.view(torch.uint8).view(-1)[2:-2].view(-1)) == BAD      # factors not 4-byte aligned


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


def _fp8_experts(hip, E=6, H=200, I=72, dtype=torch.bfloat16, seed=3):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts

    fl = _float_experts(E, H, I, dtype, seed)
    return fl, FP8Experts.from_float(fl, device=hip)


def _inputs(hip, T, k, E, H, dtype, seed=0, invalid=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, H, generator=g) * 1.5).to(dtype)
    logits = torch.randn(T, E, generator=g)
    w, idx = torch.topk(torch.softmax(logits, -1), k, dim=-1)
    if invalid and T > 2:
        idx[1, 0], idx[2, k - 1] = -1, E                                     # "no expert" sentinels: contribute nothing
    return x.to(hip), idx.to(hip), w.to(hip)


def test_from_float_and_recover_against_the_oracle_quantiser(hip):
    fl, m = _fp8_experts(hip)
    E = m.num_experts
    assert m.gate_up_qweight.dtype is torch.uint8 and tuple(m.gate_up_qweight.shape) == (E, 144, 256)
    assert m.gate_up_w_scale.dtype is torch.float32 and tuple(m.gate_up_w_scale.shape) == (E, 144)
    assert tuple(m.down_qweight.shape) == (E, 200, 128) and tuple(m.down_w_scale.shape) == (E, 200)
    for e in range(E):
        rec = m.recover(torch.float32, expert=e)
        for i, (prefix, p) in enumerate((("gate_up", fl.gate_up_proj), ("down", fl.down_proj))):
            q, s = F.quant_rows(p[e].detach())
            assert torch.equal(getattr(m, prefix + "_qweight")[e].cpu(), q), (prefix, e)
            assert torch.equal(getattr(m, prefix + "_w_scale")[e].cpu(), s), (prefix, e)
            want = (F.code_table(F.FP8).float()[q.long()] * s[:, None])[:, :p.shape[2]]          # one fp32 multiply per element
            assert torch.equal(rec[i].cpu(), want), (prefix, e)
    gu, dn = m.recover()
    assert gu.dtype is torch.bfloat16 and tuple(gu.shape) == (E, 144, 200) and tuple(dn.shape) == (E, 200, 72)
    assert torch.equal(gu[2].float(), m.recover(torch.float32, expert=2)[0].bfloat16().float())
    assert "fp8_config=E4M3" in m.extra_repr() and "num_experts=6" in m.extra_repr()


def _six_calls(m, x, idx, w, cdt):
    from neural_compressor_amd import ops

    T, k = idx.shape
    route = ops.moe_route(idx, m.num_experts)
    xq, xs = ops.fp8_quant_rows(x, None, m.kp_h)
    h = ops.fp8_moe_gemm(0, xq, xs, route, m.gate_up_qweight, m.gate_up_w_scale, T, k, out_dtype=cdt)
    hq, hs = ops.fp8_quant_rows(h, None, m.kp_i)
    y = ops.fp8_moe_gemm(1, hq, hs, route, m.down_qweight, m.down_w_scale, T, k, routing_weights=w)
    return ops.moe_combine(y, route, T, k, m.num_experts, cdt), h, route


@pytest.mark.parametrize("xdtype", F.DTYPES, ids=F.DTYPE_IDS)
def test_fused_forward_is_the_chain_of_the_six_calls(hip, xdtype, monkeypatch):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts

    monkeypatch.setattr(FP8Experts, "MOE_FUSED", True)
    monkeypatch.setattr(FP8Experts, "MOE_MAX_ROWS", 64)
    ft = torch.float16 if xdtype is torch.float32 else xdtype
    _, m = _fp8_experts(hip, dtype=ft)
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


def _emulate_second_half(m, h, ro, w, cdt):
    """float64: y[p] = w[order[p]] * (dequant(quant(h[p])) . Wd[e]) on the fused route's own h, combined in slot order -> (ref, bound)
    [T, H].  The bound per product is PIPE * sum_k |a_k b_k| (both factors inside the mass) plus three fp32 roundings, then k fp32
    additions and one rounding to cdt: the per-slot allowance of fp8_moe_cases.random_gate, summed by the combine."""
    T, k, nvalid = ro["T"], ro["k"], ro["nvalid"]
    hd = F.dequant(*F.quant_rows(h[:nvalid].cpu(), None, m.kp_i))
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
            ty[lo:hi] = wt.abs() * PIPE * (hd[lo:hi].abs() @ dn[e].abs().T) + 3 * 2.0 ** -24 * y[lo:hi].abs()
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


def test_both_routes_against_the_emulation_fed_the_fused_h(hip, monkeypatch):
    """The first half (h) is pinned by the exact and random GEMM tests; here the second half of both routes is checked against a
    float64 emulation that starts from the fused route's own h.

    The fused route is held to the emulation's own bound (PIPE per product term, three fp32 roundings, k fp32 additions, one rounding
    to the output type, i.e. one output ulp).
    The dense route forms its own h from g and u ROUNDED to 16 bits, with act_fn and the product rounded again:
        |dh| <= 1.5 (1.1 |g| |u| u_out + 3 u_out |h|)      (|silu'| <= 1.1; three roundings on the product; 1.5 covers second order
                                                            and the difference between the tile kernel's and the strip kernel's sums)
    and quantises that h with its own row scale.  A quantised element is within half a grid step of its input, and the e4m3 grid has
    3 mantissa bits: half a step is at most 2^-4 of the element, or s 2^-10 in the subnormals (s the row's scale), for the dense h and
    the fused h alike:  |dhq| <= |dh| + 2^-3 (|h| + |dh|) + 2^-9 s', s' = (max |h| + max |dh|) / 448.  The dense product carries PIPE
    on its own mass; then y is rounded to 16 bits, multiplied by the routing weight and rounded, and added in 16 bits (k roundings):
    (k + 2) u_out sum_s |w_s| (|h| . |Wd|) on top."""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts

    cdt = torch.bfloat16
    _, m = _fp8_experts(hip, dtype=cdt)
    T, k = 37, 2
    x, idx, w = _inputs(hip, T, k, m.num_experts, 200, cdt, seed=5)
    monkeypatch.setattr(FP8Experts, "MOE_FUSED", True)
    fused = m(x, idx, w)
    _, h, route = _six_calls(m, x, idx, w, cdt)
    ro = S.route_oracle(idx.cpu(), m.num_experts)
    S.assert_route(route.cpu(), ro)
    ref, tol = _emulate_second_half(m, h, ro, w, cdt)
    r, (i, j) = S.worst_ratio(fused.cpu(), ref, tol)
    print(f"fused against the emulation: worst ratio {r:.4f}")
    assert r <= 1.0, (r, i, j)

    monkeypatch.setattr(FP8Experts, "MOE_FUSED", False)
    dense = m(x, idx, w)
    assert dense.dtype is cdt and dense.shape == x.shape
    nvalid, order, I = ro["nvalid"], ro["order"].long(), m.intermediate_dim
    u_out, _ = S.out_rounding(cdt)
    xq, xs = ops.fp8_quant_rows(x, None, m.kp_h)
    gu = ops.fp8_moe_gemm(2, xq, xs, route, m.gate_up_qweight, m.gate_up_w_scale, T, k)[:nvalid].double().cpu()
    hf = h[:nvalid].double().cpu()
    dh = 1.5 * (1.1 * gu[:, :I].abs() * gu[:, I:].abs() * u_out + 3 * u_out * hf.abs())
    s_up = (hf.abs().amax(dim=1, keepdim=True) + dh.amax(dim=1, keepdim=True)) / 448.0
    dhq = torch.nn.functional.pad(dh + 2.0 ** -3 * (hf.abs() + dh) + 2.0 ** -9 * s_up, (0, m.kp_i - I))
    habs = torch.nn.functional.pad(hf.abs(), (0, m.kp_i - I))
    _, dn = m.recover(torch.float32)
    dn = torch.nn.functional.pad(dn.cpu().double().abs(), (0, m.kp_i - I))
    extra = torch.zeros(nvalid, m.hidden_dim, dtype=torch.float64)
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo < hi:
            wt = w.reshape(-1).double().cpu()[order[lo:hi]][:, None].abs()
            extra[lo:hi] = wt * ((1 + PIPE) * (dhq[lo:hi] @ dn[e].T) + (k + 2) * u_out * ((habs[lo:hi] + dhq[lo:hi]) @ dn[e].T))
    tol_dense = tol.clone()
    pos = ro["pos"].long().view(T, k)
    for s in range(k):
        p = pos[:, s]
        ok = p < nvalid
        tol_dense[ok] += extra[p[ok]]
    r, (i, j) = S.worst_ratio(dense.cpu(), ref, tol_dense)
    print(f"dense against the emulation: worst ratio {r:.4f}")
    assert r <= 1.0, (r, i, j)


def test_rows_above_the_threshold_take_the_dense_route(hip, monkeypatch):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts

    _, m = _fp8_experts(hip, E=2, H=128, I=64)
    monkeypatch.setattr(FP8Experts, "MOE_FUSED", True)
    monkeypatch.setattr(FP8Experts, "MOE_MAX_ROWS", 4)
    calls = []
    real = ops.fp8_moe_gemm
    monkeypatch.setattr(ops, "fp8_moe_gemm", lambda *a, **kw: (calls.append(a[0]), real(*a, **kw))[1])
    for T, fused in ((4, True), (5, False)):                                 # T * k <= 4 * E = 8
        del calls[:]
        x, idx, w = _inputs(hip, T, 2, 2, 128, torch.bfloat16, seed=T, invalid=False)
        y = m(x, idx, w)
        assert calls == ([0, 1] if fused else []) and bool(torch.isfinite(y).all()), (T, calls)
    monkeypatch.setattr(FP8Experts, "MOE_FUSED", False)
    del calls[:]
    x, idx, w = _inputs(hip, 4, 2, 2, 128, torch.bfloat16, seed=4, invalid=False)
    m(x, idx, w)
    assert calls == []


# ---- model ---------------------------------------------------------------------------------------------------------------------------
MODELS = [moe_models.tiny_mixtral, moe_models.tiny_qwen3_moe, moe_models.tiny_olmoe]
MODEL_IDS = ["mixtral", "qwen3_moe", "olmoe"]


def _ids(n=2, seq=12):
    return torch.randint(0, 128, (n, seq), generator=torch.Generator().manual_seed(0))


def _rel(y, ref):
    return float((y.float() - ref.float()).norm() / ref.float().norm())


@pytest.mark.parametrize("build", MODELS, ids=MODEL_IDS)
def test_model_with_moe_experts(hip, build, tmp_path):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts, FP8Linear, load
    from neural_compressor_amd.torch.quantization import FP8Config, quantize
    from neural_compressor_amd.torch.utils.utility import set_module

    float_model = build(dtype=torch.bfloat16).to(hip)
    names = [n for n, _ in moe_models.experts_of(float_model)]
    linears = [n for n, mod in float_model.named_modules() if isinstance(mod, torch.nn.Linear) and n != "lm_head"]
    q = quantize(build(dtype=torch.bfloat16).to(hip), FP8Config(moe_experts=True))
    assert names and all(isinstance(q.get_submodule(n), FP8Experts) for n in names)
    assert all(isinstance(q.get_submodule(n), FP8Linear) for n in linears) and isinstance(q.lm_head, torch.nn.Linear)
    ids = _ids().to(hip)
    with torch.no_grad():
        y = q(ids).logits
        ref = float_model(ids).logits
    assert bool(torch.isfinite(y).all())
    q.save(str(tmp_path))
    back = load(str(tmp_path), build(dtype=torch.bfloat16), device=hip)
    assert all(isinstance(back.get_submodule(n), FP8Experts) for n in names)
    assert type(back.get_submodule(names[0]).act_fn) is type(float_model.get_submodule(names[0]).act_fn)
    sa, sb = q.state_dict(), back.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k_], sb[k_]) for k_ in sa)
    with torch.no_grad():
        assert torch.equal(back(ids).logits, y)
    # records, not thresholds: the error against the float logits, next to the CPU fake-quant emulation's
    emu = build(dtype=torch.bfloat16).to(hip)
    for n in linears:
        set_module(emu, n, F.FakeQuantLinear(emu.get_submodule(n), torch.bfloat16))
    for n in names:
        set_module(emu, n, M.FakeQuantExperts(emu.get_submodule(n)))
    with torch.no_grad():
        ye = emu(ids).logits
    print(f"{build.__name__}: relative error of the logits against float: FP8 model {_rel(y, ref):.4f}, CPU fake-quant emulation "
          f"{_rel(ye, ref):.4f}")


@pytest.mark.parametrize("build", MODELS, ids=MODEL_IDS)
def test_model_without_the_flag_is_as_before(hip, build):
    """The default conversion: the experts keep their type, the Linears convert, the state-dict keys are those of a Linears-only
    conversion, and the logits are those of the same model converted by FP8Linear.from_float module by module (today's conversion)."""
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts, FP8Linear
    from neural_compressor_amd.torch.quantization import FP8Config, quantize
    from neural_compressor_amd.torch.utils.utility import set_module

    float_model = build(dtype=torch.bfloat16)
    names = [n for n, _ in moe_models.experts_of(float_model)]
    linears = [n for n, mod in float_model.named_modules() if isinstance(mod, torch.nn.Linear) and n != "lm_head"]
    want_keys = []
    for key in float_model.state_dict():
        owner = key.rsplit(".", 1)[0]
        want_keys += [owner + ".qweight", owner + ".w_scale"] if owner in linears and key.endswith(".weight") else [key]
    by_hand = build(dtype=torch.bfloat16).to(hip)
    for n in linears:
        set_module(by_hand, n, FP8Linear.from_float(by_hand.get_submodule(n), device=hip))
    ids = _ids().to(hip)
    with torch.no_grad():
        want = by_hand(ids).logits
    for cfg in (FP8Config(), FP8Config(moe_experts=False)):
        q = quantize(build(dtype=torch.bfloat16).to(hip), cfg)
        assert not any(isinstance(mod, FP8Experts) for mod in q.modules())
        assert all(type(q.get_submodule(n)) is type(float_model.get_submodule(n)) for n in names)
        assert all(isinstance(q.get_submodule(n), FP8Linear) for n in linears)
        assert sorted(q.state_dict()) == sorted(want_keys)
        with torch.no_grad():
            assert torch.equal(q(ids).logits, want)


def test_set_local_leaves_one_experts_module_float(hip):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts
    from neural_compressor_amd.torch.quantization import FP8Config, quantize

    model = moe_models.tiny_mixtral(dtype=torch.bfloat16)
    names = [n for n, _ in moe_models.experts_of(model)]
    cfg = FP8Config(moe_experts=True)
    cfg.set_local(names[0], FP8Config(fp8_config="fp32"))
    q = quantize(model.to(hip), cfg)
    assert not isinstance(q.get_submodule(names[0]), FP8Experts) and isinstance(q.get_submodule(names[1]), FP8Experts)
    with torch.no_grad():
        assert bool(torch.isfinite(q(_ids().to(hip)).logits).all())


def test_unsupported_experts_stay_float_with_one_warning(hip, caplog):
    from neural_compressor_amd.common.utils import logger
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts, FP8Quantizer
    from neural_compressor_amd.torch.utils.utility import is_fused_experts

    model = torch.nn.Module()
    model.gelu = _float_experts(2, 128, 64, torch.bfloat16, 1, act=torch.nn.GELU())
    model.silu = _float_experts(2, 128, 64, torch.bfloat16, 2)
    model.oss = moe_models.tiny_gpt_oss_experts()
    assert not is_fused_experts(model.oss)
    cfg = {"fp8_config": "E4M3"}
    messages = []
    handler = logging.Handler()
    handler.emit = lambda record: messages.append(record.getMessage())
    target = logger if isinstance(logger, logging.Logger) else getattr(logger, "_logger", logging.getLogger())
    target.addHandler(handler)
    try:
        out = FP8Quantizer(quant_config={"gelu": cfg, "silu": cfg, "oss": cfg}).convert(model)
    finally:
        target.removeHandler(handler)
    assert isinstance(out.silu, FP8Experts) and not isinstance(out.gelu, FP8Experts) and type(out.oss).__name__ == "GptOssExperts"
    about = [t for t in messages if "stays in floating point" in t]
    assert len(about) == 1 and "gelu" in about[0] and "GELU is not SiLU" in about[0], messages
