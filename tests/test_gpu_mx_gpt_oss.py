"""-m gpu: the routed MX GEMM with the GPT-OSS epilogue (inc_mx_moe_gemm_glu) and MXGptOssExperts against the oracle of
tests/mx_gpt_oss_cases.py.

  exact     mx_moe_cases' table x three pairs x both scale rules with the bias: modes 2 / 1 bit-equal to the float64 result (fp32 and
            bf16 routing weights, fp16 once), mode 0 (bf16 and fp16, three (alpha, limit) sets) inside the gate of the helper's
            docstring.  `out` sits in a sentinel window: rows past the valid positions and the guards stay untouched, unnamed source rows
            are poisoned, repeated calls are bit-identical;
  no bias   bias = NULL in modes 1 / 2 is inc_mx_moe_gemm bit for bit;
  random    Gaussian operands within the chain bound with the bias added;
  module    from_float / from_mxfp4 / recover against the oracle quantiser and transformers' MXFP4 dequantiser; the fused forward is the
            chain of the six ops calls bit for bit with no host read; both routes against a float64 emulation fed the fused route's own
            h; both routes against transformers' GptOssExperts on the recovered weights (a record);
  model     tiny GptOssForCausalLM: every experts module becomes MXGptOssExperts, finite logits, save -> load bit-identical.
"""

import math

import pytest
import torch

from tests import moe_models
from tests import moe_stage_cases as S
from tests import mx_cases as C
from tests import mx_gpt_oss_cases as G
from tests import mx_moe_cases as M

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x7B5A, 0x7B5A7B5A
GUARD = 16
DTYPES16 = [torch.bfloat16, torch.float16]
PIPE = 2.0 ** -8                # per-term allowance of the module-level emulation (test_gpu_mx_moe._emulate_second_half)
ALPHA, LIMIT = 1.702, 7.0


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float32: _lib.INC_F32, torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


def _route_on(hip, ro):
    return S.route_buffer(ro, fill=-1).to(hip)


def _launch(hip, mode, aq, as_, afmt, route, wq, ws, wfmt, bias, alpha, limit, rw, odtype, T, k, plain=False):
    """One call of inc_mx_moe_gemm_glu (plain: inc_mx_moe_gemm) with `out` inside sentinels -> (rc, the whole window as raw ints
    [S, Nout] on the CPU, guards ok)."""
    from neural_compressor_amd import _lib

    E, N = wq.shape[:2]
    Kp = ws.shape[2] * 32
    Sn, Nout = T * k, (N // 2 if mode == 0 else N)
    idt, sent = (torch.int16, SENT16) if mode == 0 else (torch.int32, SENT32)
    buf = torch.full((GUARD + Sn * Nout + GUARD,), sent, dtype=idt, device=hip)
    win = buf[GUARD:GUARD + Sn * Nout]
    assert win.data_ptr() % 16 == 0
    head = (mode, aq.data_ptr(), as_.data_ptr(), afmt, route.data_ptr(), wq.data_ptr(), ws.data_ptr(), wfmt)
    tail = (None if rw is None else rw.data_ptr(), _code(rw.dtype) if rw is not None else _lib.INC_F32, win.data_ptr(), _code(odtype),
            T, k, E, N, Kp, torch.cuda.current_stream().cuda_stream)
    if plain:
        rc = _lib.lib.inc_mx_moe_gemm(*head, *tail)
    else:
        rc = _lib.lib.inc_mx_moe_gemm_glu(*head, None if bias is None else bias.data_ptr(), alpha, limit, *tail)
    torch.cuda.synchronize()
    guards = bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + Sn * Nout:] == sent).all())
    return rc, win.cpu().view(Sn, Nout), guards


def _bias_on(hip, d):
    return G.bias_of(d["ro"]["E"], d["N"]).float().contiguous().to(hip)


_on_device = {}


def _operands(hip, d, pair, poison):
    """The stored operands of d on the device, one entry kept (a test walks its launches case by case)."""
    key = (d["case"].name, d["mode"], d["rule"], pair, poison)
    if key not in _on_device:
        _on_device.clear()
        _on_device[key] = tuple(t.to(hip) for t in M.stored_operands(d, *pair, poison=poison))
    return _on_device[key]


def _run_exact(hip, d, pair, alpha, limit, odtype=None, wdtype=torch.float32, poison=True):
    """The exact case d on the device -> the valid rows of the output (CPU, in its float type), every side condition asserted."""
    afmt, wfmt = pair
    mode, ro = d["mode"], d["ro"]
    aq, as_, wq, ws = _operands(hip, d, pair, poison)
    rw = d["rw"].to(wdtype).to(hip) if mode == 1 else None
    otype = odtype if mode == 0 else torch.float32
    args = (hip, mode, aq, as_, afmt, _route_on(hip, ro), wq, ws, wfmt, _bias_on(hip, d), alpha, limit, rw, otype, ro["T"], ro["k"])
    rc, raw, guards = _launch(*args)
    assert rc == 0, rc
    assert guards, "wrote around out"
    sent = SENT16 if mode == 0 else SENT32
    nv = ro["nvalid"]
    assert bool((raw[nv:] == sent).all()), "wrote a row past the valid positions"
    rc2, raw2, _ = _launch(*args)
    assert rc2 == 0 and torch.equal(raw, raw2), "repeated calls differ"
    return raw[:nv].contiguous().view(otype)


# ---- the entry point on exact operands -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_exact_operands_with_bias(hip, cm, pair):
    c, mode = cm
    for rule in M.RULES:
        d = M.exact_case(c, mode, rule)
        G.assert_exact_condition(d)
        if mode == 0:
            for _, alpha, limit in G.PARAMS:
                for odtype in DTYPES16:
                    y = _run_exact(hip, d, pair, alpha, limit, odtype)
                    why = G.check_output(d, y, alpha, limit, odtype)
                    assert why is None, f"{c.name} mode 0 {rule} alpha {alpha} limit {limit} {odtype}: {why}"
        else:
            for wdtype in ((torch.float32, torch.bfloat16) if mode == 1 else (torch.float32,)):
                y = _run_exact(hip, d, pair, ALPHA, LIMIT, None, wdtype)
                why = G.check_output(d, y, ALPHA, LIMIT)
                assert why is None, f"{c.name} mode {mode} {rule} {wdtype}: {why}"


def test_fp16_routing_weights(hip):
    d = M.exact_case(M.case("kW"), 1, "block")
    y = _run_exact(hip, d, C.PAIRS[0], ALPHA, LIMIT, None, torch.float16)
    assert G.check_output(d, y, ALPHA, LIMIT) is None


def test_poisoned_rows_do_not_change_valid_outputs(hip):
    for name, mode in (("short_waves", 0), ("kW_plus1", 1), ("short_waves", 2)):
        d = M.exact_case(M.case(name), mode, "block")
        assert not bool(d["named"].all())
        outs = [_run_exact(hip, d, C.PAIRS[1], ALPHA, LIMIT, torch.bfloat16, poison=p) for p in (True, False)]
        assert torch.equal(outs[0].view(torch.int16 if mode == 0 else torch.int32),
                           outs[1].view(torch.int16 if mode == 0 else torch.int32)), (name, mode)


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("mode", [2, 1])
def test_null_bias_is_the_plain_entry_point(hip, mode, pair):
    afmt, wfmt = pair
    d = M.random_case(mode, afmt, wfmt)
    ro = d["ro"]
    rw = d["rw"].to(hip) if mode == 1 else None
    args = (hip, mode, d["aq"].to(hip), d["as_"].to(hip), afmt, _route_on(hip, ro), d["wq"].to(hip), d["ws"].to(hip), wfmt)
    rc, raw, guards = _launch(*args, None, ALPHA, LIMIT, rw, torch.float32, ro["T"], ro["k"])
    rc0, raw0, _ = _launch(*args, None, ALPHA, LIMIT, rw, torch.float32, ro["T"], ro["k"], plain=True)
    assert rc == 0 and rc0 == 0 and guards
    assert torch.equal(raw, raw0)


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
                                  wfmt, _bias_on(hip, d), ALPHA, LIMIT, rw, otype, ro["T"], ro["k"])
        assert rc == 0 and guards
        y = raw[:ro["nvalid"]].contiguous().view(otype)
        ref, tol, ok = G.random_gate(d, ALPHA, LIMIT, odtype)
        assert float(ok.double().mean()) >= 0.5, "too few comparable outputs"
        err = (y.double() - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)[ok]
        print(f"random mode {mode} {C.PAIR_IDS[C.PAIRS.index(pair)]} {odtype}: worst |y - ref| / bound = {float(ratio.max()):.4f} "
              f"over {int(ok.sum())} outputs")
        assert bool(torch.isfinite(y[ok].float()).all()) and float(ratio.max()) <= 1.0, f"worst ratio {float(ratio.max())}"


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(hip):
    d = M.exact_case(M.case("one_slot"), 2, "block")
    ro = d["ro"]
    aq, as_, wq, ws = (t.to(hip) for t in M.stored_operands(d, C.FP8, C.FP8))
    route = _route_on(hip, ro)
    bias = _bias_on(hip, d)
    rw = d["rw"].float().to(hip)
    T, k = ro["T"], ro["k"]
    BAD, UNSUPPORTED = -1, -2

    def rc_of(mode=2, afmt=C.FP8, ws=ws, bias=bias, alpha=ALPHA, limit=LIMIT, rw=None, odtype=torch.float32):
        rc, raw, guards = _launch(hip, mode, aq, as_, afmt, route, wq, ws, C.FP8, bias, alpha, limit, rw, odtype, T, k)
        assert guards and bool((raw == (SENT16 if mode == 0 else SENT32)).all()), "a rejected call wrote"
        return rc

    assert rc_of(limit=0.0) == BAD and rc_of(limit=-1.0) == BAD and rc_of(alpha=math.nan) == BAD and rc_of(limit=math.nan) == BAD
    assert rc_of(bias=bias.view(torch.int16).reshape(-1)[1:]) == BAD         # 2-byte aligned
    assert rc_of(mode=1) == BAD and rc_of(mode=3) == BAD
    assert rc_of(afmt=2) == UNSUPPORTED and rc_of(ws=ws[:, :, :6].contiguous()) == UNSUPPORTED
    assert rc_of(mode=0, odtype=torch.float32) == UNSUPPORTED and rc_of(odtype=torch.float16) == UNSUPPORTED
    assert rc_of(mode=1, rw=rw, odtype=torch.bfloat16) == UNSUPPORTED


# ---- module --------------------------------------------------------------------------------------------------------------------------
def _float_experts(E, H, I, dtype, seed):
    """transformers' GptOssExperts of the given sizes with seeded parameters."""
    from transformers import GptOssConfig
    from transformers.models.gpt_oss.modeling_gpt_oss import GptOssExperts

    m = GptOssExperts(GptOssConfig(vocab_size=128, hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=4,
                                   num_key_value_heads=2, num_local_experts=E, num_experts_per_tok=2, head_dim=16))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.gate_up_proj.copy_(torch.randn(E, H, 2 * I, generator=g) * 0.08)
        m.gate_up_proj_bias.copy_(torch.randn(E, 2 * I, generator=g) * 0.5)
        m.down_proj.copy_(torch.randn(E, I, H, generator=g) * 0.08)
        m.down_proj_bias.copy_(torch.randn(E, H, generator=g) * 0.5)
    assert (m.alpha, m.limit) == (ALPHA, LIMIT)
    return m.to(dtype)


def _mx_experts(hip, pair, E=6, H=200, I=72, dtype=torch.bfloat16, seed=3):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts
    from neural_compressor_amd.torch.utils import is_gpt_oss_experts

    afmt, wfmt = pair
    fl = _float_experts(E, H, I, dtype, seed)
    assert is_gpt_oss_experts(fl)
    return fl, MXGptOssExperts.from_float(fl, w_dtype=C.FMT_NAMES[wfmt], act_dtype=C.FMT_NAMES[afmt], device=hip)


def _inputs(hip, T, k, E, H, dtype, seed=0, invalid=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, H, generator=g) * 1.5).to(dtype)
    logits = torch.randn(T, E, generator=g)
    w, idx = torch.topk(torch.softmax(logits, -1), k, dim=-1)
    if invalid and T > 2:
        idx[1, 0], idx[2, k - 1] = -1, E                                     # -1 and the router's mask class E: contribute nothing
    return x.to(hip), idx.to(hip), w.to(hip)


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_from_float_and_recover_against_the_oracle_quantiser(hip, pair):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant.experts import gpt_oss_bias_rows, gpt_oss_rows

    afmt, wfmt = pair
    fl, m = _mx_experts(hip, pair)
    E, H, I = 6, 200, 72
    rows = {"gate_up": gpt_oss_rows(fl.gate_up_proj.detach()).contiguous(), "down": fl.down_proj.detach().transpose(1, 2).contiguous()}
    assert tuple(m.gate_up_w_scale.shape) == (E, 144, 256 // 32) and tuple(m.down_qweight.shape) == (E, 200, 128 if wfmt == C.FP8 else 64)
    assert m.gate_up_bias.dtype is torch.float32 and tuple(m.gate_up_bias.shape) == (E, 144) and tuple(m.down_bias.shape) == (E, 200)
    assert torch.equal(m.gate_up_bias.cpu(), gpt_oss_bias_rows(fl.gate_up_proj_bias.detach().float()))
    assert torch.equal(m.down_bias.cpu(), fl.down_proj_bias.detach().float())
    gu32, dn32 = m.recover(torch.float32)
    assert tuple(gu32.shape) == (E, H, 2 * I) and tuple(dn32.shape) == (E, I, H)
    for prefix, p in rows.items():
        N, K = p.shape[1:]
        codes, scales = ops.mx_quant(p.to(hip).reshape(E * N, K), wfmt, C.padded_k(K))
        assert torch.equal(getattr(m, prefix + "_qweight"), codes.view(E, N, -1)) and torch.equal(getattr(m, prefix + "_w_scale"), scales.view(E, N, -1))
        for e in range(E):
            q, s = C.quant_mx(p[e], wfmt)
            assert torch.equal(getattr(m, prefix + "_qweight")[e].cpu(), C.stored(q, wfmt)), (prefix, e)
            assert torch.equal(getattr(m, prefix + "_w_scale")[e].cpu(), s), (prefix, e)
            deq = C.dequant_mx(q, s, wfmt)[:, :K]                                   # [N, K] in the kernel's row order
            if prefix == "gate_up":
                want = torch.stack([deq[:I], deq[I:]], 1).reshape(2 * I, H).T        # column 2 j = gate j, 2 j + 1 = up j
            else:
                want = deq.T
            got = (gu32 if prefix == "gate_up" else dn32)[e].cpu().double()
            assert torch.equal(got, want), (prefix, e)
            assert torch.equal(m.recover(torch.float32, expert=e)[0 if prefix == "gate_up" else 1].cpu().double(), want)
    gu, dn = m.recover()
    assert gu.dtype is torch.bfloat16 and torch.equal(gu, gu32.bfloat16())
    gb, db = m.recover_biases(torch.float32)
    assert torch.equal(gb.cpu(), fl.gate_up_proj_bias.detach().float()) and torch.equal(db.cpu(), fl.down_proj_bias.detach().float())
    assert "alpha=1.702" in m.extra_repr() and "num_experts=6" in m.extra_repr()


def test_from_mxfp4_is_the_checkpoint(hip):
    from transformers.integrations.mxfp4 import convert_moe_packed_tensors

    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts

    E, H, I = 3, 160, 96                                                      # Kp(H) = 256, Kp(I) = 128: padding blocks in both
    g = torch.Generator().manual_seed(11)
    gub = torch.randint(0, 256, (E, 2 * I, H // 32, 16), generator=g, dtype=torch.uint8)
    gus = torch.randint(118, 130, (E, 2 * I, H // 32), generator=g, dtype=torch.uint8)
    dnb = torch.randint(0, 256, (E, H, I // 32, 16), generator=g, dtype=torch.uint8)
    dns = torch.randint(118, 130, (E, H, I // 32), generator=g, dtype=torch.uint8)
    gb, db = torch.randn(E, 2 * I, generator=g), torch.randn(E, H, generator=g)
    m = MXGptOssExperts.from_mxfp4(gub, gus, gb, dnb, dns, db, device=hip)
    assert m.w_dtype == "fp4" and m.act_dtype == "fp8_e4m3" and (m.hidden_dim, m.intermediate_dim) == (H, I)
    gu, dn = m.recover(torch.float32)
    for got, want in ((gu, convert_moe_packed_tensors(gub, gus, dtype=torch.float32)),
                      (dn, convert_moe_packed_tensors(dnb, dns, dtype=torch.float32))):
        assert got.shape == want.shape
        assert torch.equal(got.cpu().contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    rgb, rdb = m.recover_biases(torch.float32)
    assert torch.equal(rgb.cpu(), gb) and torch.equal(rdb.cpu(), db)
    x, idx, w = _inputs(hip, 9, 2, E, H, torch.bfloat16, seed=2)
    y = m(x, idx, w)
    assert y.shape == x.shape and bool(torch.isfinite(y).all())


def _six_calls(m, x, idx, w, cdt):
    from neural_compressor_amd import ops

    T, k = idx.shape
    route = ops.moe_route(idx, m.num_experts)
    xq, xs = ops.mx_quant(x, m.act_fmt, m.kp_h)
    h = ops.mx_moe_gemm_glu(0, xq, xs, m.act_fmt, route, m.gate_up_qweight, m.gate_up_w_scale, m.w_fmt, T, k, bias=m.gate_up_bias,
                            alpha=m.alpha, limit=m.limit, out_dtype=cdt)
    hq, hs = ops.mx_quant(h, m.act_fmt, m.kp_i)
    y = ops.mx_moe_gemm_glu(1, hq, hs, m.act_fmt, route, m.down_qweight, m.down_w_scale, m.w_fmt, T, k, bias=m.down_bias,
                            routing_weights=w)
    return ops.moe_combine(y, route, T, k, m.num_experts, cdt), h, route


@pytest.mark.parametrize("xdtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_fused_forward_is_the_chain_of_the_six_calls(hip, pair, xdtype, monkeypatch):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts

    monkeypatch.setattr(MXGptOssExperts, "MOE_FUSED", True)
    monkeypatch.setattr(MXGptOssExperts, "MOE_MAX_ROWS", 64)
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


def _emulate_second_half(m, h, ro, w, cdt):
    """test_gpu_mx_moe._emulate_second_half with down_bias inside: float64 y[p] = w[order[p]] * (dequant(quant(h[p])) . Wd[e] +
    bd[e]) on the fused route's own h, combined in slot order -> (ref, bound) [T, H].  Per product PIPE * sum_k |a_k b_k| (the
    reasons are in that docstring), one fp32 rounding for the bias add, then k fp32 additions and one rounding to cdt."""
    T, k, nvalid = ro["T"], ro["k"], ro["nvalid"]
    afmt = m.act_fmt
    hq, hs = C.quant_mx(h[:nvalid].cpu(), afmt, m.kp_i)
    hd = C.dequant_mx(hq, hs, afmt)
    _, dn = m.recover(torch.float32)                                             # [E, I, H]
    dn = torch.nn.functional.pad(dn.cpu().double().transpose(1, 2), (0, m.kp_i - m.intermediate_dim))
    bd = m.down_bias.cpu().double()
    y = torch.zeros(nvalid, m.hidden_dim, dtype=torch.float64)
    ty = torch.zeros_like(y)
    order = ro["order"].long()
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo < hi:
            wt = w.reshape(-1).double().cpu()[order[lo:hi]][:, None]
            acc = hd[lo:hi] @ dn[e].T
            y[lo:hi] = wt * (acc + bd[e])
            ty[lo:hi] = wt.abs() * (PIPE * (hd[lo:hi].abs() @ dn[e].abs().T) + 2.0 ** -24 * (acc + bd[e]).abs())
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
    """Per element of h (CPU, [rows, K]): the spacing of the MX grid its quantisation lands on (test_gpu_mx_moe._grid_step)."""
    f = C._F[fmt]
    q, sb = C.quant_mx(h, fmt, Kp)
    v = C.dequant_mx(q, torch.full_like(sb, 127), fmt).abs()
    e = torch.where(v > 0, C._floor_log2(torch.where(v > 0, v, torch.ones_like(v))), torch.full_like(v, f["emin"], dtype=torch.int32))
    step = torch.ldexp(torch.ones_like(v), e.clamp(min=f["emin"]) - f["mb"])
    scale = torch.ldexp(torch.ones(sb.shape, dtype=torch.float64), sb.int() - 127)
    return (step.view(h.shape[0], Kp // 32, 32) * scale[:, :, None]).view(h.shape[0], Kp)


def _hf_forward(m, x, idx, w):
    """transformers' GptOssExperts in fp32 holding recover(torch.float32) and the biases, on the same inputs; a slot whose id is
    outside 0..E-1 goes to expert 0 with a zero routing weight, which adds zero."""
    E, H, I = m.num_experts, m.hidden_dim, m.intermediate_dim
    ref = _float_experts(E, H, I, torch.float32, 0).to(x.device)
    gu, dn = m.recover(torch.float32)
    gb, db = m.recover_biases(torch.float32)
    with torch.no_grad():
        for p, v in ((ref.gate_up_proj, gu), (ref.down_proj, dn), (ref.gate_up_proj_bias, gb), (ref.down_proj_bias, db)):
            p.copy_(v)
        valid = (idx >= 0) & (idx < E)
        return ref(x.float(), torch.where(valid, idx, torch.zeros_like(idx)), torch.where(valid, w.float(), torch.zeros_like(w.float())))


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_both_routes_against_the_emulation_fed_the_fused_h(hip, pair, monkeypatch):
    """test_gpu_mx_moe.test_both_routes_against_the_emulation_fed_the_fused_h with the GPT-OSS epilogue; the same tolerance
    construction.  The fused route is held to the emulation's own bound.  The dense route forms its own h from g and u ROUNDED to 16
    bits (after the bias add) and _apply_gate's five 16-bit operations (two clamps are exact; alpha g, the sigmoid, g sigmoid, u + 1
    and the product round):
        |dh| <= 1.5 (1.1 |g| (|u| + 1) u_out + 5 u_out |h|)      (|d (g sigmoid(alpha g)) / dg| <= 1.1, as for silu)
    and quantises that h: |dhq| <= |dh| + 2 step.  Then y (with its bias) is rounded to 16 bits, multiplied by the routing weight and
    rounded, and added in 16 bits (k roundings): (k + 2) u_out sum_s |w_s| (|h| . |Wd| + |bd|) on top.

    Against transformers' GptOssExperts in fp32 on the recovered weights (a record; T = 37, k = 2, E = 6, H = 200, I = 72, bf16): the
    relative Frobenius errors of both routes are printed; what is left is the quantisation error of the activations, which the float
    forward does not make.  Measured on an MI355X, fused / dense (dense against the emulation, over the same norm): (fp8, fp8)
    0.0499 / 0.0509 (0.0142); fp4 weights x fp8 0.0510 / 0.0505 (0.0122); (fp4, fp4) 0.2079 / 0.2082 (0.0325)."""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts

    cdt = torch.bfloat16
    _, m = _mx_experts(hip, pair, dtype=cdt)
    T, k = 37, 2
    x, idx, w = _inputs(hip, T, k, m.num_experts, 200, cdt, seed=5)
    monkeypatch.setattr(MXGptOssExperts, "MOE_FUSED", True)
    fused = m(x, idx, w)
    _, h, route = _six_calls(m, x, idx, w, cdt)
    ro = S.route_oracle(idx.cpu(), m.num_experts)
    S.assert_route(route.cpu(), ro)
    ref, tol = _emulate_second_half(m, h, ro, w, cdt)
    r, (i, j) = S.worst_ratio(fused.cpu(), ref, tol)
    print(f"fused against the emulation {C.PAIR_IDS[C.PAIRS.index(pair)]}: worst ratio {r:.4f}")
    assert r <= 1.0, (r, i, j)

    monkeypatch.setattr(MXGptOssExperts, "MOE_FUSED", False)
    dense = m(x, idx, w)
    assert dense.dtype is cdt and dense.shape == x.shape
    nvalid, order, I = ro["nvalid"], ro["order"].long(), m.intermediate_dim
    u_out, _ = S.out_rounding(cdt)
    xq, xs = ops.mx_quant(x, m.act_fmt, m.kp_h)
    gu = ops.mx_moe_gemm_glu(2, xq, xs, m.act_fmt, route, m.gate_up_qweight, m.gate_up_w_scale, m.w_fmt, T, k,
                             bias=m.gate_up_bias)[:nvalid].double().cpu()
    hf = h[:nvalid].double().cpu()
    gc, uc = gu[:, :I].clamp(max=m.limit), gu[:, I:].clamp(min=-m.limit, max=m.limit)
    dh = 1.5 * (1.1 * gu[:, :I].abs() * (uc.abs() + 1) * u_out + gc.abs() * gu[:, I:].abs() * u_out + 5 * u_out * hf.abs())
    dhq = torch.nn.functional.pad(dh, (0, m.kp_i - I)) + 2 * _grid_step(h[:nvalid].cpu(), m.act_fmt, m.kp_i)
    habs = torch.nn.functional.pad(hf.abs(), (0, m.kp_i - I))
    _, dn = m.recover(torch.float32)
    dn = torch.nn.functional.pad(dn.cpu().double().abs().transpose(1, 2), (0, m.kp_i - I))
    bd = m.down_bias.cpu().double().abs()
    extra = torch.zeros(nvalid, m.hidden_dim, dtype=torch.float64)
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo < hi:
            wt = w.reshape(-1).double().cpu()[order[lo:hi]][:, None].abs()
            extra[lo:hi] = wt * (dhq[lo:hi] @ dn[e].T + (k + 2) * u_out * (habs[lo:hi] @ dn[e].T + bd[e]))
    tol_dense = tol.clone()
    pos = ro["pos"].long().view(T, k)
    for s in range(k):
        p = pos[:, s]
        ok = p < nvalid
        tol_dense[ok] += extra[p[ok]]
    rd, (i, j) = S.worst_ratio(dense.cpu(), ref, tol_dense)
    print(f"dense against the emulation {C.PAIR_IDS[C.PAIRS.index(pair)]}: worst ratio {rd:.4f}")
    assert rd <= 1.0, (rd, i, j)

    # the record against transformers' float forward; the only gate: fused is not further from it than dense by more than dense's own
    # distance from the emulation
    hf_y = _hf_forward(m, x, idx, w).double().cpu()
    assert hf_y.shape == fused.shape and bool(torch.isfinite(hf_y).all()) and bool(torch.isfinite(fused).all())
    rel = lambda y: float((y.double().cpu() - hf_y).norm() / hf_y.norm())  # noqa: E731
    e_fused, e_dense = rel(fused), rel(dense)
    e_dense_emu = float((dense.double().cpu() - ref).norm() / hf_y.norm())
    print(f"against GptOssExperts fp32 {C.PAIR_IDS[C.PAIRS.index(pair)]}: fused {e_fused:.4f} dense {e_dense:.4f} "
          f"(dense against the emulation {e_dense_emu:.4f})")
    assert e_fused <= e_dense + e_dense_emu, (e_fused, e_dense, e_dense_emu)


def test_rows_above_the_threshold_take_the_dense_route(hip, monkeypatch):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts

    _, m = _mx_experts(hip, C.PAIRS[0], E=2, H=128, I=64)
    monkeypatch.setattr(MXGptOssExperts, "MOE_FUSED", True)
    monkeypatch.setattr(MXGptOssExperts, "MOE_MAX_ROWS", 4)
    calls = []
    real = ops.mx_moe_gemm_glu
    monkeypatch.setattr(ops, "mx_moe_gemm_glu", lambda *a, **kw: (calls.append(a[0]), real(*a, **kw))[1])
    for T, fused in ((4, True), (5, False)):                                 # T * k <= 4 * E = 8
        del calls[:]
        x, idx, w = _inputs(hip, T, 2, 2, 128, torch.bfloat16, seed=T, invalid=False)
        y = m(x, idx, w)
        assert calls == ([0, 1] if fused else []) and bool(torch.isfinite(y).all()), (T, calls)


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def _ids(n=2, seq=12):
    return torch.randint(0, 128, (n, seq), generator=torch.Generator().manual_seed(0))


@pytest.mark.parametrize("fp4", [False, True], ids=["fp8", "fp4_fp8"])
def test_model_with_quant_experts(hip, fp4, tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts, MXLinear, load
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    kw = dict(w_dtype="fp4", act_dtype="fp8_e4m3") if fp4 else {}
    float_model = G.tiny_gpt_oss(dtype=torch.bfloat16)
    names = [n for n, _ in G.gpt_oss_experts_of(float_model)]
    linears = [n for n, mod in float_model.named_modules() if isinstance(mod, torch.nn.Linear) and n != "lm_head"]
    q = quantize(G.tiny_gpt_oss(dtype=torch.bfloat16).to(hip), MXQuantConfig(quant_experts=True, **kw))
    assert len(names) == 2 and all(isinstance(q.get_submodule(n), MXGptOssExperts) for n in names)
    assert q.get_submodule(names[0]).w_dtype == ("fp4" if fp4 else "fp8_e4m3")
    assert linears and all(isinstance(q.get_submodule(n), MXLinear) for n in linears) and isinstance(q.lm_head, torch.nn.Linear)
    ids = _ids().to(hip)
    with torch.no_grad():
        y = q(ids).logits
    assert bool(torch.isfinite(y).all())
    q.save(str(tmp_path))
    back = load(str(tmp_path), G.tiny_gpt_oss(dtype=torch.bfloat16), device=hip)
    assert all(isinstance(back.get_submodule(n), MXGptOssExperts) for n in names)
    assert back.get_submodule(names[0]).alpha == 1.702 and back.get_submodule(names[0]).limit == 7.0
    sa, sb = q.state_dict(), back.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k_], sb[k_]) for k_ in sa)
    with torch.no_grad():
        assert torch.equal(back(ids).logits, y)


def test_model_without_quant_experts_is_as_before(hip):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts, MXLinear
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    float_model = G.tiny_gpt_oss(dtype=torch.bfloat16)
    names = [n for n, _ in G.gpt_oss_experts_of(float_model)]
    linears = [n for n, mod in float_model.named_modules() if isinstance(mod, torch.nn.Linear) and n != "lm_head"]
    want_keys = []
    for key in float_model.state_dict():
        owner = key.rsplit(".", 1)[0]
        want_keys += [owner + ".qweight", owner + ".w_scale"] if owner in linears and key.endswith(".weight") else [key]
    for cfg in (MXQuantConfig(), MXQuantConfig(quant_experts=False)):
        q = quantize(G.tiny_gpt_oss(dtype=torch.bfloat16).to(hip), cfg)
        assert not any(isinstance(mod, MXExperts) for mod in q.modules())
        assert all(type(q.get_submodule(n)) is type(float_model.get_submodule(n)) for n in names)
        assert all(isinstance(q.get_submodule(n), MXLinear) for n in linears)
        assert sorted(q.state_dict()) == sorted(want_keys)


def test_set_local_and_a_bare_dict_leave_the_module_float(hip):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts, MXGptOssExperts, MXQuantizer
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    model = G.tiny_gpt_oss(dtype=torch.bfloat16)
    names = [n for n, _ in G.gpt_oss_experts_of(model)]
    cfg = MXQuantConfig(w_dtype="fp4", act_dtype="fp8_e4m3", quant_experts=True)
    cfg.set_local(names[0], MXQuantConfig(w_dtype="fp32"))
    q = quantize(model.to(hip), cfg)
    assert type(q.get_submodule(names[0])).__name__ == "GptOssExperts"
    assert isinstance(q.get_submodule(names[1]), MXGptOssExperts) and q.get_submodule(names[1]).w_dtype == "fp4"
    with torch.no_grad():
        assert bool(torch.isfinite(q(_ids().to(hip)).logits).all())
    holder = torch.nn.Module()
    holder.oss = moe_models.tiny_gpt_oss_experts()
    holder.oss2 = moe_models.tiny_gpt_oss_experts()
    bare = {"w_dtype": "fp8_e4m3", "act_dtype": "fp8_e4m3"}
    out = MXQuantizer(quant_config={"oss": bare, "oss2": dict(bare, gpt_oss_experts=True)}).convert(holder)
    assert type(out.oss).__name__ == "GptOssExperts" and not isinstance(out.oss, MXExperts)
    assert isinstance(out.oss2, MXGptOssExperts)
