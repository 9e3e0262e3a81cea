"""-m gpu: inc_mx_wo_moe_gemm / _glu and MXWeightOnlyExperts / MXWeightOnlyGptOssExperts.  mx_moe_cases.exact_case activations are
integers -3..3 times a power of two, so ad.bfloat16() is exact and M.reference / G.reference are this kernel's float64 results too."""

import pytest
import torch

from tests import moe_models
from tests import moe_stage_cases as S
from tests import mx_cases as C
from tests import mx_gpt_oss_cases as G
from tests import mx_moe_cases as M

pytestmark = pytest.mark.gpu

SENT16, SENT32, GUARD = 0x7B5A, 0x7B5A7B5A, 16
ALPHA, LIMIT = 1.702, 7.0
BF16 = torch.bfloat16
FMTS, FMT_IDS = [C.FP4, C.FP8], ["fp4", "fp8"]
WO = dict(w_dtype="fp4", act_dtype="bf16", weight_only=True, quant_experts=True)


def _launch(hip, mode, x, ro, wq, ws, wfmt, glu, rw=None, bias=None, nan_around_x=False):
    """One ops call, `out` inside sentinels, x [rows, K] (CPU) inside its own buffer -> the valid rows [nvalid, Nout] on the CPU."""
    from neural_compressor_amd import ops

    T, k, Sn, nv = ro["T"], ro["k"], ro["S"], ro["nvalid"]
    Nout = wq.shape[1] // 2 if mode == 0 else wq.shape[1]
    idt, sent, odt = (torch.int16, SENT16, BF16) if mode == 0 else (torch.int32, SENT32, torch.float32)
    xbuf = torch.full((8 + x.numel() + 256,), float("nan") if nan_around_x else 0.0, dtype=BF16)
    xbuf[8:8 + x.numel()] = x.reshape(-1)
    xd = xbuf.to(hip)[8:8 + x.numel()].view(x.shape)
    route = S.route_buffer(ro, fill=-1).to(hip)
    kw = dict(routing_weights=None if rw is None else rw.to(hip))
    if glu:
        kw.update(bias=None if bias is None else bias.float().contiguous().to(hip), alpha=ALPHA, limit=LIMIT)
    raws = []
    for _ in range(2):
        buf = torch.full((GUARD + Sn * Nout + GUARD,), sent, dtype=idt, device=hip)
        out = buf[GUARD:GUARD + Sn * Nout].view(odt).view(Sn, Nout)
        (ops.mx_wo_moe_gemm_glu if glu else ops.mx_wo_moe_gemm)(mode, xd, route, wq.to(hip), ws.to(hip), wfmt, T, k, out=out, **kw)
        raws.append(buf.cpu())
    raw = raws[0]
    assert torch.equal(raw, raws[1]), "repeated calls differ"
    assert bool((raw[:GUARD] == sent).all()) and bool((raw[GUARD + nv * Nout:] == sent).all()), "wrote outside the valid rows"
    return raw[GUARD:GUARD + nv * Nout].view(odt).view(nv, Nout)


def _exact(hip, d, wfmt, glu, K=None):
    """Exact case d through one entry -> the gate's verdict.  K < Kp: NaN behind x, the oracle copy's columns at k >= K are zero."""
    E, N, Kp = d["w"].shape
    if K is not None:
        d = {key: v for key, v in d.items() if isinstance(key, str)}
        d["ad"] = d["ad"].clone()
        d["ad"][:, K:] = 0
    wq = C.stored(C.encode_values(d["w"].view(E * N, Kp), wfmt), wfmt).view(E, N, -1)
    x = d["ad"][:, :K].bfloat16()
    assert torch.equal(x.double(), d["ad"][:, :K])
    y = _launch(hip, d["mode"], x, d["ro"], wq, d["ws"], wfmt, glu, d["rw"].float() if d["mode"] == 1 else None,
                G.bias_of(E, N) if glu else None, nan_around_x=K is not None)
    dt = BF16 if d["mode"] == 0 else None
    return G.check_output(d, y, ALPHA, LIMIT, dt) if glu else M.check_output(d, y, dt)


SHORT = [(M.case(n), m, s) for n, m in (("kW_plus1", 2), ("short_waves", 0)) for s in (64, 120)]     # K = Kp - s: GPT-OSS's situation


@pytest.mark.parametrize("rule", M.RULES)
@pytest.mark.parametrize("wfmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("cms", [(c, m, 0) for c, m in M.CASE_MODES] + SHORT, ids=M.CASE_MODE_IDS + [f"{c.name}-mode{m}-K-{s}" for c, m, s in SHORT])
def test_exact_operands(hip, cms, wfmt, rule):
    c, mode, short = cms
    d = M.exact_case(c, mode, rule)
    G.assert_exact_condition(d)
    for glu in (False, True):
        why = _exact(hip, d, wfmt, glu, d["w"].shape[2] - short if short else None)
        assert why is None, f"{c.name} mode {mode} {rule} glu={glu} short={short}: {why}"


@pytest.mark.parametrize("wfmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("T", [5, 16])
def test_one_experts_rows_are_the_gemv(hip, T, wfmt):
    """E = 1, k = 1, K = 1152 (9 K-tiles: more than the waves): mode 2 rounded once is inc_mx_wo_gemv's output."""
    from neural_compressor_amd import ops

    p = C.random_operands(T, 40, 1152, C.FP8, wfmt, seed=77)
    x = torch.randn(T, 1152, generator=torch.Generator().manual_seed(T)).bfloat16()
    wq, ws = C.stored(p["wq"], wfmt), p["ws"]
    ro = S.route_oracle(torch.zeros(T, 1, dtype=torch.int64), 1)
    y = _launch(hip, 2, x, ro, wq[None], ws[None], wfmt, False)
    want = ops.mx_wo_gemv(x.to(hip), wq.to(hip), ws.to(hip), wfmt, None, BF16).cpu()
    assert torch.equal(y[ro["pos"].long().view(-1)].bfloat16().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("wfmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_random_operands_are_within_the_chain_bound(hip, mode, wfmt):
    """M.random_gate with the reference recomputed from x.double(): Kp 2^-23 (|x| . |W|), times |w| in mode 1, mode0_tolerance in mode 0."""
    d = M.random_case(mode, C.FP8, wfmt)
    ro = d["ro"]
    x = d["ad"].bfloat16()
    d = dict(d, ad=x.double())
    nv, order, k = ro["nvalid"], ro["order"].long(), ro["k"]
    acc, mass = torch.zeros(nv, d["N"], dtype=torch.float64), torch.zeros(nv, d["N"], dtype=torch.float64)
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        r = d["ad"][lo:hi] if mode == 1 else d["ad"][order[lo:hi] // k]
        acc[lo:hi], mass[lo:hi] = r @ d["wd"][e].T, r.abs() @ d["wd"][e].abs().T
    d["acc"], d["dacc"] = acc, d["Kp"] * 2.0 ** -23 * mass
    ref, tol, ok = M.random_gate(d, BF16)
    assert float(ok.double().mean()) >= 0.5, "too few comparable outputs"
    y = _launch(hip, mode, x[:, :600], ro, d["wq"], d["ws"], wfmt, False, d["rw"] if mode == 1 else None)
    err = (y.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)[ok]
    print(f"random mode {mode} {C.FMT_IDS[wfmt]}: worst |y - ref| / bound = {float(ratio.max()):.4f} over {int(ok.sum())} outputs")
    assert bool(torch.isfinite(y[ok].float()).all()) and float(ratio.max()) <= 1.0


# ---- modules -------------------------------------------------------------------------------------------------------------------------
def _modules(hip, oss, wfmt, E=6, H=200, I=72, dtype=BF16):
    """(parent-class module, weight-only module) from the same float experts."""
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts, MXGptOssExperts, MXWeightOnlyExperts, MXWeightOnlyGptOssExperts
    from tests.test_gpu_mx_gpt_oss import _float_experts

    if oss:
        fl = _float_experts(E, H, I, dtype, 3)
    else:
        fl = moe_models.experts_of(moe_models.tiny_qwen3_moe(dtype=dtype))[0][1]
    name = C.FMT_NAMES[wfmt]
    return ((MXGptOssExperts if oss else MXExperts).from_float(fl, w_dtype=name, device=hip),
            (MXWeightOnlyGptOssExperts if oss else MXWeightOnlyExperts).from_float(fl, w_dtype=name, device=hip))


def _four_calls(m, x, idx, w, oss):
    from neural_compressor_amd import ops

    T, k = idx.shape
    route = ops.moe_route(idx, m.num_experts)
    xb = x.to(BF16)
    gemm = ops.mx_wo_moe_gemm_glu if oss else ops.mx_wo_moe_gemm
    e0, e1 = (dict(bias=m.gate_up_bias, alpha=m.alpha, limit=m.limit), dict(bias=m.down_bias)) if oss else ({}, {})
    h = gemm(0, xb, route, m.gate_up_qweight, m.gate_up_w_scale, m.w_fmt, T, k, **e0)
    y = gemm(1, h, route, m.down_qweight, m.down_w_scale, m.w_fmt, T, k, routing_weights=w, **e1)
    return ops.moe_combine(y, route, T, k, m.num_experts, BF16)


def _float64_forward(m, x, idx, w, oss, dense):
    """(ref, bound) [T, H]: the plain float64 forward on recover(float64) and x.bfloat16().  The bound, from the project's terms only: h
    is off by S.mode0_tolerance / G.mode0_gate (sensitivity 1.1) with dg, du = Kp(H) 2^-23 of the mass + one fp32 rounding of the bias
    add; dh goes through |Wd|; the down product adds Kp(I) 2^-23 of its mass, bias add and routing weight 2^-22 |y|; combine k fp32
    additions and S.out_rounding(bf16).  The dense route also rounds g, u (u_out each), the activation's 16-bit operations (2 for SiLU,
    5 for _apply_gate: 1.5 u_out |h| each, as test_gpu_mx_gpt_oss enumerates) and y, w y and the k additions ((k + 2) u_out)."""
    E, I, k = m.num_experts, m.intermediate_dim, idx.shape[1]
    gu, dn = (t.cpu() for t in m.recover(torch.float64))
    if oss:
        gu, dn = torch.cat([gu[:, :, 0::2], gu[:, :, 1::2]], 2).transpose(1, 2), dn.transpose(1, 2)   # kernel order: [E, 2I, H], [E, H, I]
    bg = m.gate_up_bias.cpu().double() if oss else torch.zeros(E, 2 * I, dtype=torch.float64)
    bd = m.down_bias.cpu().double() if oss else torch.zeros(E, m.hidden_dim, dtype=torch.float64)
    xb, u16 = x.bfloat16().double().cpu(), 2.0 ** -8
    ref, tol, mag = (torch.zeros(x.shape[0], m.hidden_dim, dtype=torch.float64) for _ in range(3))
    for t in range(x.shape[0]):
        for s in range(k):
            e, wt = int(idx[t, s]), abs(float(w[t, s]))
            if not 0 <= e < E:
                continue
            a, amass = gu[e] @ xb[t] + bg[e], gu[e].abs() @ xb[t].abs()
            da = m.kp_h * 2.0 ** -23 * amass + 2.0 ** -24 * a.abs() + (u16 * a.abs() if dense else 0)
            g, u, dg, du = a[:I], a[I:], da[:I], da[I:]
            h, th = G.mode0_gate(g, u, m.alpha, m.limit, BF16, dg, du)[:2] if oss else S.mode0_tolerance(g, u, dg, du, BF16)
            th = th + (1.5 * (5 if oss else 2) * u16 * h.abs() if dense else 0)
            y, ymass = dn[e] @ h + bd[e], dn[e].abs() @ h.abs() + bd[e].abs()
            ty = dn[e].abs() @ th + m.kp_i * 2.0 ** -23 * ymass + 2.0 ** -22 * y.abs() + ((k + 2) * u16 * (ymass + dn[e].abs() @ th) if dense else 0)
            ref[t], tol[t], mag[t] = ref[t] + float(w[t, s]) * y, tol[t] + wt * ty, mag[t] + wt * (y.abs() + ty)
    tol = tol + k * 2.0 ** -24 * mag
    return ref, tol + u16 * (ref.abs() + tol)


@pytest.mark.parametrize("wfmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("oss", [False, True], ids=["silu", "gpt_oss"])
def test_modules(hip, oss, wfmt, monkeypatch):
    parent, m = _modules(hip, oss, wfmt)
    assert list(parent.state_dict()) == list(m.state_dict()) and all(torch.equal(v, m.state_dict()[n]) for n, v in parent.state_dict().items())
    assert (m.act_dtype, m.act_fmt) == ("bf16", None) and m._fusable()
    E, H = m.num_experts, m.hidden_dim
    for T, k, xdtype in ((1, 2, BF16), (37, 2, torch.float16), (5, 1, torch.float32)):
        g = torch.Generator().manual_seed(T)
        x = (torch.randn(T, H, generator=g) * 1.5).to(xdtype).to(hip)
        w, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=g), -1), k, dim=-1)
        if T > 2:
            idx[1, 0], idx[2, k - 1] = -1, E
        with monkeypatch.context() as mp:
            for name in ("item", "tolist", "cpu", "nonzero"):
                mp.setattr(torch.Tensor, name, lambda self, *a, **kw: pytest.fail("host read in a fused forward"))
            fused = m(x, idx.to(hip), w.to(hip))
        assert fused.dtype is xdtype and torch.equal(fused, _four_calls(m, x, idx.to(hip), w.to(hip), oss).to(xdtype)), (T, k)
        with monkeypatch.context() as mp:
            mp.setattr(type(m), "MOE_FUSED", False)
            dense = m(x, idx.to(hip), w.to(hip))
        for y, is_dense in ((fused, False), (dense, True)):
            ref, tol = _float64_forward(m, x, idx, w, oss, is_dense)
            r, at = S.worst_ratio(y.bfloat16().cpu(), ref, tol)
            print(f"{'dense' if is_dense else 'fused'} T {T} {C.FMT_IDS[wfmt]} oss={oss}: worst ratio {r:.4f}")
            assert r <= 1.0, (is_dense, T, r, at)


def test_threshold_switches_routes_and_from_mxfp4_is_the_checkpoint(hip, monkeypatch):
    from transformers.integrations.mxfp4 import convert_moe_packed_tensors

    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXWeightOnlyGptOssExperts as W

    E, H, I = 3, 160, 96
    g = torch.Generator().manual_seed(11)
    gub, dnb = (torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in ((E, 2 * I, H // 32, 16), (E, H, I // 32, 16)))
    gus, dns = (torch.randint(118, 130, s, generator=g, dtype=torch.uint8) for s in ((E, 2 * I, H // 32), (E, H, I // 32)))
    m = W.from_mxfp4(gub, gus, torch.randn(E, 2 * I, generator=g), dnb, dns, torch.randn(E, H, generator=g), device=hip)
    for got, blocks, scales in zip(m.recover(torch.float32), (gub, dnb), (gus, dns)):
        want = convert_moe_packed_tensors(blocks, scales, dtype=torch.float32)
        assert torch.equal(got.cpu().contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    calls, real = [], ops.mx_wo_moe_gemm_glu
    monkeypatch.setattr(ops, "mx_wo_moe_gemm_glu", lambda *a, **kw: (calls.append(a[0]), real(*a, **kw))[1])
    monkeypatch.setattr(W, "MOE_MAX_ROWS", 4)
    for T, fused in ((4 * E, True), (4 * E + 1, False)):                      # k = 1: T * k = 4 E + 1 takes the dense route
        del calls[:]
        y = m(torch.randn(T, H, device=hip).bfloat16(), torch.arange(T, device=hip)[:, None] % E, torch.ones(T, 1, device=hip))
        assert calls == ([0, 1] if fused else []) and bool(torch.isfinite(y).all()), (T, calls)


@pytest.mark.parametrize("oss", [False, True], ids=["qwen3_moe", "gpt_oss"])
def test_model(hip, oss, tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXWeightOnlyExperts, MXWeightOnlyGptOssExperts, MXWeightOnlyLinear, load
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    build = (lambda: G.tiny_gpt_oss(dtype=BF16)) if oss else (lambda: moe_models.tiny_qwen3_moe(dtype=BF16))
    fl = build()
    names = [n for n, _ in (G.gpt_oss_experts_of(fl) if oss else moe_models.experts_of(fl))]
    linears = [n for n, mod in fl.named_modules() if isinstance(mod, torch.nn.Linear) and n != "lm_head"]
    cfg = MXQuantConfig(**WO)
    cfg.set_local(names[0], MXQuantConfig(w_dtype="fp32"))
    q = quantize(build().to(hip), cfg)
    cls = MXWeightOnlyGptOssExperts if oss else MXWeightOnlyExperts
    assert type(q.get_submodule(names[0])) is type(fl.get_submodule(names[0]))
    assert len(names) > 1 and all(type(q.get_submodule(n)) is cls for n in names[1:])
    assert linears and all(type(q.get_submodule(n)) is MXWeightOnlyLinear for n in linears)
    ids = torch.randint(0, 128, (2, 12), generator=torch.Generator().manual_seed(0)).to(hip)
    with torch.no_grad():
        y = q(ids).logits
        assert bool(torch.isfinite(y).all())
        q.save(str(tmp_path))
        back = load(str(tmp_path), build(), device=hip)
        sa, sb = q.state_dict(), back.state_dict()
        assert type(back.get_submodule(names[1])) is cls and list(sa) == list(sb) and all(torch.equal(sa[n], sb[n]) for n in sa)
        assert torch.equal(back(ids).logits, y)
