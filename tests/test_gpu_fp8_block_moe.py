"""-m gpu: inc_fp8_block_moe_gemm (exact operands bit-equal to float64, random codes within the instruction's allowance, one expert ==
inc_fp8_block_gemv) and FP8BlockExperts (buffers, the six-op chain, fused against dense, from_finegrained, recover, save / load)."""

import pytest
import torch

from tests import fp8_block_cases as B
from tests import fp8_cases as F
from tests import moe_models
from tests import moe_stage_cases as S
from tests.mx_moe_cases import route_of, routing_weights

pytestmark = pytest.mark.gpu
DTYPES16 = [torch.bfloat16, torch.float16]
PIPE = 2.0 ** -8                # the instruction's per-term allowance
TAB = F.code_table(F.FP8)
SENT = 0x7B5A
_reference, _exact = B.moe_reference, B.moe_exact


def _run(hip, mode, aq, as_, ro, wq, ws, rw=None, odtype=None):
    """The valid rows of the output on the CPU; the rows behind them keep the sentinel and a second call gives the same bits."""
    from neural_compressor_amd import ops
    T, k, nv, idt = ro["T"], ro["k"], ro["nvalid"], torch.int16 if mode == 0 else torch.int32
    args = [t.to(hip) for t in (aq, as_, S.route_buffer(ro, fill=-1), wq, ws)]
    outs = []
    for _ in range(2):
        out = torch.full((T * k, wq.shape[1] // (2 if mode == 0 else 1)), SENT, dtype=idt, device=hip).view(odtype if mode == 0 else torch.float32)
        ops.fp8_block_moe_gemm(mode, *args, T, k, routing_weights=None if rw is None else rw.to(hip), out=out)
        outs.append(out.cpu())
    assert bool((outs[0][nv:].view(idt) == SENT).all()), "wrote a row past the valid positions"
    assert torch.equal(outs[0].view(idt), outs[1].view(idt)), "repeated calls differ"
    return outs[0][:nv]


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("routing,Nout,Kp", B.MOE_EXACT)
def test_exact_operands_are_bit_equal_to_float64(hip, routing, Nout, Kp, mode):
    ro, aq, as_, wq, ws, val = _exact(routing, mode, Nout, Kp)
    rw = routing_weights(ro["T"], ro["k"], torch.float64)
    want = rw.reshape(-1)[ro["order"].long()[:ro["nvalid"]]][:, None] * val if mode == 1 else val
    assert bool((want.float().double() == want).all()) and (ro["nvalid"] > 0) == (routing != "all_invalid")
    for wdtype in ([torch.float32, torch.bfloat16] if mode == 1 else [None]):
        y = _run(hip, mode, aq, as_, ro, wq, ws, rw.to(wdtype) if mode == 1 else None)
        assert torch.equal(y.view(torch.int32), want.float().view(torch.int32)), (routing, Nout, Kp, mode, wdtype)


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("I,Kp", B.MOE_EXACT_MODE0)
def test_exact_operands_mode0(hip, I, Kp, dtype):
    ro, aq, as_, wq, ws, val = _exact("edges3", 0, I, Kp)
    ref, tol = S.mode0_tolerance(val[:, :I], val[:, I:], torch.zeros(()), torch.zeros(()), dtype)
    ok = 1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2
    assert float((~ok).double().mean()) <= 0.01
    bad = ok & ~((_run(hip, 0, aq, as_, ro, wq, ws, odtype=dtype).double() - ref).abs() <= tol)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[0].tolist())


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_random_codes_and_scales(hip, mode, Nout=260, Kp=640):
    ro = route_of("edges3")
    E, N, rows = ro["E"], (2 if mode == 0 else 1) * Nout, ro["S"] if mode == 1 else ro["T"]
    aq, as_ = F.random_codes(rows, 1, Kp, 9100 + mode)["xq"], B.random_scales(rows, 1, Kp, 9300 + mode)[0]
    wq = torch.stack([F.random_codes(1, N, Kp, 9200 + 10 * mode + e)["wq"] for e in range(E)])
    ws = torch.stack([torch.cat([B.random_scales(1, Nout, Kp, 9400 + 100 * mode + 2 * e + h)[1] for h in range(N // Nout)]) for e in range(E)])
    val, mass, _ = _reference(ro, mode, TAB[aq.long()], as_, TAB[wq.long()], ws)
    dv, rw = PIPE * mass + (Kp // B.B + 10) * 2.0 ** -24 * mass, S.make_routing_weights(ro["T"], ro["k"])
    for odtype in (DTYPES16 if mode == 0 else [None]):
        y = _run(hip, mode, aq, as_, ro, wq, ws, rw if mode == 1 else None, odtype)
        if mode == 0:
            ref, tol = S.mode0_tolerance(val[:, :Nout], val[:, Nout:], dv[:, :Nout], dv[:, Nout:], odtype)
            ok = ref.abs() + tol < float(torch.finfo(odtype).max) / 2
        else:
            w = rw.reshape(-1).double()[ro["order"].long()[:ro["nvalid"]]][:, None] if mode == 1 else torch.ones(())
            ref, tol, ok = w * val, w.abs() * dv, torch.ones_like(val, dtype=torch.bool)
        ratio = S.worst_ratio(torch.where(ok, y.double(), ref), ref, tol)[0]
        print(f"random codes and scales, mode {mode} {odtype}: worst |y - ref| / bound = {ratio:.4f} over {int(ok.sum())} outputs")
        assert float(ok.double().mean()) >= 0.5 and ratio <= 1.0


@pytest.mark.parametrize("rows", [1, 15, 16])
def test_one_expert_is_the_gemv(hip, rows, N=260, Kp=128 * 26):
    from neural_compressor_amd import ops
    rc, (xs, ws, _) = F.random_codes(rows, N, Kp, 9500 + rows), B.random_scales(rows, N, Kp, 9600 + rows)
    ro = S.route_oracle(torch.zeros(rows, 1, dtype=torch.int64), 1)             # T = rows, k = 1, E = 1: position p is token p
    y = _run(hip, 2, rc["xq"], xs, ro, rc["wq"][None], ws[None])
    want = ops.fp8_block_gemv(rc["xq"].to(hip), xs.to(hip), rc["wq"].to(hip), ws.to(hip), None, torch.bfloat16).cpu()
    assert bool(torch.isfinite(want.float()).all()) and torch.equal(y.to(torch.bfloat16), want)


class _Experts(torch.nn.Module):
    def __init__(self, E, H, I, act=None):
        super().__init__()
        g = torch.Generator().manual_seed(E + H + I)
        self.gate_up_proj = torch.nn.Parameter((torch.randn(E, 2 * I, H, generator=g) * 0.08).bfloat16())
        self.down_proj = torch.nn.Parameter((torch.randn(E, H, I, generator=g) * 0.08).bfloat16())
        self.act_fn = act if act is not None else torch.nn.SiLU()


@pytest.mark.parametrize("which", ["mixtral", "i136"])                           # I = 136: a second, partial block row per half
def test_module(hip, which, monkeypatch):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockExperts
    fl = moe_models.experts_of(moe_models.tiny_mixtral(dtype=torch.bfloat16))[0][1] if which == "mixtral" else _Experts(6, 200, 136)
    m = FP8BlockExperts.from_float(fl, device=hip)
    E, H, I = m.num_experts, m.hidden_dim, m.intermediate_dim
    rec, parts = m.recover(torch.float32), []
    for e in range(E):
        for w, q, s, got in ((fl.gate_up_proj[e, :I], m.gate_up_qweight[e, :I], m.gate_up_w_scale[e, 0], rec[0][e, :I]),
                             (fl.gate_up_proj[e, I:], m.gate_up_qweight[e, I:], m.gate_up_w_scale[e, 1], rec[0][e, I:]),
                             (fl.down_proj[e], m.down_qweight[e], m.down_w_scale[e], rec[1][e])):
            wq, wsc = B.quant_blocked(w.detach().cpu(), B.B)
            assert torch.equal(q.cpu(), wq) and torch.equal(s.cpu(), wsc), e
            want = (TAB.float()[wq.long()] * wsc.repeat_interleave(B.B, 0)[:w.shape[0]].repeat_interleave(B.B, 1))[:, :w.shape[1]]
            assert torch.equal(got.cpu(), want), e
            parts.append((wq[:, :w.shape[1]], wsc))
    # from_finegrained on the same bytes (float8 gate / down, uint8 up): the same state dict
    st = lambda i, j: torch.stack([parts[3 * e + i][j] for e in range(E)])  # noqa: E731
    fg = FP8BlockExperts.from_finegrained(st(0, 0).view(torch.float8_e4m3fn), st(0, 1), st(1, 0), st(1, 1), st(2, 0).view(torch.float8_e4m3fn),
                                          st(2, 1), float_type=torch.bfloat16, device=hip)
    assert list(m.state_dict()) == list(fg.state_dict()) and all(torch.equal(v, fg.state_dict()[key]) for key, v in m.state_dict().items())
    T, k, g = 37, 2, torch.Generator().manual_seed(37)
    x = (torch.randn(T, H, generator=g) * 1.5).bfloat16().to(hip)
    w, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=g), -1), k, dim=-1)
    idx[1, 0], idx[2, k - 1] = -1, E                                            # "no expert" sentinels: contribute nothing
    idx, w = idx.to(hip), w.to(hip)
    monkeypatch.setattr(FP8BlockExperts, "MOE_FUSED", True)
    fused = m(x, idx, w)
    route = ops.moe_route(idx, E)
    xq, xs = ops.fp8_quant_groups(x, m.kp_h)
    h = ops.fp8_block_moe_gemm(0, xq, xs, route, m.gate_up_qweight, m.gate_up_w_scale, T, k, out_dtype=torch.bfloat16)
    hq, hs = ops.fp8_quant_groups(h, m.kp_i)
    y = ops.fp8_block_moe_gemm(1, hq, hs, route, m.down_qweight, m.down_w_scale, T, k, routing_weights=w)
    assert torch.equal(fused, ops.moe_combine(y, route, T, k, E, torch.bfloat16)) and torch.equal(fused, fg(x, idx, w))
    # fused against dense: one output ulp plus, through `down`, the random test's product bound on both routes' own h.  The dense h
    # comes from g and u rounded to bf16 (|dh| <= 1.5 (1.1 |g| |u| + 3 |h|) u, test_gpu_fp8_moe.py) and is re-quantised (half an e4m3
    # step on either h); the dense route rounds y, its product with the routing weight and its k additions to bf16: (k + 2) u
    monkeypatch.setattr(FP8BlockExperts, "MOE_FUSED", False)
    dense = m(x, idx, w)
    ro = S.route_oracle(idx.cpu(), E)
    nv, order, u = ro["nvalid"], ro["order"].long(), 2.0 ** -8
    gv, uv = (ops.fp8_block_moe_gemm(2, xq, xs, route, m.gate_up_qweight[:, i * I:(i + 1) * I].contiguous(),
                                     m.gate_up_w_scale[:, i].contiguous(), T, k)[:nv].double().cpu() for i in range(2))
    hf = h[:nv].double().cpu()
    dh = 1.5 * u * (1.1 * gv.abs() * uv.abs() + 3 * hf.abs())
    dhq = dh + 2.0 ** -3 * (hf.abs() + dh) + 2.0 ** -9 * (hf.abs().amax(dim=1, keepdim=True) + dh.amax(dim=1, keepdim=True)) / 448.0
    dn, tol_p = rec[1].double().abs().cpu(), torch.zeros(nv, H, dtype=torch.float64)
    for e in range(E):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        wt = w.reshape(-1).double().cpu()[order[lo:hi]][:, None].abs()
        m_h, m_d = hf[lo:hi].abs() @ dn[e].T, dhq[lo:hi] @ dn[e].T
        tol_p[lo:hi] = wt * ((2 * PIPE + (2 * (m.kp_i // B.B + 10) + k + 2) * 2.0 ** -24 + (k + 2) * u) * (m_h + m_d) + (1 + PIPE) * m_d)
    tol, pos = torch.zeros(T, H, dtype=torch.float64), ro["pos"].long().view(T, k)
    for s in range(k):
        okp = pos[:, s] < nv
        tol[okp] += tol_p[pos[okp, s]]
    ratio = S.worst_ratio(dense.cpu(), fused.double().cpu(), tol + u * (fused.double().cpu().abs() + tol))[0]
    print(f"{which}: dense against fused, worst ratio {ratio:.4f}")
    assert ratio <= 1.0


def test_save_load_and_convert(hip, tmp_path, monkeypatch):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockExperts, FP8BlockLinear, FP8Experts, block_experts, load, save
    def build():
        model = torch.nn.Module()
        model.silu, model.gelu = _Experts(2, 128, 72), _Experts(2, 128, 64, act=torch.nn.GELU())
        model.token, model.lin = _Experts(3, 128, 64), torch.nn.Linear(128, 36).bfloat16()
        return model

    model, about = build(), []
    monkeypatch.setattr(block_experts.logger, "warning", lambda fmt, *a: about.append(fmt % a))
    assert block_experts.convert_block_experts(model, names=["silu", "gelu"], device=hip) is model
    assert isinstance(model.silu, FP8BlockExperts) and type(model.gelu) is _Experts and type(model.token) is _Experts
    assert len(about) == 1 and "gelu stays in floating point" in about[0] and "GELU is not SiLU" in about[0], about
    model.token, model.lin = FP8Experts.from_float(model.token, device=hip), FP8BlockLinear.from_float(model.lin, device=hip)
    save(model, str(tmp_path))
    back = load(str(tmp_path), build(), device=hip)
    assert [type(getattr(back, n)) for n in ("silu", "gelu", "token", "lin")] == [FP8BlockExperts, _Experts, FP8Experts, FP8BlockLinear]
    sa, sb = model.state_dict(), back.state_dict()
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[key], sb[key].to(sa[key].device)) for key in sa)
