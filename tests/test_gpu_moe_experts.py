"""-m gpu: weight-only INT4 fused MoE experts (MI355XWeightOnlyExperts, inc_moe_route / inc_woq_moe_gemm / inc_moe_combine, DESIGN K4e).
The weight each expert decodes is recover(x.dtype) bit for bit (identity rows), the module matches an fp32 referee at the Mixtral and
Qwen3-MoE expert shapes for every T, routing edge cases hold, repeated calls and a captured graph are bit-identical, recover() never
runs on the fused route, and RTN packs the experts of tiny Mixtral / Qwen3-MoE models."""

import pytest
import torch
import torch.nn.functional as F

from tests.moe_models import experts_of, tiny_mixtral, tiny_qwen3_moe

pytestmark = pytest.mark.gpu

TS = [1, 4, 16, 64, 256, 1024, 4096]


def _experts(hip, E, H, I, gs, asym=False, seed=0, scale=0.002):
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts

    g = torch.Generator(device=hip).manual_seed(seed)
    m = MI355XWeightOnlyExperts(E, H, I, bits=4, group_size=gs, device=hip)
    parts = []
    for N, K in ((2 * I, H), (H, I)):
        G = K // (K if gs == -1 else gs)
        lo, hi = (0, 16) if asym else (-8, 8)
        iw = torch.randint(lo, hi, (E, N, K), generator=g, device=hip, dtype=torch.int32)
        sc = torch.rand(E, N, G, generator=g, device=hip) * scale + scale / 4
        zp = torch.randint(0, 16, (E, N, G), generator=g, device=hip, dtype=torch.int32) if asym else None
        parts += [iw, sc, zp]
    m.pack(*parts)
    return m


def _routing(hip, T, E, k, seed=1):
    g = torch.Generator(device=hip).manual_seed(seed)
    logits = torch.randn(T, E, generator=g, device=hip)
    w, idx = torch.topk(torch.softmax(logits, dim=-1), k, dim=-1)
    return idx, (w / w.sum(-1, keepdim=True)).to(torch.bfloat16)


def _referee(m, x, idx, w):
    """fp32 forward on the recovered weights (the bf16 weights the kernels decode), transformers' loop order."""
    gu, dn = m.recover(x.dtype)
    xf, out = x.float(), torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in range(m.num_experts):
        tok, pos = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        gate, up = F.linear(xf[tok], gu[e].float()).chunk(2, dim=-1)
        h = F.silu(gate) * up
        out.index_add_(0, tok, F.linear(h, dn[e].float()) * w[tok, pos, None].float())
    return out


def _check(y, ref, bar=2.0**-7):
    err = float((y.float() - ref).abs().max())
    bar = bar * float(ref.abs().max())
    assert err <= bar, f"max error {err} > {bar}"


# 1. bit-exact decode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("gs", [32, 128])
def test_decoded_weight_is_recover(hip, asym, gs, dtype):
    from neural_compressor_amd import ops

    E, H, I = 4, 256, 512
    m = _experts(hip, E, H, I, gs, asym=asym)
    gu, dn = m.recover(dtype)
    for name, (qw, sc, qz), W in (("gate_up", m._bufs("gate_up"), gu), ("down", m._bufs("down"), dn)):
        K = qw.shape[1] * 8
        x = torch.eye(K, dtype=dtype, device=hip)
        for e in (0, E - 1):
            idx = torch.full((K, 1), e, dtype=torch.int64, device=hip)
            route = ops.moe_route(idx, E)
            y = ops.woq_moe_gemm(2, x, route, qw, sc, qz, K, 1, gs)
            assert torch.equal(y.t(), W[e].float()), f"{name} expert {e}"


# 2. fp32 referee at the production expert shapes ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixtral_experts(hip):
    return _experts(hip, 8, 4096, 14336, 128, asym=True, seed=2)


@pytest.fixture(scope="module")
def qwen3_experts(hip):
    return _experts(hip, 128, 2048, 768, 128, asym=False, seed=3, scale=0.004)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", ["mixtral", "qwen3"])
def test_referee_production_shapes(hip, request, monkeypatch, shape, T):
    m = request.getfixturevalue(f"{shape}_experts")
    monkeypatch.setattr(type(m), "MOE_MAX_ROWS", 1 << 30)  # the fused route at every T
    k = 2 if shape == "mixtral" else 8
    idx, w = _routing(hip, T, m.num_experts, k, seed=T)
    x = torch.randn(T, m.hidden_dim, device=hip).to(torch.bfloat16)
    with torch.no_grad():
        y = m(x, idx, w)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    _check(y, _referee(m, x, idx, w))


# 3. routing edge cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["idle_experts", "one_expert", "ragged", "invalid_ids"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_routing_edge_cases(hip, monkeypatch, case, dtype):
    E, H, I, k = 8, 256, 512, 2
    m = _experts(hip, E, H, I, 32, asym=True, seed=4)
    T = 37 if case == "ragged" else 100  # 74 slots: not a multiple of the 64-row tile
    g = torch.Generator(device=hip).manual_seed(5)
    if case == "idle_experts":  # experts 1, 2, 4..7 get nothing
        idx = torch.stack([torch.zeros(T, dtype=torch.int64, device=hip), torch.full((T,), 3, dtype=torch.int64, device=hip)], 1)
    elif case == "one_expert":  # every token's first choice is expert 5
        idx = torch.stack([torch.full((T,), 5, dtype=torch.int64, device=hip), torch.randint(0, 5, (T,), generator=g, device=hip)], 1)
    else:
        idx, _ = _routing(hip, T, E, k, seed=6)
    if case == "invalid_ids":  # a "no expert" sentinel and an id past the last expert contribute nothing
        idx = idx.clone()
        idx[::3, 1] = -1
        idx[1::5, 0] = E
    w = torch.rand(T, k, generator=g, device=hip)
    x = torch.randn(T, H, generator=g, device=hip).to(dtype)
    ref = _referee(m, x, idx, w)
    with torch.no_grad():
        y = m(x, idx, w)
    _check(y, ref)
    if case == "invalid_ids":  # the dense route agrees
        monkeypatch.setattr(type(m), "MOE_FUSED", False)
        with torch.no_grad():
            _check(m(x, idx, w), ref, bar=2.0**-6)


# 4. / 5. determinism and graph capture --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 16, 256])
def test_repeated_calls_bit_identical(hip, qwen3_experts, T):
    m = qwen3_experts
    idx, w = _routing(hip, T, m.num_experts, 8, seed=7)
    x = torch.randn(T, m.hidden_dim, device=hip).to(torch.bfloat16)
    with torch.no_grad():
        ys = [m(x, idx, w) for _ in range(3)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_graph_capture_decode(hip, mixtral_experts):
    m = mixtral_experts
    idx, w = _routing(hip, 1, m.num_experts, 2, seed=8)
    x = torch.randn(1, m.hidden_dim, device=hip).to(torch.bfloat16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        eager = m(x, idx, w)  # builds the prepared call and its buffers outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = m(x, idx, w)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(torch.randn(1, m.hidden_dim, device=hip).to(torch.bfloat16))
    graph.replay()
    with torch.no_grad():
        assert torch.equal(out, m(x, idx, w))


def test_many_shapes_bounded_memory_and_graph_survives(hip, qwen3_experts):
    """Calls at more than 8 distinct T keep only the split-K workspace (intermediates are per call), and a decode graph captured
    before them still replays equal to eager."""
    m = qwen3_experts
    idx1, w1 = _routing(hip, 1, m.num_experts, 8, seed=12)
    x1 = torch.randn(1, m.hidden_dim, device=hip).to(torch.bfloat16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        m(x1, idx1, w1)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = m(x1, idx1, w1)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    call = m.__dict__["_call"]
    from neural_compressor_amd._lib import lib

    Ts = [2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 200, 256]
    need = max(max(lib.inc_woq_moe_gemm_workspace_bytes(0, T, 8, m.num_experts, 2 * m.intermediate_dim, m.hidden_dim),
                   lib.inc_woq_moe_gemm_workspace_bytes(1, T, 8, m.num_experts, m.hidden_dim, m.intermediate_dim)) for T in Ts + [1])
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        for T in Ts:
            idx, w = _routing(hip, T, m.num_experts, 8, seed=T)
            x = torch.randn(T, m.hidden_dim, device=hip).to(torch.bfloat16)
            y = m(x, idx, w)
            del idx, w, x, y
    torch.cuda.synchronize()
    assert m.__dict__["_call"] is call
    assert call.held_bytes() < 4 * need  # (the grow-only workspace bound, WoqMoeCall)
    assert torch.cuda.memory_allocated() - base < 4 * need
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(out, m(x1, idx1, w1))


# 6. / 7. recover() stays off the fused route; MOE_MAX_ROWS routes larger batches to the dense route -----------------------------
def test_fused_route_never_recovers(hip, monkeypatch):
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts

    m = _experts(hip, 8, 256, 512, 64, seed=9)
    idx, w = _routing(hip, 16, 8, 2, seed=10)
    x = torch.randn(16, 256, device=hip).to(torch.bfloat16)
    ref = _referee(m, x, idx, w)

    def boom(*a, **k):
        raise AssertionError("recover() on the fused route")

    monkeypatch.setattr(MI355XWeightOnlyExperts, "recover", boom)
    with torch.no_grad():
        y = m(x, idx, w)
    _check(y, ref)


def test_max_rows_routing(hip, monkeypatch):
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts

    m = _experts(hip, 8, 256, 512, 32, seed=11)
    calls = []
    orig = MI355XWeightOnlyExperts.recover
    monkeypatch.setattr(MI355XWeightOnlyExperts, "recover", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    monkeypatch.setattr(MI355XWeightOnlyExperts, "MOE_MAX_ROWS", 1)  # T * k <= 1 * E = 8 routed rows: fused
    for T, dense in ((4, False), (5, True)):
        idx, w = _routing(hip, T, 8, 2, seed=T)
        x = torch.randn(T, 256, device=hip).to(torch.bfloat16)
        calls.clear()
        with torch.no_grad():
            y = m(x, idx, w)
        assert bool(calls) == dense
        _check(y, _referee(m, x, idx, w), bar=2.0**-6 if dense else 2.0**-7)  # (the dense route rounds every eager step to bf16)
    monkeypatch.setattr(MI355XWeightOnlyExperts, "MOE_FUSED", False)
    calls.clear()
    with torch.no_grad():
        m(x[:1], idx[:1], w[:1])
    assert calls


def test_empty_batch_is_zeros(hip, monkeypatch):
    m = _experts(hip, 8, 256, 512, 32, seed=11)
    idx, w = _routing(hip, 4, 8, 2, seed=4)
    x = torch.randn(4, 256, device=hip).to(torch.bfloat16)
    for fused in (True, False):
        monkeypatch.setattr(type(m), "MOE_FUSED", fused)
        with torch.no_grad():
            y = m(x[:0], idx[:0], w[:0])
            y3 = m(x.reshape(1, 4, 256)[:, :0], idx[:0], w[:0])
            yk = m(x, idx[:, :0], w[:, :0])
        assert y.shape == (0, 256) and y.dtype == torch.bfloat16
        assert y3.shape == (1, 0, 256) and y3.dtype == torch.bfloat16
        assert yk.shape == x.shape and yk.dtype == torch.bfloat16 and not yk.any()


# 8. model level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [tiny_mixtral, tiny_qwen3_moe])
def test_rtn_model(hip, tmp_path, make):
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear
    from neural_compressor_amd.torch.algorithms.weight_only.save_load import load, save
    from neural_compressor_amd.torch.algorithms.weight_only.utility import quant_tensor
    from neural_compressor_amd.torch.quantization import RTNConfig, quantize

    float_model = make(dtype=torch.bfloat16).to(hip)
    names = [n for n, _ in experts_of(float_model)]
    floats = {n: (m.gate_up_proj.detach().clone(), m.down_proj.detach().clone()) for n, m in experts_of(float_model)}
    q = quantize(make(dtype=torch.bfloat16), RTNConfig(bits=4, group_size=32, use_sym=False))
    off = quantize(make(dtype=torch.bfloat16), RTNConfig(bits=4, group_size=32, use_sym=False).set_local(".*experts", RTNConfig(dtype="fp32")))
    mods = dict(q.named_modules())
    assert all(isinstance(mods[n], MI355XWeightOnlyExperts) for n in names)
    # codes and scales of each expert == quant_tensor on that expert's slice, packed as MI355XWeightOnlyLinear packs it
    for n in names:
        em = mods[n]
        for (prefix, p), W in zip((("gate_up", 0), ("down", 1)), floats[n]):
            qw, sc, qz = em._bufs(prefix)
            for e in range(em.num_experts):
                iw, s, zp = quant_tensor(W[e].clone(), dtype="int", bits=4, group_size=32, scheme="asym", return_int=True)
                lin = MI355XWeightOnlyLinear(W.shape[2], W.shape[1], bits=4, group_size=32, zp=True, device=hip)
                lin.pack(iw, s, zp, None)
                assert torch.equal(qw[e], lin.qweight) and torch.equal(sc[e], lin.scales) and torch.equal(qz[e], lin.qzeros)
    # the Linear modules are exactly what the opt-out model has
    offm = dict(off.named_modules())
    assert not any(isinstance(m, MI355XWeightOnlyExperts) for m in off.modules())
    for name, m in q.named_modules():
        if isinstance(m, MI355XWeightOnlyLinear):
            for b in ("qweight", "scales", "qzeros"):
                assert torch.equal(getattr(m, b), getattr(offm[name], b)), name
    # logits vs a float model that carries the recovered expert weights (and the same packed Linears)
    ids = torch.randint(0, 128, (2, 24), generator=torch.Generator().manual_seed(0)).to(hip)
    with torch.no_grad():
        logits = q(ids).logits.float()
        for n in names:
            gu, dn = mods[n].recover(torch.bfloat16)
            offm[n].gate_up_proj.data.copy_(gu)
            offm[n].down_proj.data.copy_(dn)
        ref = off(ids).logits.float()
    assert float((logits - ref).norm() / ref.norm()) <= 2e-2
    # default-format round trip
    save(q, str(tmp_path / "default"))
    back = load(str(tmp_path / "default"), original_model=make(dtype=torch.bfloat16), device=hip)
    bmods = dict(back.named_modules())
    for n in names:
        assert isinstance(bmods[n], MI355XWeightOnlyExperts)
        for k, v in mods[n].state_dict().items():
            assert torch.equal(v, bmods[n].state_dict()[k])
    with torch.no_grad():
        assert torch.equal(back(ids).logits.float(), logits)
    with pytest.raises(ValueError):
        save(q, str(tmp_path / "hf"), format="huggingface")


@pytest.mark.parametrize("cfg", [dict(bits=8), dict(dtype="nf4"), dict(use_mse_search=True)])
def test_unsupported_configs_stay_float(hip, cfg):
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts
    from neural_compressor_amd.torch.quantization import RTNConfig, quantize

    kw = dict(bits=4, group_size=32)
    kw.update(cfg)
    q = quantize(tiny_mixtral(dtype=torch.bfloat16), RTNConfig(**kw))
    assert not any(isinstance(m, MI355XWeightOnlyExperts) for m in q.modules())
    assert all(m.gate_up_proj.dtype == torch.bfloat16 for _, m in experts_of(q))
    ids = torch.randint(0, 128, (1, 8)).to(hip)
    with torch.no_grad():
        assert torch.isfinite(q(ids).logits.float()).all()
