"""-m gpu: the dynamic per-token int8 activation cell of SmoothQuant W8A8 against the oracle of tests/w8a8_token_cases.py.

  quantiser   inc_sq_quant_act_token (csrc/sq.hip) through the C entry point with buffers the test owns: every byte of q (padding
              included) and every bit of row_scale equal the oracle, inside sentinel guards around both outputs; all input types, with
              and without in_scale, every case of QCASES (both kernels at their boundary, ragged K, an unaligned x);
  GEMM        inc_w8a8_gemm_rowscale on every route of tests/w8a8_route_cases.CASES: bit-exact without bias, within the bound of
              that file with bias, the M = 17 / M = 16 hand-over;
  module      W8A8Linear(act_quant="per_token") is the chained oracle; the accuracy condition; the model flow (prepare -> convert,
              save / load, a mixed model, alpha="auto").
"""

import pytest
import torch

from tests import w8a8_route_cases as R
from tests import w8a8_token_cases as T
from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu

Q_SENTINEL = 0x5A
S_SENTINEL = 0x7B5A7B5A
Y_SENTINEL = 0x7B5A
GUARD = 64
OUT_DTYPES = [torch.bfloat16, torch.float16]
OUT_IDS = ["bf16", "fp16"]
TOKEN_CELL = dict(act_dtype="int8", act_sym=True, act_granularity="per_token")


def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ---- quantiser ------------------------------------------------------------------------------------------------------------------------
_want = {}


def _quant_case(c, dtype, with_in_scale):
    """Inputs and oracle outputs of a case on the CPU, computed once (nothing writes to them)."""
    key = (c.name, dtype, with_in_scale)
    if key not in _want:
        x, in_scale = T.quant_inputs(c, dtype, with_in_scale)
        _want[key] = (x, in_scale, *T.quant_token(x, in_scale, c.Kp))
    return _want[key]


@pytest.mark.parametrize("with_in_scale", [False, True], ids=["plain", "in_scale"])
@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.DTYPE_IDS)
@pytest.mark.parametrize("c", T.QCASES, ids=T.QCASE_IDS)
def test_quantiser_is_bit_exact_inside_guards(hip, c, dtype, with_in_scale):
    from neural_compressor_amd import _lib

    x, in_scale, want_q, want_s = _quant_case(c, dtype, with_in_scale)
    assert (c.Kp <= T.HELD_KP) == ("two_reads" not in c.name) and c.Kp % 16 == 0 and c.Kp - c.K < 128
    if "ties" in c.specials and not with_in_scale:
        r = 1 + c.specials.index("ties")
        assert float(want_s[r]) == 1.0 and want_q[r, :len(T.TIES_Q)].tolist() == T.TIES_Q
    if "zero" in c.specials:
        r = 1 + c.specials.index("zero")
        assert float(want_s[r]) == T.EPS and not bool(want_q[r].any())
    if "last_neg" in c.specials:
        assert int(want_q[1 + c.specials.index("last_neg"), c.K - 1]) == -127
    if "first" in c.specials:
        assert int(want_q[1 + c.specials.index("first"), 0]) == 127
    n = c.M * c.K
    lead = 8 + (1 if c.unaligned else 0)                      # elements in front of x: 16-byte aligned, or one element past
    xbuf = torch.zeros(lead + n + 8, dtype=dtype, device=hip)
    xbuf[lead:lead + n] = x.reshape(-1).to(hip)
    xd = xbuf[lead:lead + n]
    assert xbuf.data_ptr() % 16 == 0 and (xd.data_ptr() % 16 != 0) == c.unaligned
    sd = None if in_scale is None else in_scale.to(hip)
    qbuf = torch.full((GUARD + c.M * c.Kp + GUARD,), Q_SENTINEL, dtype=torch.uint8, device=hip)
    sbuf = torch.full((4 + c.M + 4,), S_SENTINEL, dtype=torch.int32, device=hip)
    qwin, swin = qbuf[GUARD:GUARD + c.M * c.Kp], sbuf[4:4 + c.M]
    assert qwin.data_ptr() % 16 == 0
    rc = _lib.lib.inc_sq_quant_act_token(xd.data_ptr(), _code(dtype), c.M, c.K,
                                         c.Kp, None if sd is None else sd.data_ptr(), qwin.data_ptr(), swin.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((qbuf[:GUARD] == Q_SENTINEL).all()) and bool((qbuf[GUARD + c.M * c.Kp:] == Q_SENTINEL).all()), "wrote around xq"
    assert bool((sbuf[:4] == S_SENTINEL).all()) and bool((sbuf[4 + c.M:] == S_SENTINEL).all()), "wrote around row_scale"
    q = qwin.view(torch.int8).view(c.M, c.Kp).cpu()
    s = swin.view(torch.float32).cpu()
    T.assert_quant_equal(q, s, want_q, want_s, f"{c.name} {dtype} in_scale={with_in_scale}")


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float32: _lib.INC_F32, torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


def test_ops_wrapper_returns_the_same_as_the_entry_point(hip):
    from neural_compressor_amd import ops

    c = T.QCASES[5]
    x, in_scale, want_q, want_s = _quant_case(c, torch.float16, True)
    q, s = ops.sq_quant_act_token(x.to(hip), in_scale.to(hip), c.Kp)
    T.assert_quant_equal(q.cpu(), s.cpu(), want_q, want_s, "ops.sq_quant_act_token")


# ---- GEMM with a row scale ------------------------------------------------------------------------------------------------------------
_dev = {}


def _route_case(hip, c):
    """The case's operands on the device; the exact accumulator (torch's float64 matmul) and the fp32 factors on the CPU, where the
    expected epilogue is computed.  Built once per case, never written to."""
    if c.name not in _dev:
        cpu = R.make_inputs(c)
        d = {k: (None if v is None else v.to(hip)) for k, v in cpu.items()}
        d["rs"] = T.gemm_row_scale(c.M).to(hip)
        d["cpu"] = dict(acc=R.accumulate(d["xq"], d["wq"]).cpu(), rs=T.gemm_row_scale(c.M), alpha=cpu["alpha"], bias=cpu["bias"])
        _dev[c.name] = d
    return _dev[c.name]


def _rowscale_gemm(hip, c, d, dtype, with_bias, M=None):
    """One call of inc_w8a8_gemm_rowscale with y a window in a sentinel-filled buffer (aligned as the case asks), two guard rows after
    row M, and the workspace inc_w8a8_gemm_workspace_bytes asks for with a canary after it."""
    from neural_compressor_amd import _lib

    M = c.M if M is None else M
    lead = 16 + R.misalign(c.y_align) // 2
    ybits = torch.full((lead + M * c.N + 2 * c.N + 16,), Y_SENTINEL, dtype=torch.int16, device=hip)
    ywin = ybits[lead:lead + M * c.N]
    need = _lib.lib.inc_w8a8_gemm_workspace_bytes(M, c.N, c.K)
    ws = torch.full((need + 4096,), 0x7F, dtype=torch.uint8, device=hip)
    ws[need:] = 0xA5
    bias = d["bias"].to(dtype) if with_bias else None
    rc = _lib.lib.inc_w8a8_gemm_rowscale(d["xq"].data_ptr(), d["wq"].data_ptr(), d["rs"].data_ptr(), d["alpha"].data_ptr(),
                                         None if bias is None else bias.data_ptr(), ywin.data_ptr(), _code(dtype), M, c.N, c.K,
                                         ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((ybits[:lead] == Y_SENTINEL).all()) and bool((ybits[lead + M * c.N:] == Y_SENTINEL).all()), f"{c.name}: wrote around y"
    assert bool((ws[need:] == 0xA5).all()), f"{c.name}: wrote past the workspace"
    return ywin.cpu().view(dtype).view(M, c.N)


def _dtypes_of(c):
    return OUT_DTYPES[:1] if c.name == "full_round_plus_split_tail" else OUT_DTYPES   # the one large case: bf16 only


ROUTE_PARAMS = [pytest.param(c, dt, id=f"{c.name}-{OUT_IDS[OUT_DTYPES.index(dt)]}") for c in R.CASES for dt in _dtypes_of(c)]


@pytest.mark.parametrize("c,dtype", ROUTE_PARAMS)
def test_rowscale_gemm_without_bias_is_bit_exact(hip, c, dtype):
    assert R.plan(c.M, c.N, c.K, c.y_align) == R.expected(c), "the case no longer reaches the route it was written for"
    d = _route_case(hip, c)
    y = _rowscale_gemm(hip, c, d, dtype, with_bias=False)
    h = d["cpu"]
    R.assert_bit_equal(y, T.expect_no_bias(h["rs"], h["alpha"], h["acc"], dtype), c.name)


@pytest.mark.parametrize("c,dtype", [p for p in ROUTE_PARAMS if p.values[0].fill == "uniform"])
def test_rowscale_gemm_with_bias_is_within_one_ulp(hip, c, dtype):
    d = _route_case(hip, c)
    y = _rowscale_gemm(hip, c, d, dtype, with_bias=True)
    h = d["cpu"]
    R.assert_within_ulp(y, T.exact_with_bias(h["rs"], h["alpha"], h["acc"], h["bias"].to(dtype)), dtype, c.name)


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
def test_rowscale_gemv_hands_over_to_the_mfma_kernel(hip, dtype):
    c = R.BY_NAME["handover_m17"]
    d = _route_case(hip, c)
    y17 = _rowscale_gemm(hip, c, d, dtype, with_bias=False)
    d16 = dict(d, xq=d["xq"][:16].contiguous(), rs=d["rs"][:16].contiguous())
    assert R.plan(16, c.N, c.K)["kernel"] == "GEMV" and R.plan(17, c.N, c.K)["kernel"] == "MFMA"
    y16 = _rowscale_gemm(hip, c, d16, dtype, with_bias=False, M=16)
    R.assert_bit_equal(y16, y17[:16], "M = 16 (GEMV) against the first 16 rows of M = 17 (MFMA)")
    g16 = R.BY_NAME["gemv_m16"]
    assert (g16.N, g16.K) == (c.N, c.K)
    h = d["cpu"]
    R.assert_bit_equal(y16, T.expect_no_bias(h["rs"][:16], h["alpha"], h["acc"][:16], dtype), "M = 16")


# ---- module ---------------------------------------------------------------------------------------------------------------------------
def _linear(K, N, bias, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(K, N, bias=bias).to(dtype)
    lin.weight.data.copy_(torch.randn(N, K, generator=g) * 0.05)
    if bias:
        lin.bias.data.copy_(torch.randn(N, generator=g))
    return lin


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("K,lead,wrapped", [(200, (1, 1), True), (200, (3, 100), False), (1024, (1, 33), True)],
                         ids=["k200_1tok_gemv", "k200_300tok", "k1024_33tok_split"])
def test_per_token_linear_is_the_chained_oracle(hip, K, lead, wrapped, dtype):
    """x -> oracle quantiser -> exact integer GEMM -> the written epilogue, with the module's own qweight and w_scale (pinned elsewhere)."""
    from neural_compressor_amd.torch.algorithms.smooth_quant import SQLinearWrapper, W8A8Linear

    Tn, N = lead[0] * lead[1], 264
    g = torch.Generator().manual_seed(Tn + K)
    x = (torch.randn(*lead, K, generator=g) * 1.2 + 0.3).to(dtype)
    for bias in (False, True):
        lin = _linear(K, N, bias, dtype, K).to(hip)
        src = lin
        if wrapped:  # a smoothed layer that kept its multiplier: input_scale reaches the quantiser
            src = SQLinearWrapper(lin, (0.5 + torch.rand(K, generator=g)).to(hip), [-torch.ones(K, device=hip), torch.ones(K, device=hip)])
        m = W8A8Linear.from_float(src, device=hip, act_quant="per_token")
        assert sorted(m.state_dict()) == sorted(["qweight", "w_scale"] + (["input_scale"] if wrapped else []) + (["bias"] if bias else []))
        assert "per_token" in m.extra_repr() and (m.input_scale is not None) == wrapped
        y = m(x.to(hip))
        assert y.shape == (*lead, N) and y.dtype is dtype
        in_scale = m.input_scale.cpu() if wrapped else None
        q, s = T.quant_token(x.reshape(Tn, K), in_scale, m.kp)
        acc = R.accumulate(q, m.qweight.cpu())
        y = y.reshape(Tn, N).cpu()
        if bias:
            R.assert_within_ulp(y, T.exact_with_bias(s, m.w_scale.cpu(), acc, m.bias.cpu()), dtype, "per-token module with bias")
        else:
            R.assert_bit_equal(y, T.expect_no_bias(s, m.w_scale.cpu(), acc, dtype), "per-token module")


def test_per_token_forward_reads_nothing_back(hip, monkeypatch):
    """The static forward reads act_scale / act_zp on the host once per (re)load; the per-token forward has no such read."""
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    lin = _linear(256, 64, True, torch.bfloat16, 3).to(hip)
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(0)).bfloat16().to(hip)
    tok = W8A8Linear.from_float(lin, device=hip, act_quant="per_token")
    stat = W8A8Linear.from_float(lin, torch.full((256,), -4.0), torch.full((256,), 4.0), device=hip)

    def no_host_read(self, *a, **k):
        raise AssertionError("host read in a forward")

    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, no_host_read)
    y = tok(x)
    with pytest.raises(AssertionError, match="host read"):
        stat(x)
    monkeypatch.undo()
    assert y.shape == (5, 64) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("seed", T.ACC_SEEDS)
def test_accuracy_condition_on_the_device(hip, seed, dtype):
    """The outlier-token input through both modules: over the 63 ordinary tokens the per-token module's output error (against the float
    layer) is at most 0.1 of the static module's, whose range was calibrated on this very input."""
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    x = T.outlier_input(seed, dtype)
    lin = _linear(T.OUT_K, 128, False, dtype, 100 + seed).to(hip)
    ref = torch.nn.functional.linear(x.double(), lin.weight.detach().double().cpu())
    stat = W8A8Linear.from_float(lin, x.float().min(dim=0)[0], x.float().max(dim=0)[0], device=hip)
    tok = W8A8Linear.from_float(lin, device=hip, act_quant="per_token")
    e_static = T.rel_err(T.ordinary(stat(x.to(hip)).cpu()), T.ordinary(ref))
    e_token = T.rel_err(T.ordinary(tok(x.to(hip)).cpu()), T.ordinary(ref))
    print(f"seed {seed} {dtype}: static {e_static:.4f}  per-token {e_token:.5f}  ratio {e_token / e_static:.4f}")
    assert e_token <= T.ACC_RATIO * e_static


def _quantize(cfg, ids):
    from neural_compressor_amd.torch.quantization import convert, prepare

    model = prepare(tiny_llama(dtype=torch.float16), cfg, example_inputs=ids[0])
    for x in ids:
        model(x.to("cuda"))
    return convert(model)


def _token_config(**kw):
    from neural_compressor_amd.torch.quantization import SmoothQuantConfig

    cfg = SmoothQuantConfig(scale_sharing=True, **TOKEN_CELL, **kw)
    cfg.set_local("lm_head", SmoothQuantConfig(w_dtype="fp32"))
    return cfg


_ref = {}


def _float_logits(ids):
    if "y" not in _ref:
        with torch.no_grad():
            _ref["y"] = tiny_llama(dtype=torch.float16).to("cuda")(ids[0].to("cuda")).logits.float()
    return _ref["y"]


@pytest.mark.parametrize("folding", [False, True])
def test_tiny_llama_per_token_end_to_end_and_save_load(hip, folding, tmp_path):
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear, load

    ids = calib_ids(n=8, seq=32)
    q = _quantize(_token_config(alpha=0.5, folding=folding), ids)
    mods = {n: m for n, m in q.named_modules() if isinstance(m, W8A8Linear)}
    assert len(mods) == 14 and "lm_head" not in mods and all(m.act_quant == "per_token" for m in mods.values())
    assert all((m.input_scale is None) == folding for m in mods.values())
    assert not any(k.endswith((".alpha", ".corr", ".act_scale", ".act_zp")) for k in q.state_dict())
    with torch.no_grad():
        y0 = q(ids[0].to("cuda")).logits
    err = rel_fro(y0.float(), _float_logits(ids))
    print(f"folding={folding}: rel_fro {err:.4f}")
    assert torch.isfinite(y0).all() and err <= 0.08, err
    q.save(str(tmp_path))
    r = load(str(tmp_path), tiny_llama(dtype=torch.float16))
    back = {n: m for n, m in r.named_modules() if isinstance(m, W8A8Linear)}
    assert back.keys() == mods.keys() and all(m.act_quant == "per_token" for m in back.values())
    for n in mods:
        a, b = mods[n].state_dict(), back[n].state_dict()
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), n
    with torch.no_grad():
        assert torch.equal(r(ids[0].to("cuda")).logits, y0)


def test_mixed_model_keeps_each_layers_cell_through_save_load(hip, tmp_path):
    """q / k / v / o per-token, the MLP static, lm_head float: convert picks the cell per layer and load finds it again in the state."""
    import json
    import os

    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear, load
    from neural_compressor_amd.torch.quantization import SmoothQuantConfig

    ids = calib_ids(n=4, seq=32)
    cfg = SmoothQuantConfig(alpha=0.5, folding=False, scale_sharing=True)
    cfg.set_local("lm_head", SmoothQuantConfig(w_dtype="fp32"))
    cfg.set_local(".*self_attn.*", SmoothQuantConfig(alpha=0.5, folding=False, scale_sharing=True, **TOKEN_CELL))
    q = _quantize(cfg, ids)
    cells = {n: m.act_quant for n, m in q.named_modules() if isinstance(m, W8A8Linear)}
    assert len(cells) == 14 and all((c == "per_token") == ("self_attn" in n) for n, c in cells.items())
    assert sorted(set(cells.values())) == ["per_token", "static"]
    with torch.no_grad():
        y0 = q(ids[0].to("cuda")).logits
    assert rel_fro(y0.float(), _float_logits(ids)) <= 0.08
    q.save(str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "qconfig.json")))
    assert sorted(saved) == ["smooth_quant", "w8a8_modules"] and sorted(saved["smooth_quant"]) == ["absorb_to_layer", "alpha", "folding"]
    r = load(str(tmp_path), tiny_llama(dtype=torch.float16))
    assert {n: m.act_quant for n, m in r.named_modules() if isinstance(m, W8A8Linear)} == cells
    assert r.state_dict().keys() == q.state_dict().keys()
    with torch.no_grad():
        assert torch.equal(r(ids[0].to("cuda")).logits, y0)


def test_auto_alpha_public_flow_per_token(hip):
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    ids = calib_ids(n=8, seq=32)
    q = _quantize(_token_config(alpha="auto", folding=False, alpha_min=0.3, alpha_max=0.7, shared_criterion="mean"), ids)
    assert sum(isinstance(m, W8A8Linear) and m.act_quant == "per_token" for m in q.modules()) == 14
    assert isinstance(q.sq_info["alpha"], dict) and len(q.sq_info["alpha"]) >= 8
    with torch.no_grad():
        err = rel_fro(q(ids[0].to("cuda")).logits.float(), _float_logits(ids))
    print(f"alpha=auto: rel_fro {err:.4f}")
    assert err <= 0.08, err
