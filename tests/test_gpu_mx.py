"""-m gpu: the MX (MXFP8 / MXFP4) cell against the oracle of tests/mx_cases.py.

  quantiser   inc_mx_quant (csrc/mx.hip) through the C entry point with buffers the test owns: every code byte (padding included) and
              every scale byte equal the oracle, inside sentinel guards around both outputs; three input types x two formats x QCASES;
  GEMM        inc_mx_gemm (csrc/gemm_mx.hip) on operands whose every partial sum is exact in fp32 in any order: bit-equal to the exact
              result without and with bias, for the three format pairs x GCASES x bf16 / fp16 x two scale rules, nothing written
              around y; on random operands within the bound of an fp32 accumulation chain in any order;
  module      MXLinear is the chained oracle within that bound, its buffers are the oracle's byte for byte, recover() is dequant_mx,
              the forward reads nothing back;
  model       tiny_llama through quantize and prepare / convert, against the float emulation, save / load, a mixed model.
"""

import json
import os

import pytest
import torch

from tests import mx_cases as C
from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu

Q_SENTINEL, S_SENTINEL, Y_SENTINEL = 0x5A, 0xC3, 0x7B5A
GUARD = 64
OUT_DTYPES = [torch.bfloat16, torch.float16]
OUT_IDS = ["bf16", "fp16"]


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float32: _lib.INC_F32, torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ---- quantiser ------------------------------------------------------------------------------------------------------------------------
_want = {}


def _quant_case(c, dtype, fmt):
    key = (c.name, dtype, fmt)
    if key not in _want:
        x = C.quant_inputs(c, dtype, fmt)
        q, s = C.quant_mx(x, fmt)
        _want[key] = (x, C.stored(q, fmt), s)
    return _want[key]


@pytest.mark.parametrize("fmt", [C.FP8, C.FP4], ids=["fp8", "fp4"])
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("c", C.QCASES, ids=C.QCASE_IDS)
def test_quantiser_is_bit_exact_inside_guards(hip, c, dtype, fmt):
    from neural_compressor_amd import _lib

    x, want_q, want_s = _quant_case(c, dtype, fmt)
    Kp = C.padded_k(c.K)
    n = c.M * c.K
    lead = 8 + (1 if c.unaligned else 0)                      # elements in front of x: 16-byte aligned, or one element past
    xbuf = torch.zeros(lead + n + 8, dtype=dtype, device=hip)
    xbuf[lead:lead + n] = x.reshape(-1).to(hip)
    xd = xbuf[lead:lead + n]
    assert xbuf.data_ptr() % 16 == 0 and (xd.data_ptr() % 16 != 0) == c.unaligned
    assert torch.equal(xd.cpu().view(torch.int16 if dtype is not torch.float32 else torch.int32),
                       x.reshape(-1).view(torch.int16 if dtype is not torch.float32 else torch.int32))   # -0.0 and subnormals arrive
    nq, ns = want_q.numel(), want_s.numel()
    qbuf = torch.full((GUARD + nq + GUARD,), Q_SENTINEL, dtype=torch.uint8, device=hip)
    sbuf = torch.full((GUARD + ns + GUARD,), S_SENTINEL, dtype=torch.uint8, device=hip)
    qwin, swin = qbuf[GUARD:GUARD + nq], sbuf[GUARD:GUARD + ns]
    assert qwin.data_ptr() % 16 == 0
    rc = _lib.lib.inc_mx_quant(xd.data_ptr(), _code(dtype), c.M, c.K, Kp, fmt, qwin.data_ptr(), swin.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((qbuf[:GUARD] == Q_SENTINEL).all()) and bool((qbuf[GUARD + nq:] == Q_SENTINEL).all()), "wrote around the codes"
    assert bool((sbuf[:GUARD] == S_SENTINEL).all()) and bool((sbuf[GUARD + ns:] == S_SENTINEL).all()), "wrote around the scales"
    s = swin.cpu().view(want_s.shape)
    q = qwin.cpu().view(want_q.shape)
    assert torch.equal(s, want_s), f"{c.name}: {int((s != want_s).sum())} scale bytes differ, first at {(s != want_s).nonzero()[:3].tolist()}"
    assert torch.equal(q, want_q), f"{c.name}: {int((q != want_q).sum())} code bytes differ, first at {(q != want_q).nonzero()[:3].tolist()}"


def test_ops_wrapper_returns_the_same_as_the_entry_point(hip):
    from neural_compressor_amd import ops

    c = C.QCASES[2]
    for fmt in (C.FP8, C.FP4):
        x, want_q, want_s = _quant_case(c, torch.float16, fmt)
        q, s = ops.mx_quant(x.to(hip), fmt)
        assert torch.equal(q.cpu(), want_q) and torch.equal(s.cpu(), want_s)


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------------
def _mx_gemm(hip, xq, xs, afmt, wq, ws, wfmt, bias, dtype, y_misaligned=False):
    """One call of inc_mx_gemm with y a window in a sentinel-filled buffer (2 bytes past 8-byte alignment when asked)."""
    from neural_compressor_amd import _lib

    M, N, Kp = xq.shape[0], wq.shape[0], xs.shape[1] * 32
    lead = 16 + (1 if y_misaligned else 0)
    ybits = torch.full((lead + M * N + 2 * N + 16,), Y_SENTINEL, dtype=torch.int16, device=hip)
    ywin = ybits[lead:lead + M * N]
    assert (ywin.data_ptr() % 8 != 0) == y_misaligned
    rc = _lib.lib.inc_mx_gemm(xq.data_ptr(), xs.data_ptr(), afmt, wq.data_ptr(), ws.data_ptr(), wfmt,
                              None if bias is None else bias.data_ptr(), ywin.data_ptr(), _code(dtype), M, N, Kp,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((ybits[:lead] == Y_SENTINEL).all()) and bool((ybits[lead + M * N:] == Y_SENTINEL).all()), "wrote around y"
    return ywin.cpu().view(dtype).view(M, N)


def _assert_bit_equal(y, want, what):
    a, b = y.view(torch.int16), want.view(torch.int16)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        i, j = bad[0].tolist()
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} outputs differ, first at [{i}, {j}]: got {float(y[i, j])}, "
                             f"want {float(want[i, j])}; rows {sorted(set(bad[:, 0].tolist()))[:8]} cols {sorted(set(bad[:, 1].tolist()))[:8]}")


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("c", C.GCASES, ids=C.GCASE_IDS)
def test_gemm_on_exact_operands_is_bit_equal(hip, c, pair, dtype):
    afmt, wfmt = pair
    for rule in C.SCALE_RULES:
        d = C.exact_operands(c, rule)
        C.assert_exact_condition(d)
        xq = C.stored(C.encode_values(d["x"], afmt), afmt).to(hip)
        wq = C.stored(C.encode_values(d["w"], wfmt), wfmt).to(hip)
        xs, ws = d["xs"].to(hip), d["ws"].to(hip)
        y = _mx_gemm(hip, xq, xs, afmt, wq, ws, wfmt, None, dtype, c.y_misaligned)
        _assert_bit_equal(y, d["y"].to(dtype), f"{c.name} {rule} no bias")
        bias = d["bias"].to(dtype).to(hip)                   # multiples of 2^-4 up to 8: exact in bf16 and fp16
        assert torch.equal(bias.cpu().double(), d["bias"])
        y = _mx_gemm(hip, xq, xs, afmt, wq, ws, wfmt, bias, dtype, c.y_misaligned)
        _assert_bit_equal(y, d["yb"].to(dtype), f"{c.name} {rule} with bias")


def _assert_within_chain_bound(y, y64, bound, dtype, what):
    """Where the exact result leaves the output type's range (fp16) the output is +-inf by specification and is not compared."""
    ok = y64.abs() + bound < float(torch.finfo(dtype).max) / 2
    assert float(ok.double().mean()) >= 0.5, f"{what}: too few comparable outputs"
    ratio = ((y.double() - y64).abs() / bound)[ok]
    print(f"{what}: worst |y - y64| / bound = {float(ratio.max()):.4f} over {int(ok.sum())} outputs")
    assert bool(torch.isfinite(y[ok].float()).all()) and float(ratio.max()) <= 1.0, f"{what}: worst ratio {float(ratio.max())}"


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_gemm_on_random_operands_is_within_the_chain_bound(hip, pair, dtype):
    afmt, wfmt = pair
    d = C.random_operands(300, 260, 600, afmt, wfmt, seed=5)
    y = _mx_gemm(hip, C.stored(d["xq"], afmt).to(hip), d["xs"].to(hip), afmt, C.stored(d["wq"], wfmt).to(hip), d["ws"].to(hip), wfmt,
                 None, dtype)
    y64 = d["xd"] @ d["wd"].T
    _assert_within_chain_bound(y, y64, C.chain_bound(d["xd"], d["wd"], y64, dtype), dtype, f"random {C.PAIR_IDS[C.PAIRS.index(pair)]}")


def test_gemm_rejects_what_it_does_not_take(hip):
    from neural_compressor_amd import _lib

    t = torch.zeros(4096, dtype=torch.uint8, device=hip)
    p, s = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert _lib.lib.inc_mx_gemm(p, p, C.FP4, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 128, s) == -2    # fp4 activations x fp8 weights
    assert _lib.lib.inc_mx_gemm(p, p, C.FP8, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 96, s) == -2
    assert _lib.lib.inc_mx_gemm(p, p, C.FP8, p, p, C.FP8, None, p, _lib.INC_F32, 1, 1, 128, s) == -2
    assert _lib.lib.inc_mx_gemm(p, None, C.FP8, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 128, s) == -1


# ---- module ---------------------------------------------------------------------------------------------------------------------------
def _linear(K, N, bias, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(K, N, bias=bias).to(dtype)
    lin.weight.data.copy_(torch.randn(N, K, generator=g) * 0.05)
    if bias:
        lin.bias.data.copy_(torch.randn(N, generator=g))
    return lin


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("K,lead", [(200, (1, 1)), (200, (3, 100)), (1024, (1, 33))], ids=["k200_1tok", "k200_300tok", "k1024_33tok"])
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_mx_linear_is_the_chained_oracle(hip, pair, K, lead, dtype):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    afmt, wfmt = pair
    Tn, N = lead[0] * lead[1], 264
    g = torch.Generator().manual_seed(Tn + K)
    x = (torch.randn(*lead, K, generator=g) * 1.2 + 0.3).to(dtype)
    for bias in (False, True):
        lin = _linear(K, N, bias, dtype, K)
        m = MXLinear.from_float(lin.to(hip), w_dtype=C.FMT_NAMES[wfmt], act_dtype=C.FMT_NAMES[afmt], device=hip)
        assert sorted(m.state_dict()) == sorted(["qweight", "w_scale"] + (["bias"] if bias else []))
        assert C.FMT_NAMES[wfmt] in m.extra_repr() and C.FMT_NAMES[afmt] in m.extra_repr()
        wq, ws = C.quant_mx(lin.weight.detach().cpu(), wfmt)
        assert torch.equal(m.qweight.cpu(), C.stored(wq, wfmt)) and torch.equal(m.w_scale.cpu(), ws)
        wd = C.dequant_mx(wq, ws, wfmt)
        rec = m.recover()
        assert rec.dtype is dtype and torch.equal(rec.cpu().double(), wd[:, :K].to(dtype).double())
        assert torch.equal(m.recover(torch.float32).cpu().double(), wd[:, :K])      # every value is exact in fp32
        y = m(x.to(hip))
        assert y.shape == (*lead, N) and y.dtype is dtype
        xq, xs = C.quant_mx(x.reshape(Tn, K), afmt)
        xd = C.dequant_mx(xq, xs, afmt)
        b64 = m.bias.cpu().double() if bias else None
        y64 = xd @ wd.T + (b64[None, :] if bias else 0.0)
        bound = C.chain_bound(xd, wd, y64, dtype, b64)
        _assert_within_chain_bound(y.reshape(Tn, N).cpu(), y64, bound, dtype, f"module {C.PAIR_IDS[C.PAIRS.index(pair)]} bias={bias}")


def test_mx_forward_reads_nothing_back(hip, monkeypatch):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    lin = _linear(256, 64, True, torch.bfloat16, 3).to(hip)
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(0)).bfloat16().to(hip)
    mods = [MXLinear.from_float(lin, w_dtype=C.FMT_NAMES[w], act_dtype=C.FMT_NAMES[a], device=hip) for a, w in C.PAIRS]

    def no_host_read(self, *a, **k):
        raise AssertionError("host read in a forward")

    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, no_host_read)
    ys = [m(x) for m in mods]
    monkeypatch.undo()
    assert all(y.shape == (5, 64) and bool(torch.isfinite(y).all()) for y in ys)


# ---- model flow -----------------------------------------------------------------------------------------------------------------------
_ref = {}


def _float_logits(ids):
    if "y" not in _ref:
        with torch.no_grad():
            _ref["y"] = tiny_llama(dtype=torch.float16).to("cuda")(ids[0].to("cuda")).logits.float()
    return _ref["y"]


def _emulated_logits(ids, pick):
    """The float model with every selected Linear replaced by the fake-quant linear, run on the device in fp32."""
    model = tiny_llama(dtype=torch.float16).to("cuda").float()
    for name, mod in list(model.named_modules()):
        if isinstance(mod, torch.nn.Linear) and name != "lm_head":
            w_fmt, a_fmt = pick(name)
            parent = model.get_submodule(name.rsplit(".", 1)[0])
            setattr(parent, name.rsplit(".", 1)[1], C.FakeQuantLinear(mod, w_fmt, a_fmt, torch.float32))
    with torch.no_grad():
        return model(ids[0].to("cuda")).logits.float()


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_tiny_llama_end_to_end_and_save_load(hip, pair, tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear, load
    from neural_compressor_amd.torch.quantization import MXQuantConfig, convert, prepare, quantize

    afmt, wfmt = pair
    ids = calib_ids(n=1, seq=32)
    cfg = dict(w_dtype=C.FMT_NAMES[wfmt], act_dtype=C.FMT_NAMES[afmt])
    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), MXQuantConfig(**cfg))
    q2 = convert(prepare(tiny_llama(dtype=torch.float16).to("cuda"), MXQuantConfig(**cfg)))
    a, b = q.state_dict(), q2.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    mods = {n: m for n, m in q.named_modules() if isinstance(m, MXLinear)}
    assert len(mods) == 14 and "lm_head" not in mods and isinstance(q.lm_head, torch.nn.Linear)
    assert all((m.w_dtype, m.act_dtype) == (C.FMT_NAMES[wfmt], C.FMT_NAMES[afmt]) for m in mods.values())
    with torch.no_grad():
        y0 = q(ids[0].to("cuda")).logits
    ref = _float_logits(ids)
    err = rel_fro(y0.float(), ref)
    emu = rel_fro(_emulated_logits(ids, lambda name: (wfmt, afmt)), ref)
    print(f"{C.PAIR_IDS[C.PAIRS.index(pair)]}: rel_fro native {err:.5f}  float emulation {emu:.5f}")
    assert bool(torch.isfinite(y0).all()) and err <= 1.25 * emu, (err, emu)
    q.save(str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "qconfig.json")))
    assert sorted(saved) == ["mx_modules", "mx_quant"] and len(saved["mx_modules"]) == 14
    r = load(str(tmp_path), tiny_llama(dtype=torch.float16))
    ra = r.state_dict()
    assert ra.keys() == a.keys() and all(torch.equal(ra[k], a[k]) for k in a)
    with torch.no_grad():
        assert torch.equal(r(ids[0].to("cuda")).logits, y0)


def test_mixed_model_keeps_each_layers_formats_through_save_load(hip, tmp_path):
    """self_attn with fp4 weights, the MLP fp8, lm_head float."""
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear, load
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    ids = calib_ids(n=1, seq=32)
    cfg = MXQuantConfig()
    cfg.set_local(".*self_attn.*", MXQuantConfig(w_dtype="fp4", act_dtype="fp8_e4m3"))
    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), cfg)
    fmts = {n: (m.w_dtype, m.act_dtype) for n, m in q.named_modules() if isinstance(m, MXLinear)}
    assert len(fmts) == 14 and all(f == (("fp4" if "self_attn" in n else "fp8_e4m3"), "fp8_e4m3") for n, f in fmts.items())
    with torch.no_grad():
        y0 = q(ids[0].to("cuda")).logits
    ref = _float_logits(ids)
    err = rel_fro(y0.float(), ref)
    emu = rel_fro(_emulated_logits(ids, lambda name: (C.FP4 if "self_attn" in name else C.FP8, C.FP8)), ref)
    print(f"mixed: rel_fro native {err:.5f}  float emulation {emu:.5f}")
    assert bool(torch.isfinite(y0).all()) and err <= 1.25 * emu
    q.save(str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "qconfig.json")))
    assert {n: tuple(v) for n, v in saved["mx_modules"].items()} == fmts
    r = load(str(tmp_path), tiny_llama(dtype=torch.float16))
    assert {n: (m.w_dtype, m.act_dtype) for n, m in r.named_modules() if isinstance(m, MXLinear)} == fmts
    a, b = q.state_dict(), r.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    with torch.no_grad():
        assert torch.equal(r(ids[0].to("cuda")).logits, y0)
