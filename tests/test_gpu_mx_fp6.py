"""-m gpu: MXFP6 (e2m3 / e3m2) linears against the oracle of tests/mx_cases.py with the format rows of tests/mx_fp6_cases.py:
the quantiser bit for bit, both products bit for bit on operands whose sums are exact in fp32 and within the fp32 chain bound on
random ones, and MXLinear (forward, recover, save / load, the one-launch group)."""

import pytest
import torch

from tests import mx_cases as C
from tests import mx_fp6_cases as F
from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu

FMTS = pytest.mark.parametrize("fmt", [F.E2M3, F.E3M2], ids=["e2m3", "e3m2"])
PAIRS = pytest.mark.parametrize("pair", F.PAIRS, ids=F.PAIR_IDS)
OUT = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


# ---- quantiser ------------------------------------------------------------------------------------------------------------------------
def _quant_rows(fmt, dtype):
    """(3, 200): row 0 holds, one block each, every tie between neighbouring grid values (+ and -, beside the largest value, which puts
    the scale at 2^0), the grid itself with its subnormals, a saturating block, zeros, subnormals of the input type and a ragged
    block; rows 1 and 2 are Gaussian at two magnitudes.  Every constructed value has at most 6 significant bits: exact in bf16."""
    grid = C.code_table(fmt)[:32]                                      # the non-negative values, ascending
    ties = (grid[:-1] + grid[1:]) / 2
    sat, fi = float(grid[-1]), torch.finfo(dtype)
    g = torch.Generator().manual_seed(60 + fmt)
    x = torch.randn(3, 224, generator=g).double() * torch.tensor([[1.0], [2.0 ** 9], [2.0 ** -7]], dtype=torch.float64)
    r = x[0].view(7, 32)
    r[0] = torch.cat([torch.tensor([sat], dtype=torch.float64), ties])
    r[1] = -r[0]
    r[2] = grid
    r[3] = torch.cat([torch.tensor([-1.96875 * 2.0 ** C._F[fmt]["emax"]], dtype=torch.float64), grid[1:]])   # past the largest value
    r[4] = 0.0
    r[4, 5] = -0.0
    r[5] = torch.arange(-16, 16).double() * (fi.tiny * fi.eps)
    out = x[:, :200].to(dtype)
    assert torch.equal(out[0, :128].double(), x[0, :128])              # the constructed values arrive
    return out


@FMTS
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
def test_quantiser_is_bit_exact(hip, dtype, fmt):
    from neural_compressor_amd import ops

    x = _quant_rows(fmt, dtype)
    want_q, want_s = C.quant_mx(x, fmt)
    assert want_q.shape == (3, 256) and int(want_s[0, 0]) == 127 and int(want_q[0, 96] & 0x1F) == 0x1F and not bool((want_q[0, 128:160] & 0x1F).any())
    q, s = ops.mx_quant(x.to(hip), fmt)
    assert q.shape == (3, 192) and torch.equal(s.cpu(), want_s)
    got = F.unpack_fp6(q.cpu())
    assert torch.equal(got, want_q), f"{int((got != want_q).sum())} codes differ, first at {(got != want_q).nonzero()[:3].tolist()}"
    assert torch.equal(q.cpu(), F.pack_fp6(want_q))


# ---- products -------------------------------------------------------------------------------------------------------------------------
def _product(hip, entry, xq, xs, afmt, wq, ws, wfmt, bias, dtype, y_misaligned=False):
    """One call of inc_mx_gemm / inc_mx_gemv on codes as the oracle has them (unpacked), y a window inside sentinels."""
    from neural_compressor_amd import _lib

    M, N, Kp = xq.shape[0], wq.shape[0], xs.shape[1] * 32
    lead = 16 + (1 if y_misaligned else 0)
    ybits = torch.full((lead + M * N + 16,), 0x7B5A, dtype=torch.int16, device=hip)
    ywin = ybits[lead:lead + M * N]
    assert (ywin.data_ptr() % 8 != 0) == y_misaligned
    dev = [t.to(hip) for t in (F.stored(xq, afmt), xs, F.stored(wq, wfmt), ws)]
    bias = None if bias is None else bias.to(dtype).to(hip)
    rc = getattr(_lib.lib, entry)(dev[0].data_ptr(), dev[1].data_ptr(), afmt, dev[2].data_ptr(), dev[3].data_ptr(), wfmt,
                                  None if bias is None else bias.data_ptr(), ywin.data_ptr(), _code(dtype), M, N, Kp,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((ybits[:lead] == 0x7B5A).all()) and bool((ybits[lead + M * N:] == 0x7B5A).all()), "wrote around y"
    return ywin.cpu().view(dtype).view(M, N)


def _check_exact(hip, entry, d, pair, dtype, what, y_misaligned=False):
    afmt, wfmt = pair
    C.assert_exact_condition(d)
    xq, wq = C.encode_values(d["x"], afmt), C.encode_values(d["w"], wfmt)
    for bias, want in ((None, d["y"]), (d["bias"], d["yb"])):
        y = _product(hip, entry, xq, d["xs"], afmt, wq, d["ws"], wfmt, bias, dtype, y_misaligned)
        bad = (y.view(torch.int16) != want.to(dtype).view(torch.int16)).nonzero()
        assert bad.numel() == 0, f"{what} bias={bias is not None}: {bad.shape[0]} of {y.numel()} outputs differ, first {bad[:4].tolist()}"


@OUT
@PAIRS
@pytest.mark.parametrize("c", [C.GCASES[0], C.GCASES[2], C.GCASES[4]], ids=lambda c: c.name)
def test_gemm_on_exact_operands_is_bit_equal(hip, c, pair, dtype):
    assert (c.M, c.N, c.Kp) in ((1, 1, 128), (255, 257, 256), (33, 260, 640))
    _check_exact(hip, "inc_mx_gemm", C.exact_operands(c, "block"), pair, dtype, c.name, c.y_misaligned)


_gemv_master = {}


def _gemv_exact(M, N, Kp):
    """Rows and columns of ONE (16, 40, 1152) problem: the "block" scale rule depends on (row, block) only, so a slice obeys it."""
    if not _gemv_master:
        g = torch.Generator().manual_seed(606)
        fx, fw = C.SCALE_RULES["block"]
        b = torch.arange(36)[None, :]
        _gemv_master.update(x=torch.randint(-3, 4, (16, 1152), generator=g), w=torch.randint(-3, 4, (40, 1152), generator=g),
                            xs=fx(torch.arange(16)[:, None], b).to(torch.uint8), ws=fw(torch.arange(40)[:, None], b).to(torch.uint8),
                            bias=torch.randint(-128, 129, (40,), generator=g).double() / 16)
    m, nb = _gemv_master, Kp // 32
    x, w, xs, ws, bias = m["x"][:M, :Kp], m["w"][:N, :Kp], m["xs"][:M, :nb].contiguous(), m["ws"][:N, :nb].contiguous(), m["bias"][:N]
    xd = (x.double().reshape(M, nb, 32) * torch.ldexp(torch.ones(M, nb, dtype=torch.float64), xs.int() - 127)[:, :, None]).view(M, Kp)
    wd = (w.double().reshape(N, nb, 32) * torch.ldexp(torch.ones(N, nb, dtype=torch.float64), ws.int() - 127)[:, :, None]).view(N, Kp)
    y = xd @ wd.T
    return dict(x=x, w=w, xs=xs, ws=ws, bias=bias, y=y, yb=y + bias[None, :], mass=xd.abs() @ wd.abs().T)


@OUT
@PAIRS
@pytest.mark.parametrize("Kp", [128, 1152])
def test_gemv_on_exact_operands_is_bit_equal(hip, Kp, pair, dtype):
    for M in (1, 5, 16):
        for N in (1, 17, 40):
            _check_exact(hip, "inc_mx_gemv", _gemv_exact(M, N, Kp), pair, dtype, f"M={M} N={N} Kp={Kp}")


@OUT
@PAIRS
@pytest.mark.parametrize("entry,shape", [("inc_mx_gemv", (16, 40, 640)), ("inc_mx_gemm", (260, 130, 384))], ids=["gemv", "gemm"])
def test_random_operands_are_within_the_chain_bound(hip, entry, shape, pair, dtype):
    afmt, wfmt = pair
    d = C.random_operands(*shape, afmt, wfmt, seed=66)
    y = _product(hip, entry, d["xq"], d["xs"], afmt, d["wq"], d["ws"], wfmt, None, dtype)
    y64 = d["xd"] @ d["wd"].T
    _assert_within(y, y64, C.chain_bound(d["xd"], d["wd"], y64, dtype), dtype)


def _assert_within(y, y64, bound, dtype):
    """Where the exact result leaves the output type's range (fp16) the output is +-inf by specification and is not compared."""
    ok = y64.abs() + bound < float(torch.finfo(dtype).max) / 2
    ratio = ((y.double() - y64).abs() / bound)[ok]
    print(f"worst |y - y64| / bound = {float(ratio.max()):.4f} over {int(ok.sum())} of {ok.numel()} outputs")
    assert float(ok.double().mean()) >= 0.5 and bool(torch.isfinite(y[ok].float()).all()) and float(ratio.max()) <= 1.0


# ---- module ---------------------------------------------------------------------------------------------------------------------------
def _linear(K, N, seed, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(K, N, bias=True).to(dtype)
    lin.weight.data.copy_(torch.randn(N, K, generator=g) * 0.05)
    lin.bias.data.copy_(torch.randn(N, generator=g))
    return lin


@PAIRS
@pytest.mark.parametrize("rows", [3, 40])
def test_mx_linear_is_the_chained_oracle(hip, rows, pair):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    afmt, wfmt = pair
    K, N, dtype = 200, 72, torch.float16
    lin = _linear(K, N, 7)
    m = MXLinear.from_float(lin.to(hip), w_dtype=F.FMT_NAMES[wfmt], act_dtype=F.FMT_NAMES[afmt], device=hip)
    assert F.FMT_NAMES[wfmt] in m.extra_repr() and F.FMT_NAMES[afmt] in m.extra_repr()
    wq, ws = C.quant_mx(lin.weight.detach().cpu(), wfmt)
    assert torch.equal(m.qweight.cpu(), F.stored(wq, wfmt)) and torch.equal(m.w_scale.cpu(), ws)
    wd = C.dequant_mx(wq, ws, wfmt)
    assert torch.equal(m.recover(torch.float32).cpu().double(), wd[:, :K])          # every value is exact in fp32
    x = (torch.randn(rows, K, generator=torch.Generator().manual_seed(rows)) * 1.2 + 0.3).to(dtype)
    y = m(x.to(hip))
    assert y.shape == (rows, N) and y.dtype is dtype
    xd = C.dequant_mx(*C.quant_mx(x, afmt), afmt)
    b64 = m.bias.cpu().double()
    y64 = xd @ wd.T + b64[None, :]
    _assert_within(y.cpu(), y64, C.chain_bound(xd, wd, y64, dtype, b64), dtype)


def test_tiny_llama_with_fp6_mlps_through_save_load(hip, tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear, load
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    ids = calib_ids(n=1, seq=32)
    cfg = MXQuantConfig()
    cfg.set_local(".*mlp.*", MXQuantConfig(w_dtype="fp6_e2m3", act_dtype="fp6_e2m3"))
    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), cfg)
    fmts = {n: (m.w_dtype, m.act_dtype) for n, m in q.named_modules() if isinstance(m, MXLinear)}
    assert len(fmts) == 14 and all(f == (("fp6_e2m3",) * 2 if "mlp" in n else ("fp8_e4m3",) * 2) for n, f in fmts.items())
    with torch.no_grad():
        y0 = q(ids[0].to("cuda")).logits
    assert bool(torch.isfinite(y0).all())
    q.save(str(tmp_path))
    r = load(str(tmp_path), tiny_llama(dtype=torch.float16))
    assert {n: (m.w_dtype, m.act_dtype) for n, m in r.named_modules() if isinstance(m, MXLinear)} == fmts
    a, b = q.state_dict(), r.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    with torch.no_grad():
        assert torch.equal(r(ids[0].to("cuda")).logits, y0)


@PAIRS
def test_group_of_fp6_members_is_the_list_of_single_forwards(hip, pair):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear, mx_linear_group

    afmt, wfmt = pair
    mods = [MXLinear.from_float(_linear(200, N, N).to(hip), w_dtype=F.FMT_NAMES[wfmt], act_dtype=F.FMT_NAMES[afmt], device=hip)
            for N in (24, 17, 40)]
    x = torch.randn(5, 200, generator=torch.Generator().manual_seed(5)).half().to(hip)
    calls = []
    real = ops.mx_gemv_multi
    ops.mx_gemv_multi = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        ys = mx_linear_group(x, mods)
    finally:
        ops.mx_gemv_multi = real
    assert calls == [1] and all(torch.equal(y, m(x)) for y, m in zip(ys, mods))
