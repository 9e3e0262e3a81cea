"""-m gpu: the decode route of the MX cell (inc_mx_gemv, inc_mx_gemv_multi, MXLinear.DECODE_GEMV, mx_linear_group) against the
oracle of tests/mx_cases.py on the cases of tests/mx_gemv_cases.py.

  exact     inc_mx_gemv on operands whose every partial sum is exact in fp32 in any order: bit-equal to the exact result without and
            with bias, three pairs x bf16 / fp16 x both scale rules x VCASES, nothing written around y; and bit-equal to inc_mx_gemm;
  random    within the bound of an fp32 chain in any order (the gate of the tile kernel);
  multi     every member of inc_mx_gemv_multi in its own sentinel window, bit-identical to the single launch, on random operands;
  module    MXLinear takes the GEMV up to DECODE_MAX_M rows and the tile kernel above, reads nothing back;
  group     mx_linear_group == [m(x) for m in modules] bit for bit with one quantiser call and one product launch;
  model     tiny_llama with the switch on and off.
"""

import contextlib
from unittest import mock

import pytest
import torch

from tests import mx_cases as C
from tests import mx_gemv_cases as V
from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu

Y_SENTINEL = 0x7B5A
OUT_DTYPES = [torch.bfloat16, torch.float16]
OUT_IDS = ["bf16", "fp16"]


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


def _window(hip, M, N, misaligned=False):
    """y [M, N] as a window in a sentinel-filled buffer (2 bytes past 8-byte alignment when asked) -> (buffer, lead, window)."""
    lead = 16 + (1 if misaligned else 0)
    ybits = torch.full((lead + M * N + 2 * N + 16,), Y_SENTINEL, dtype=torch.int16, device=hip)
    ywin = ybits[lead:lead + M * N]
    assert (ywin.data_ptr() % 8 != 0) == misaligned
    return ybits, lead, ywin


def _untouched_around(ybits, lead, n):
    return bool((ybits[:lead] == Y_SENTINEL).all()) and bool((ybits[lead + n:] == Y_SENTINEL).all())


def _product(hip, entry, xq, xs, afmt, wq, ws, wfmt, bias, dtype, y_misaligned=False):
    """One call of inc_mx_gemv / inc_mx_gemm (same signature) with y inside sentinels."""
    from neural_compressor_amd import _lib

    M, N, Kp = xq.shape[0], wq.shape[0], xs.shape[1] * 32
    ybits, lead, ywin = _window(hip, M, N, y_misaligned)
    rc = getattr(_lib.lib, entry)(xq.data_ptr(), xs.data_ptr(), afmt, wq.data_ptr(), ws.data_ptr(), wfmt,
                                  None if bias is None else bias.data_ptr(), ywin.data_ptr(), _code(dtype), M, N, Kp,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert _untouched_around(ybits, lead, M * N), "wrote around y"
    return ywin.cpu().view(dtype).view(M, N)


def _assert_bit_equal(y, want, what):
    a, b = y.view(torch.int16), want.view(torch.int16)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        i, j = bad[0].tolist()
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} outputs differ, first at [{i}, {j}]: got {float(y[i, j])}, "
                             f"want {float(want[i, j])}; rows {sorted(set(bad[:, 0].tolist()))[:8]} cols {sorted(set(bad[:, 1].tolist()))[:8]}")


def _exact_on_device(hip, c, rule, pair, dtype):
    afmt, wfmt = pair
    d = V.exact_operands(c, rule)
    xq = C.stored(C.encode_values(d["x"], afmt), afmt).to(hip)
    wq = C.stored(C.encode_values(d["w"], wfmt), wfmt).to(hip)
    bias = d["bias"].to(dtype).to(hip)                       # multiples of 2^-4 up to 8: exact in bf16 and fp16
    assert torch.equal(bias.cpu().double(), d["bias"])
    return d, xq, d["xs"].to(hip), wq, d["ws"].to(hip), bias


# ---- the entry point ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("c", V.VCASES, ids=V.VCASE_IDS)
def test_gemv_on_exact_operands_is_bit_equal(hip, c, pair, dtype):
    afmt, wfmt = pair
    for rule in C.SCALE_RULES:
        d, xq, xs, wq, ws, bias = _exact_on_device(hip, c, rule, pair, dtype)
        C.assert_exact_condition(d)
        y = _product(hip, "inc_mx_gemv", xq, xs, afmt, wq, ws, wfmt, None, dtype, c.y_misaligned)
        _assert_bit_equal(y, d["y"].to(dtype), f"{c.name} {rule} no bias")
        y = _product(hip, "inc_mx_gemv", xq, xs, afmt, wq, ws, wfmt, bias, dtype, c.y_misaligned)
        _assert_bit_equal(y, d["yb"].to(dtype), f"{c.name} {rule} with bias")


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_gemv_on_random_operands_is_within_the_chain_bound(hip, pair, M, dtype):
    afmt, wfmt = pair
    d = C.random_operands(M, 260, 600, afmt, wfmt, seed=11 + M)
    y = _product(hip, "inc_mx_gemv", C.stored(d["xq"], afmt).to(hip), d["xs"].to(hip), afmt, C.stored(d["wq"], wfmt).to(hip),
                 d["ws"].to(hip), wfmt, None, dtype)
    y64 = d["xd"] @ d["wd"].T
    bound = C.chain_bound(d["xd"], d["wd"], y64, dtype)
    ok = y64.abs() + bound < float(torch.finfo(dtype).max) / 2    # past the type's range the output is +-inf by specification
    assert float(ok.double().mean()) >= 0.5, "too few comparable outputs"
    ratio = ((y.double() - y64).abs() / bound)[ok]
    print(f"random {C.PAIR_IDS[C.PAIRS.index(pair)]} M={M}: worst |y - y64| / bound = {float(ratio.max()):.4f} over {int(ok.sum())} outputs")
    assert bool(torch.isfinite(y[ok].float()).all()) and float(ratio.max()) <= 1.0, f"worst ratio {float(ratio.max())}"


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
@pytest.mark.parametrize("c", V.VCASES, ids=V.VCASE_IDS)
def test_gemv_and_tile_kernel_give_the_same_bits(hip, c, pair):
    afmt, wfmt = pair
    for dtype in OUT_DTYPES:
        d, xq, xs, wq, ws, bias = _exact_on_device(hip, c, "block", pair, dtype)
        a = _product(hip, "inc_mx_gemv", xq, xs, afmt, wq, ws, wfmt, bias, dtype, c.y_misaligned)
        b = _product(hip, "inc_mx_gemm", xq, xs, afmt, wq, ws, wfmt, bias, dtype, c.y_misaligned)
        _assert_bit_equal(a, b, f"{c.name} gemv against gemm")


def test_gemv_is_deterministic(hip):
    afmt, wfmt = C.PAIRS[0]
    d = C.random_operands(16, 260, 600, afmt, wfmt, seed=3)
    args = (C.stored(d["xq"], afmt).to(hip), d["xs"].to(hip), afmt, C.stored(d["wq"], wfmt).to(hip), d["ws"].to(hip), wfmt, None,
            torch.bfloat16)
    first = _product(hip, "inc_mx_gemv", *args)
    for _ in range(3):
        _assert_bit_equal(_product(hip, "inc_mx_gemv", *args), first, "repeated call")


# ---- several weight matrices in one launch -----------------------------------------------------------------------------------------
_multi = {}


def _multi_operands(Ns, M, K, pair, seed):
    """x and the members as random operands through the oracle quantiser (one x, the members' rows cut from one weight)."""
    key = (Ns, M, K, pair, seed)
    if key not in _multi:
        afmt, wfmt = pair
        d = C.random_operands(M, sum(Ns), K, afmt, wfmt, seed)
        g = torch.Generator().manual_seed(seed + 1)
        _multi[key] = (C.stored(d["xq"], afmt), d["xs"], [w.contiguous() for w in C.stored(d["wq"], wfmt).split(list(Ns))],
                       [s.contiguous() for s in d["ws"].split(list(Ns))], [torch.randn(N, generator=g) for N in Ns])
    return _multi[key]


def _run_multi(hip, Ns, M, K, pair, dtype, without_bias=()):
    import ctypes

    from neural_compressor_amd import _lib

    afmt, wfmt = pair
    xq, xs, wqs, wss, biases = _multi_operands(Ns, M, K, pair, seed=21)
    xq, xs = xq.to(hip), xs.to(hip)
    wqs, wss = [w.to(hip) for w in wqs], [s.to(hip) for s in wss]
    biases = [None if i in without_bias else b.to(dtype).to(hip) for i, b in enumerate(biases)]
    n, Kp = len(Ns), xs.shape[1] * 32
    wins = [_window(hip, M, N) for N in Ns]
    arr = lambda ps: (ctypes.c_void_p * n)(*ps)  # noqa: E731
    rc = _lib.lib.inc_mx_gemv_multi(n, xq.data_ptr(), xs.data_ptr(), afmt, arr([w.data_ptr() for w in wqs]),
                                    arr([s.data_ptr() for s in wss]), wfmt, arr([None if b is None else b.data_ptr() for b in biases]),
                                    arr([w[2].data_ptr() for w in wins]), _code(dtype), M, (ctypes.c_int64 * n)(*Ns), Kp,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for i, (N, (ybits, lead, ywin)) in enumerate(zip(Ns, wins)):
        assert _untouched_around(ybits, lead, M * N), f"member {i}: wrote around y"
        single = _product(hip, "inc_mx_gemv", xq, xs, afmt, wqs[i], wss[i], wfmt, biases[i], dtype)
        assert bool(torch.isfinite(single.float()).any())
        _assert_bit_equal(ywin.cpu().view(dtype).view(M, N), single, f"member {i} of {Ns}")


@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_multi_members_are_the_single_launch_bit_for_bit(hip, pair, M):
    _run_multi(hip, (24, 17, 40), M, 640, pair, torch.bfloat16, without_bias=(1,))
    _run_multi(hip, (24, 17, 40), M, 640, pair, torch.float16, without_bias=(1,))


@pytest.mark.parametrize("Ns", [(1, 1030), (5, 16, 17, 1, 33, 48, 2, 20)], ids=["n2_1_1030", "n8"])
def test_multi_with_two_and_with_eight_members(hip, Ns):
    for pair in C.PAIRS:
        _run_multi(hip, Ns, 5, 384, pair, torch.bfloat16, without_bias=(0,))


def test_multi_takes_a_null_bias_array(hip):
    import ctypes

    from neural_compressor_amd import _lib

    afmt, wfmt = C.PAIRS[1]
    Ns, M = (24, 17, 40), 3
    xq, xs, wqs, wss, _ = _multi_operands(Ns, M, 640, C.PAIRS[1], seed=21)
    xq, xs, wqs, wss = xq.to(hip), xs.to(hip), [w.to(hip) for w in wqs], [s.to(hip) for s in wss]
    ys = [torch.empty(M, N, dtype=torch.bfloat16, device=hip) for N in Ns]
    arr = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])  # noqa: E731
    rc = _lib.lib.inc_mx_gemv_multi(3, xq.data_ptr(), xs.data_ptr(), afmt, arr(wqs), arr(wss), wfmt, None, arr(ys), _lib.INC_BF16, M,
                                    (ctypes.c_int64 * 3)(*Ns), 640, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for i in range(3):
        _assert_bit_equal(ys[i].cpu(), _product(hip, "inc_mx_gemv", xq, xs, afmt, wqs[i], wss[i], wfmt, None, torch.bfloat16), f"member {i}")


# ---- module ---------------------------------------------------------------------------------------------------------------------------
def _linear(K, N, bias, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(K, N, bias=bias).to(dtype)
    lin.weight.data.copy_(torch.randn(N, K, generator=g) * 0.05)
    if bias:
        lin.bias.data.copy_(torch.randn(N, generator=g))
    return lin


def _mx(lin, pair, hip):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    afmt, wfmt = pair
    return MXLinear.from_float(lin.to(hip), w_dtype=C.FMT_NAMES[wfmt], act_dtype=C.FMT_NAMES[afmt], device=hip)


@contextlib.contextmanager
def _counting(*names):
    """Counts the calls of ops.<name> made inside the block -> {name: count}."""
    from neural_compressor_amd import ops

    calls = dict.fromkeys(names, 0)

    def counted(name, f):
        def wrapped(*a, **k):
            calls[name] += 1
            return f(*a, **k)
        return wrapped

    with contextlib.ExitStack() as stack:
        for name in names:
            stack.enter_context(mock.patch.object(ops, name, counted(name, getattr(ops, name))))
        yield calls


def _switch_on(monkeypatch):
    """The route under test whatever defaults the timing left: the GEMV for up to 16 rows."""
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    monkeypatch.setattr(MXLinear, "DECODE_GEMV", True)
    monkeypatch.setattr(MXLinear, "DECODE_MAX_M", 16)
    return MXLinear


@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_module_routes_by_row_count(hip, pair, monkeypatch):
    from neural_compressor_amd import ops

    MXLinear = _switch_on(monkeypatch)
    m = _mx(_linear(200, 72, True, torch.bfloat16, 5), pair, hip)
    g = torch.Generator().manual_seed(9)
    for rows, switch in ((1, True), (5, True), (16, True), (17, True), (5, False)):
        monkeypatch.setattr(MXLinear, "DECODE_GEMV", switch)
        x = torch.randn(rows, 200, generator=g).bfloat16().to(hip)
        xq, xs = ops.mx_quant(x, m.act_fmt, m.kp)
        gemv = switch and rows <= 16
        want = (ops.mx_gemv if gemv else ops.mx_gemm)(xq, xs, m.act_fmt, m.qweight, m.w_scale, m.w_fmt, m.bias, torch.bfloat16)
        with _counting("mx_gemv", "mx_gemm") as calls:
            y = m(x)
        assert calls == {"mx_gemv": int(gemv), "mx_gemm": int(not gemv)}, (rows, switch, calls)
        _assert_bit_equal(y.cpu(), want.cpu(), f"{rows} rows, DECODE_GEMV = {switch}")


def test_shipped_defaults_are_within_what_the_kernel_takes(hip):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    assert 1 <= MXLinear.DECODE_MAX_M <= ops.MX_GEMV_MAX_M == 16
    m = _mx(_linear(256, 64, False, torch.float16, 2), C.PAIRS[0], hip)
    with _counting("mx_gemv", "mx_gemm") as calls:
        m(torch.randn(1, 256, generator=torch.Generator().manual_seed(1)).half().to(hip))
    assert calls == {"mx_gemv": int(MXLinear.DECODE_GEMV), "mx_gemm": int(not MXLinear.DECODE_GEMV)}


def test_decode_forward_and_group_read_nothing_back(hip, monkeypatch):
    from neural_compressor_amd.torch.algorithms.mx_quant import mx_linear_group

    lin = _linear(256, 64, True, torch.bfloat16, 3)
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(0)).bfloat16().to(hip)
    mods = [_mx(lin, pair, hip) for pair in C.PAIRS]
    same = [_mx(_linear(256, N, True, torch.bfloat16, N), C.PAIRS[0], hip) for N in (64, 40)]

    def no_host_read(self, *a, **k):
        raise AssertionError("host read in a forward")

    _switch_on(monkeypatch)
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, no_host_read)
    ys = [m(x) for m in mods] + mx_linear_group(x, same)
    monkeypatch.undo()
    assert [tuple(y.shape) for y in ys] == [(5, 64)] * 4 + [(5, 40)] and all(bool(torch.isfinite(y).all()) for y in ys)


# ---- group ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("pair", C.PAIRS, ids=C.PAIR_IDS)
def test_group_is_the_list_of_single_forwards(hip, pair, bias, xdtype, monkeypatch):
    from neural_compressor_amd.torch.algorithms.mx_quant import mx_linear_group

    _switch_on(monkeypatch)
    ft = torch.bfloat16 if xdtype is torch.bfloat16 else torch.float16
    qkv = [_mx(_linear(200, N, bias, ft, 30 + N), pair, hip) for N in (72, 24, 33)]
    g = torch.Generator().manual_seed(4)
    for lead, rows in (((1,), 1), ((2, 8), 16), ((17,), 17)):
        x = (torch.randn(*lead, 200, generator=g) * 1.2 + 0.3).to(xdtype).to(hip)
        want = [m(x) for m in qkv]
        with _counting("mx_quant", "mx_gemv_multi", "mx_gemv", "mx_gemm") as calls:
            got = mx_linear_group(x, qkv)
        decode = rows <= 16
        assert calls == {"mx_quant": 1, "mx_gemv_multi": int(decode), "mx_gemv": 0, "mx_gemm": 0 if decode else 3}, (rows, calls)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape == (*lead, qkv[i].out_features) and a.dtype is b.dtype is xdtype
            assert torch.equal(a.view(torch.int32 if xdtype is torch.float32 else torch.int16),
                               b.view(torch.int32 if xdtype is torch.float32 else torch.int16)), f"{rows} rows, member {i}"


def test_group_falls_back_to_the_list_of_forwards(hip, monkeypatch):
    from neural_compressor_amd.torch.algorithms.mx_quant import mx_linear_group

    MXLinear = _switch_on(monkeypatch)
    x = torch.randn(3, 256, generator=torch.Generator().manual_seed(6)).half().to(hip)
    a8w8 = [_mx(_linear(256, N, True, torch.float16, N), C.PAIRS[0], hip) for N in (40, 24)]
    a8w4 = _mx(_linear(256, 32, False, torch.float16, 7), C.PAIRS[1], hip)
    dense = _linear(256, 16, True, torch.float16, 8).to(hip)
    nine = [a8w8[i % 2] for i in range(9)]
    empty = x[:0]
    for what, mods, inp in (("mixed w_dtype", a8w8 + [a8w4], x), ("an nn.Linear", a8w8 + [dense], x), ("one member", a8w8[:1], x),
                            ("nine members", nine, x), ("an empty batch", a8w8, empty)):
        with torch.no_grad():
            want = [m(inp) for m in mods]
            with _counting("mx_gemv_multi") as calls:
                got = mx_linear_group(inp, mods)
        assert calls == {"mx_gemv_multi": 0}, what
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), what
    monkeypatch.setattr(MXLinear, "DECODE_GEMV", False)               # the switch off at decode size: exactly the single forwards
    with _counting("mx_gemv_multi", "mx_gemv", "mx_quant", "mx_gemm") as calls:
        got = mx_linear_group(x, a8w8)
    assert calls == {"mx_gemv_multi": 0, "mx_gemv": 0, "mx_quant": 2, "mx_gemm": 2}, calls
    assert all(torch.equal(a, b) for a, b in zip(got, [m(x) for m in a8w8]))


# ---- model ----------------------------------------------------------------------------------------------------------------------------
def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def test_tiny_llama_one_token_with_the_switch_on_and_off(hip, monkeypatch):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    ids = calib_ids(n=1, seq=32)[0][:, :1].to("cuda")
    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), MXQuantConfig())
    assert sum(isinstance(m, MXLinear) for m in q.modules()) == 14
    emu = tiny_llama(dtype=torch.float16).to("cuda").float()
    for name, mod in list(emu.named_modules()):
        if isinstance(mod, torch.nn.Linear) and name != "lm_head":
            setattr(emu.get_submodule(name.rsplit(".", 1)[0]), name.rsplit(".", 1)[1], C.FakeQuantLinear(mod, C.FP8, C.FP8, torch.float32))
    with torch.no_grad():
        y_emu = emu(ids).logits.float()
        _switch_on(monkeypatch)
        with _counting("mx_gemv", "mx_gemm") as calls:
            y_on = q(ids).logits.float()
        assert calls == {"mx_gemv": 14, "mx_gemm": 0}, calls
        monkeypatch.setattr(MXLinear, "DECODE_GEMV", False)
        with _counting("mx_gemv", "mx_gemm") as calls:
            y_off = q(ids).logits.float()
        assert calls == {"mx_gemv": 0, "mx_gemm": 14}, calls
    d, e_on, e_off = rel_fro(y_on, y_off), rel_fro(y_on, y_emu), rel_fro(y_off, y_emu)
    print(f"one token: rel_fro GEMV against tile kernel {d:.3e}; against the float emulation: GEMV {e_on:.3e}, tile kernel {e_off:.3e}")
    assert bool(torch.isfinite(y_on).all()) and d <= e_on and d <= e_off, (d, e_on, e_off)
