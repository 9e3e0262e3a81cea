"""-m gpu: the decode GEMV of the 1 / 2 / 3 / 5 / 6 / 7-bit modules (inc_woq_gemv_anyw) on the cases of tests/anyw_decode_cases.py.

  oracle    every case in bf16 and fp16, with and without bias, through ops.woq_gemv_anyw against the float64 product on the oracle's
            weight within the element-wise bound of tests/gemm_route_cases.py; x is a 16-byte aligned window in a NaN-filled buffer, so a
            read past row M - 1, or past column K - 1 of the last row, shows;
  guards    the same call through the C entry point with buffers the test owns: y is the first M rows of a 16-row block between sentinel
            guards, the workspace is exactly inc_woq_gemv_anyw_workspace_bytes long with a sentinel tail -- every guard byte and every row
            >= M is unchanged, the counters are zero again, and the result equals the wrapper's bit for bit;
  one-hot   rows of x with a single 1 return recover(dtype)[:, k] exactly (torch.equal): the weight is rounded once, bit for bit
            inc_woq_dequant;
  repeat    two calls are equal, and a call at another M on the same workspace right afterwards is correct (the counters re-armed);
  module    MI355XWeightOnlyLinear takes the call at decode without recover(), keeps the parent's route everywhere else;
  model     a 3-bit tiny Llama's one-token logits with the switch on against the switch off.
"""

import pytest
import torch

from tests import anyw_decode_cases as A

pytestmark = pytest.mark.gpu

Y_SENTINEL = 0x7B5A          # as bf16 / fp16 a large finite value no case produces
WS_SENTINEL = 0xA5
WS_TAIL = 4096
COUNTER_BYTES = 16384
GUARD = 256                  # elements of y in front of and behind the 16-row block (a multiple of 8: the block stays 16-byte aligned)

_dev_layers = {}
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\n[anyw decode] worst |y - ref| / tol per width (<= 1 passes)")
        for (bits, dt), (r, name) in sorted(_worst.items()):
            print(f"[anyw decode] {bits} bits {dt:5s} {r:.3f}  ({name})")


def _device_layer(hip, c):
    if c.name not in _dev_layers:
        L = A.layer_of(c)
        _dev_layers[c.name] = tuple(torch.from_numpy(L[k]).to(hip) for k in ("qweight", "scales", "qzeros"))
    return _dev_layers[c.name]


def _in_nans(hip, x):
    """x on the device as a 16-byte aligned window of a NaN-filled buffer (64 NaNs in front, 4096 behind)."""
    buf = torch.full((64 + x.numel() + 4096,), float("nan"), dtype=x.dtype, device=hip)
    view = buf[64:64 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return view


def _entry_point(hip, c, x, bias, tensors, M=None):
    """inc_woq_gemv_anyw on buffers the test owns -> (y [M, N], everything the guards need)."""
    from neural_compressor_amd import _lib

    L = _lib.lib
    M = x.shape[0] if M is None else M
    qw, sc, qz = tensors
    ybuf = torch.full((2 * GUARD + 16 * c.N,), Y_SENTINEL, dtype=torch.int16, device=hip)
    yblock = ybuf[GUARD:GUARD + 16 * c.N].view(16, c.N)
    assert yblock.data_ptr() % 16 == 0
    need = L.inc_woq_gemv_anyw_workspace_bytes(M, c.N, c.K, c.bits)
    ws = None
    if need:
        ws = torch.full((need + WS_TAIL,), WS_SENTINEL, dtype=torch.uint8, device=hip)
        ws[:COUNTER_BYTES] = 0
    return dict(L=L, M=M, ybuf=ybuf, yblock=yblock, ws=ws, need=need, x=x, bias=bias, qw=qw, sc=sc, qz=qz, c=c)


def _launch(e, x=None, M=None):
    from neural_compressor_amd import _lib

    c, x = e["c"], e["x"] if x is None else x
    M = x.shape[0] if M is None else M
    rc = e["L"].inc_woq_gemv_anyw(
        x.data_ptr(), _lib.INC_BF16 if x.dtype is torch.bfloat16 else _lib.INC_F16, e["qw"].data_ptr(), e["sc"].data_ptr(), e["qz"].data_ptr(),
        None if e["bias"] is None else e["bias"].data_ptr(), e["yblock"].data_ptr(), M, c.N, c.K, e["sc"].shape[0], c.group_size, c.bits,
        None if e["ws"] is None else e["ws"].data_ptr(), e["need"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return e["yblock"][:M].view(x.dtype).clone()


def _guards_intact(e, M):
    c = e["c"]
    sent = torch.tensor(Y_SENTINEL, dtype=torch.int16, device=e["ybuf"].device)
    assert bool((e["ybuf"][:GUARD] == sent).all()) and bool((e["ybuf"][GUARD + 16 * c.N:] == sent).all()), "a guard around y was written"
    assert bool((e["yblock"][M:] == sent).all()), "a row >= M of y was written"
    if e["ws"] is not None:
        assert bool((e["ws"][:COUNTER_BYTES] == 0).all()), "the arrival counters did not return to zero"
        assert bool((e["ws"][e["need"]:] == WS_SENTINEL).all()), "the workspace was written past inc_woq_gemv_anyw_workspace_bytes"


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", A.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", A.CASES, ids=A.CASE_IDS)
def test_case_against_the_oracle_with_guards(hip, c, dtype, with_bias):
    from neural_compressor_amd import _lib, ops

    tensors = _device_layer(hip, c)
    w64 = A.dense_weight64(A.layer_of(c), dtype)
    x, bias = A.make_x(c.M, c.K, dtype), A.make_bias(c.N, dtype)
    ref, S = A.reference(x, w64, bias if with_bias else torch.zeros(c.N, dtype=dtype))
    xd, bd = _in_nans(hip, x), bias.to(hip) if with_bias else None
    slices = _lib.lib.inc_woq_gemv_anyw_slices(c.M, c.N, c.K, c.bits)
    if c.pins.splits:
        assert slices >= 2 and c.K % A.SLICE_K[c.bits] != 0 and slices == A.slices_of(c)  # it splits, and the last slice is the short one
    else:
        assert slices == 1
    y = ops.woq_gemv_anyw(xd, *tensors, bd, c.N, c.K, c.group_size, c.bits)
    assert y.shape == (c.M, c.N) and y.dtype is dtype
    r = A.assert_elementwise(y, ref, S, c.K, dtype, f"{c.name} {dtype}")
    key = (c.bits, str(dtype).split(".")[-1])
    if r > _worst.get(key, (0.0, ""))[0]:
        _worst[key] = (r, c.name)
    e = _entry_point(hip, c, xd, bd, tensors)
    y2 = _launch(e)
    _guards_intact(e, c.M)
    assert torch.equal(y2, y), "the entry point on the test's buffers and the wrapper disagree"
    assert torch.equal(_launch(e), y), "a second call is not bit-identical"
    _guards_intact(e, c.M)


@pytest.mark.parametrize("dtype", A.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", A.CASES, ids=A.CASE_IDS)
def test_one_hot_rows_equal_recover(hip, c, dtype):
    from neural_compressor_amd import ops

    qw, sc, qz = _device_layer(hip, c)
    w = ops.woq_dequant(qw, sc, qz, None, c.N, c.K, A.group_size_eff(c), c.bits, out_dtype=dtype)  # what recover(dtype) returns
    assert torch.equal(w.cpu().double(), A.dense_weight64(A.layer_of(c), dtype))
    x, ks = A.one_hot(c, dtype)
    y = ops.woq_gemv_anyw(_in_nans(hip, x), qw, sc, qz, None, c.N, c.K, c.group_size, c.bits)
    for i, k in enumerate(ks):
        assert torch.equal(y[i], w[:, k]), f"{c.name}: row for k = {k} is not the decoded weight column"


@pytest.mark.parametrize("c", [c for c in A.CASES if c.pins.splits], ids=[c.name for c in A.CASES if c.pins.splits])
def test_another_m_on_the_same_workspace(hip, c):
    """The counters re-arm: after a call at M rows, a call at another M on the same workspace is correct at once."""
    dtype = torch.bfloat16
    tensors = _device_layer(hip, c)
    w64 = A.dense_weight64(A.layer_of(c), dtype)
    M2 = 16 if c.M != 16 else 3
    bias = A.make_bias(c.N, dtype)
    e = _entry_point(hip, c, _in_nans(hip, A.make_x(c.M, c.K, dtype)), bias.to(hip), tensors, M=max(c.M, M2))  # sized for the larger M
    _launch(e)
    x2 = A.make_x(M2, c.K, dtype)
    e["yblock"].fill_(Y_SENTINEL)
    y2 = _launch(e, x=_in_nans(hip, x2))
    ref, S = A.reference(x2, w64, bias)
    A.assert_elementwise(y2, ref, S, c.K, dtype, f"{c.name} second M = {M2}")
    _guards_intact(e, M2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------------
def _module(hip, c):
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    L = A.layer_of(c)
    m = MI355XWeightOnlyLinear(c.K, c.N, bits=c.bits, group_size=A.group_size_eff(c), zp=True, bias=True, device=hip)
    sc = torch.from_numpy(L["scales"]).t().float().contiguous()
    m.pack(torch.from_numpy(L["int_weight"]).to(torch.int32).to(hip), sc.to(hip), torch.from_numpy(L["zp"]).to(torch.int32).to(hip),
           A.make_bias(c.N, torch.float16).to(hip))
    return m, L


def _no_recover(*a, **k):
    raise AssertionError("recover() ran on the decode path")


def _parent_route(m, x):
    """What forward computed before the decode kernel existed: HIP recover() + the library GEMM."""
    b = None if m.bias is None else m.bias.to(x.dtype)
    return torch.nn.functional.linear(x, m.recover(dtype=x.dtype), b)


MODULE_CASE = next(c for c in A.CASES if c.name == "b3_long_m16")


@pytest.mark.parametrize("dtype", A.DTYPES, ids=["bf16", "fp16"])
def test_module_decodes_without_recover(hip, dtype, monkeypatch):
    from neural_compressor_amd import ops

    c = MODULE_CASE
    m, L = _module(hip, c)
    assert torch.equal(m.qweight.cpu(), torch.from_numpy(L["qweight"])) and torch.equal(m.qzeros.cpu(), torch.from_numpy(L["qzeros"]))
    assert m.ODD_WIDTH_DECODE is True and 1 <= m.ODD_WIDTH_DECODE_MAX_M <= 16
    w64 = A.dense_weight64(L, dtype)
    bias = m.bias.detach().cpu().to(dtype)
    monkeypatch.setattr(m, "recover", _no_recover)
    for M in (1, m.ODD_WIDTH_DECODE_MAX_M):
        x = A.make_x(M, c.K, dtype)
        ref, S = A.reference(x, w64, bias)
        for _ in range(2):  # the call that builds the prepared call, then the fast path at the top of forward
            y = m(x.to(hip))
            A.assert_elementwise(y, ref, S, c.K, dtype, f"module M = {M}")
            assert isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall)
        y3 = m(x.to(hip).view(1, M, c.K))
        assert y3.shape == (1, M, c.N) and torch.equal(y3.view(M, c.N), y)
    assert m._plan == "dense"


@pytest.mark.parametrize("dtype", A.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["b3_long_m16", "b5_long", "b3_g64_ragged_group"])
def test_module_one_hot_rows_equal_its_recover(hip, name, dtype):
    """m(x) on one-hot rows is m.recover(dtype)[:, k], bit for bit (no bias): the module's own recover() is the yardstick."""
    from neural_compressor_amd import ops

    c = next(c for c in A.CASES if c.name == name)
    m, _ = _module(hip, c)
    m.bias = None
    w = m.recover(dtype)
    x, ks = A.one_hot(c, dtype)
    y = m(x.to(hip))
    assert isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall)
    for i, k in enumerate(ks):
        assert torch.equal(y[i], w[:, k]), f"{name}: row for k = {k} is not recover()'s column"


def test_module_keeps_the_parent_route_elsewhere(hip):
    from neural_compressor_amd import ops

    c, dtype = MODULE_CASE, torch.bfloat16
    m, _ = _module(hip, c)
    x1 = A.make_x(1, c.K, dtype).to(hip)
    y_decode = m(x1)
    assert isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall)
    # a batch one row over the limit, right after a decode call (the fast path must not hand it over)
    xb = A.make_x(m.ODD_WIDTH_DECODE_MAX_M + 1, c.K, dtype).to(hip)
    assert torch.equal(m(xb), _parent_route(m, xb))
    assert m.__dict__.get("_call") is None
    # the switch off
    m(x1)
    assert isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall)
    m.ODD_WIDTH_DECODE = False
    assert torch.equal(m(x1), _parent_route(m, x1))
    m(x1)
    assert m.__dict__.get("_call") is None
    m.ODD_WIDTH_DECODE = True
    assert torch.equal(m(x1), y_decode)
    # fp32 in, fp32 out (computed in fp16); an empty batch
    y32 = m(x1.float())
    assert y32.dtype is torch.float32 and torch.equal(y32, m(x1.half()).float())
    assert m(x1[:0]).shape == (0, c.N)
    # the fused form keeps its meaning and takes precedence
    m(x1)
    assert isinstance(m.__dict__["_call"], ops.WoqGemvAnywCall)
    m.ODD_WIDTH_FUSED = True
    y_fused = m(x1)
    assert m._plan == "fused" and type(m.__dict__.get("_call")) is ops.WoqGemmCall
    assert torch.equal(y_fused, ops.woq_gemm(x1, m.qweight, m.scales, m.qzeros, m.bias, c.N, c.K, m.group_size, m.bits))


def test_ineligible_module_takes_the_parent_route(hip):
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    N, K, gs, bits = 21, 150, 32, 3
    g = torch.Generator().manual_seed(5)
    m = MI355XWeightOnlyLinear(K, N, bits=bits, group_size=gs, zp=True, bias=True, device=hip)
    G = -(-K // gs)
    m.pack(torch.randint(0, 1 << bits, (N, K), generator=g, dtype=torch.int32).to(hip), (torch.rand(N, G, generator=g) * 0.05 + 0.005).to(hip),
           torch.randint(0, 1 << bits, (N, G), generator=g, dtype=torch.int32).to(hip), torch.randn(N, generator=g).to(hip))
    x = torch.randn(1, K, generator=g).to(torch.bfloat16).to(hip)
    y = m(x)
    assert m._plan == "dense" and m._decode_anyw is False and m.__dict__.get("_call") is None
    assert torch.equal(y, _parent_route(m, x))


def test_repacking_in_place_rebuilds_the_call(hip):
    c, dtype = MODULE_CASE, torch.float16
    m, L = _module(hip, c)
    x = A.make_x(4, c.K, dtype).to(hip)
    y_old = m(x)
    call_old = m.__dict__["_call"]
    iw = (torch.from_numpy(L["int_weight"]).to(torch.int32) + 3) % (1 << c.bits)
    m.pack(iw.to(hip), torch.from_numpy(L["scales"]).t().float().contiguous().to(hip), torch.from_numpy(L["zp"]).to(torch.int32).to(hip),
           A.make_bias(c.N, torch.float16).to(hip))
    y_new = m(x)
    assert m.__dict__["_call"] is not None and m.__dict__["_call"] is not call_old
    assert not torch.equal(y_new, y_old)
    ref = _parent_route(m, x).float()
    assert float((y_new.float() - ref).norm() / ref.norm()) <= 2e-3
    # written through a tensor op instead: the version counter invalidates the prepared call
    call_mid = m.__dict__["_call"]
    m.qweight.copy_(torch.from_numpy(L["qweight"]).to(hip))
    assert torch.equal(m(x), y_old) and m.__dict__["_call"] is not call_mid


# ---------------------------------------------------------------------------------------------------------------------------------------
# a model
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_tiny_llama_3bit_one_token_logits(hip, monkeypatch):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear
    from neural_compressor_amd.torch.quantization import RTNConfig, quantize
    from tests.model_zoo import calib_ids, tiny_llama

    q = quantize(tiny_llama(), RTNConfig(bits=3, group_size=32, use_sym=False, use_layer_wise=False))
    mods = [m for m in q.modules() if isinstance(m, MI355XWeightOnlyLinear)]
    assert len(mods) == 14
    ids = calib_ids()[0][:, :1].to("cuda")
    with torch.no_grad():
        on = q(ids).logits.float().cpu()
        took = sum(isinstance(m.__dict__.get("_call"), ops.WoqGemvAnywCall) for m in mods)
        monkeypatch.setattr(MI355XWeightOnlyLinear, "ODD_WIDTH_DECODE", False)
        off = q(ids).logits.float().cpu()
    assert took == 14, f"only {took} of 14 modules took the decode kernel"
    assert all(m.__dict__.get("_call") is None for m in mods)
    assert torch.isfinite(on).all() and float((on - off).norm() / off.norm()) <= 2e-3
