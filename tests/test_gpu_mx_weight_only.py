"""-m gpu: the weight-only MX cell (inc_mx_wo_gemv, inc_mx_wo_gemm, MXWeightOnlyLinear) against float64 on the oracle of
tests/mx_cases.py: MX weights, bf16 activations, y = x @ dequant(W)^T + bias accumulated in fp32, one rounding.

  exact        operands whose every partial sum is exact in fp32 in any order: bit-equal to the float64 result, nothing written around y;
  zero_blocks  all-zero weight blocks with scale byte 0 / 254 against large x contribute exactly nothing;
  random       within the bound of an fp32 chain in any order;
  module       MXQuantConfig(weight_only=True) through quantize, the route by row count, save / load.
"""

import pytest
import torch

from tests import mx_cases as C
from tests.model_zoo import calib_ids, tiny_llama
from tests.test_gpu_mx_gemv import _assert_bit_equal, _code, _counting, _untouched_around, _window

pytestmark = pytest.mark.gpu

FMTS = [C.FP4, C.FP8]
FMT_IDS = ["fp4", "fp8"]
OUT_DTYPES = [torch.bfloat16, torch.float16]
OUT_IDS = ["bf16", "fp16"]
# (entry, M, N, K, y misaligned, x inside a NaN-filled buffer)
CASES = [("inc_mx_wo_gemv", 1, 16, 128, False, False), ("inc_mx_wo_gemv", 5, 17, 384, False, False),
         ("inc_mx_wo_gemv", 16, 33, 1152, False, False),        # 9 tiles: more than the waves
         ("inc_mx_wo_gemv", 3, 40, 160, False, True),           # K < Kp: the tail chunks are guarded
         ("inc_mx_wo_gemm", 17, 16, 128, False, False), ("inc_mx_wo_gemm", 255, 257, 256, False, False),
         ("inc_mx_wo_gemm", 257, 255, 384, False, False), ("inc_mx_wo_gemm", 33, 260, 640, True, False),
         ("inc_mx_wo_gemm", 40, 64, 160, False, True)]
CASE_IDS = [f"{c[0][10:]}_m{c[1]}_n{c[2]}_k{c[3]}" for c in CASES]


def _product(hip, entry, x, wq, ws, wfmt, bias, dtype, K, y_misaligned=False, nan_around_x=False):
    """One call of inc_mx_wo_gemv / inc_mx_wo_gemm with y inside sentinels; x [M, K] bf16 on the CPU."""
    from neural_compressor_amd import _lib

    M, N, Kp = x.shape[0], wq.shape[0], ws.shape[1] * 32
    xbuf = torch.full((8 + M * K + 256,), float("nan") if nan_around_x else 0.0, dtype=torch.bfloat16)
    xbuf[8:8 + M * K] = x.reshape(-1)
    xbuf = xbuf.to(hip)
    ybits, lead, ywin = _window(hip, M, N, y_misaligned)
    rc = getattr(_lib.lib, entry)(xbuf[8:].data_ptr(), wq.data_ptr(), ws.data_ptr(), wfmt, None if bias is None else bias.data_ptr(),
                                  ywin.data_ptr(), _code(dtype), M, N, K, Kp, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert _untouched_around(ybits, lead, M * N), "wrote around y"
    return ywin.cpu().view(dtype).view(M, N)


_exact = {}


def _exact_operands(M, N, K):
    """Weights in {0, +-1, +-2, +-3} with the "block" rule's scale bytes, x = integers in [-3, 3] times a per-row power of two in
    2^-2 .. 2^2: every product is a multiple of 2^-4 and every partial sum stays below 2^18 -- exact in fp32 in any order."""
    if (M, N, K) not in _exact:
        g = torch.Generator().manual_seed(500 + M + N + K)
        Kp = C.padded_k(K)
        w = torch.randint(-3, 4, (N, Kp), generator=g)
        w[:, K:] = 0
        ws = C.SCALE_RULES["block"][1](torch.arange(N)[:, None], torch.arange(Kp // 32)[None, :]).to(torch.uint8)
        x = (torch.randint(-3, 4, (M, K), generator=g).double() * torch.ldexp(torch.ones(M, 1, dtype=torch.float64),
                                                                             torch.randint(-2, 3, (M, 1), generator=g)))
        bias = torch.randint(-128, 129, (N,), generator=g).double() / 16
        wd = (w.double().view(N, Kp // 32, 32) * torch.ldexp(torch.ones(N, Kp // 32, dtype=torch.float64), ws.int() - 127)[:, :, None])
        wd = wd.view(N, Kp)[:, :K]
        y = x @ wd.T
        d = dict(x=x, w=w, ws=ws, bias=bias, y=y, yb=y + bias, mass=x.abs() @ wd.abs().T, xs=ws)
        C.assert_exact_condition(d)                             # the scale bytes, the mass below 2^18, multiples of 2^-4
        assert torch.equal(x.bfloat16().double(), x)
        _exact[(M, N, K)] = d
    return _exact[(M, N, K)]


@pytest.mark.parametrize("dtype", OUT_DTYPES, ids=OUT_IDS)
@pytest.mark.parametrize("wfmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_exact_operands_are_bit_equal_to_float64(hip, case, wfmt, dtype):
    entry, M, N, K, y_mis, nan_x = case
    d = _exact_operands(M, N, K)
    wq = C.stored(C.encode_values(d["w"], wfmt), wfmt).to(hip)
    ws, x = d["ws"].to(hip), d["x"].bfloat16()
    bias = d["bias"].to(dtype).to(hip)
    y = _product(hip, entry, x, wq, ws, wfmt, None, dtype, K, y_mis, nan_x)
    _assert_bit_equal(y, d["y"].to(dtype), f"{entry} no bias")
    yb = _product(hip, entry, x, wq, ws, wfmt, bias, dtype, K, y_mis, nan_x)
    _assert_bit_equal(yb, d["yb"].to(dtype), f"{entry} with bias")
    if entry == "inc_mx_wo_gemv" and M == 16:                   # both kernels on the same operands
        _assert_bit_equal(yb, _product(hip, "inc_mx_wo_gemm", x, wq, ws, wfmt, bias, dtype, K), "gemv against gemm")


@pytest.mark.parametrize("wfmt", FMTS, ids=FMT_IDS)
def test_zero_blocks_with_extreme_scales_contribute_nothing(hip, wfmt):
    """Zero codes under scale byte 0 and 254 next to ordinary blocks, x = 2^8 there: a decode that adds exponents into a zero, or
    0 x inf, shows."""
    M, N, K = 4, 32, 256
    d = _exact_operands(M, N, K)
    w, ws, x = d["w"].clone(), d["ws"].clone(), d["x"].clone()
    rows = torch.arange(N) % 3 != 0
    w[rows, 32:64] = 0
    ws[rows, 1] = torch.where(torch.arange(N)[rows] % 2 == 0, 0, 254).to(torch.uint8)
    w[::4, 96:128] = 0
    ws[::4, 3] = 254
    x[:, 32:64] = 256.0
    wd = C.dequant_mx(C.encode_values(w, wfmt), ws, wfmt)
    y64 = x @ wd.T
    assert float((x.abs() @ wd.abs().T).max()) < 2.0 ** 18 and bool((y64 * 16 == torch.round(y64 * 16)).all())
    wq = C.stored(C.encode_values(w, wfmt), wfmt).to(hip)
    for entry in ("inc_mx_wo_gemv", "inc_mx_wo_gemm"):
        y = _product(hip, entry, x.bfloat16(), wq, ws.to(hip), wfmt, None, torch.bfloat16, K)
        _assert_bit_equal(y, y64.to(torch.bfloat16), entry)


@pytest.mark.parametrize("wfmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("shape", [("inc_mx_wo_gemv", 16, 48, 1152), ("inc_mx_wo_gemm", 300, 516, 1024)], ids=["gemv", "gemm"])
def test_random_operands_are_within_the_chain_bound(hip, shape, wfmt):
    entry, M, N, K = shape
    d = C.random_operands(1, N, K, C.FP8, wfmt, seed=31 + M)    # the weight half: Gaussian rows through the oracle quantiser
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).bfloat16()
    y = _product(hip, entry, x, C.stored(d["wq"], wfmt).to(hip), d["ws"].to(hip), wfmt, None, torch.bfloat16, K)
    y64 = x.double() @ d["wd"].T
    ratio = (y.double() - y64).abs() / C.chain_bound(x.double(), d["wd"], y64, torch.bfloat16)
    print(f"random {entry} {C.FMT_IDS[wfmt]}: worst |y - y64| / bound = {float(ratio.max()):.4f}")
    assert bool(torch.isfinite(y.float()).all()) and float(ratio.max()) <= 1.0


@pytest.mark.parametrize("w_dtype", ["fp4", "fp8_e4m3"])
def test_module_through_quantize_routes_and_survives_save_load(hip, w_dtype, tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXWeightOnlyLinear, load
    from neural_compressor_amd.torch.quantization import MXQuantConfig, quantize

    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), MXQuantConfig(w_dtype=w_dtype, act_dtype="bf16", weight_only=True))
    mods = {n: m for n, m in q.named_modules() if isinstance(m, MXWeightOnlyLinear)}
    assert len(mods) == 14 and isinstance(q.lm_head, torch.nn.Linear)
    g = torch.Generator().manual_seed(8)
    for name, m in mods.items():
        wd = m.recover(torch.float64).cpu()
        bias = None if m.bias is None else m.bias.double().cpu()
        for rows in (3, 40):
            x = torch.randn(rows, m.in_features, generator=g).half()
            with _counting("mx_wo_gemv", "mx_wo_gemm") as calls:
                y = m(x.to(hip))
            assert calls == {"mx_wo_gemv": int(rows <= 16), "mx_wo_gemm": int(rows > 16)}, (name, rows, calls)
            assert y.dtype is torch.float16 and y.shape == (rows, m.out_features)
            xd = x.bfloat16().double()
            y64 = torch.nn.functional.linear(xd, wd, bias)
            bound = C.chain_bound(xd, wd, y64, torch.float16, bias)
            assert bool(((y.double().cpu() - y64).abs() <= bound).all()), (name, rows)
    ids = calib_ids(n=1, seq=32)[0].to("cuda")
    with torch.no_grad():
        y0 = q(ids).logits
    q.save(str(tmp_path))
    r = load(str(tmp_path), tiny_llama(dtype=torch.float16))
    assert sum(isinstance(m, MXWeightOnlyLinear) for m in r.modules()) == 14
    with torch.no_grad():
        assert torch.equal(r(ids).logits, y0) and bool(torch.isfinite(y0).all())
