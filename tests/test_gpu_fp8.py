"""GPU: the FP8 per-token / per-channel cell (inc_fp8_quant_rows, inc_fp8_gemm, inc_fp8_gemv, FP8Linear, FP8Config) against the CPU
oracle of tests/fp8_cases.py.

  quantiser   bit-exact codes and scales: every K path, three input types, in_scale, an unaligned input, zero rows, the ties row,
              sentinels behind both outputs.
  products    exact operands (integers, power-of-two factors) bit-equal to the float64 result rounded once; random e4m3 codes
              bit-identical to the pinned MX kernels at scale bytes 127; Gaussian factors within one output ulp + 2^-8 of the mass.
  module      FP8Linear is the chain of the three ops bit for bit, both routes, recover, save / load, tiny_llama end to end.
"""

import json
import os

import pytest
import torch

from tests import fp8_cases as C
from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu

E4M3 = 0  # INC_MX_FP8_E4M3


def _check_quant(ops, x, in_scale=None):
    q, s = ops.fp8_quant_rows(x.cuda(), None if in_scale is None else in_scale.cuda())
    wq, ws = C.quant_rows(x, in_scale)
    assert q.shape == wq.shape and q.dtype == torch.uint8 and s.dtype == torch.float32
    assert torch.equal(s.cpu(), ws), "row_scale differs"
    assert torch.equal(q.cpu(), wq), f"{int((q.cpu() != wq).sum())} codes differ"
    return q, s


# ---- quantiser ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("K", C.QUANT_KS)
def test_quantiser_is_bit_exact(hip, K, dtype):
    from neural_compressor_amd import ops

    for M in C.QUANT_MS:
        x = C.quant_input(M, K, dtype)
        _check_quant(ops, x)
        _check_quant(ops, x, C.in_scale_for(K))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
def test_quantiser_rereads_a_long_row(hip, dtype):
    from neural_compressor_amd import ops

    assert C.padded_k(C.REREAD_K) > C.HELD_MAX
    x = C.quant_input(1, C.REREAD_K, dtype)
    _check_quant(ops, x)
    _check_quant(ops, x, C.in_scale_for(C.REREAD_K))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("K", [128, 600])
def test_quantiser_takes_an_unaligned_input(hip, K, dtype):
    """x one element off a 16-byte boundary: the element-load path."""
    from neural_compressor_amd import ops

    x = C.quant_input(3, K, dtype)
    buf = torch.empty(3 * K + 1, dtype=dtype, device="cuda")
    view = buf[1:].view(3, K)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    q, s = ops.fp8_quant_rows(view)
    wq, ws = C.quant_rows(x)
    assert torch.equal(q.cpu(), wq) and torch.equal(s.cpu(), ws)


def test_quantiser_zero_rows_and_ties(hip):
    from neural_compressor_amd import ops

    x = C.quant_input(3, 600, torch.float32).clone()
    x[1] = 0.0
    x[1, 7] = -0.0
    q, s = _check_quant(ops, x)
    assert float(s[1]) == 2.0 ** -60 and q[1].cpu().tolist() == [0x80 if k == 7 else 0 for k in range(640)]
    table = C.code_table(C.FP8)
    for j in (-20, -3, 0, 7):
        row, to = C.ties_row(j, K=200)
        for dtype in C.DTYPES:
            if bool((row.to(dtype).float() == row).all()):       # the type holds the row exactly (fp16 does not at 2^-20 or 448 * 2^7)
                q, s = _check_quant(ops, row[None, :].to(dtype))
                assert float(s[0]) == 2.0 ** j
                assert torch.equal(table[q[0, :200].cpu().long()], to), f"a tie went to the wrong neighbour at 2^{j}"
    assert bool((C.ties_row(0)[0].to(torch.bfloat16).float() == C.ties_row(0)[0]).all())


@pytest.mark.parametrize("K", [17, 600, C.REREAD_K])
def test_quantiser_writes_nothing_past_its_outputs(hip, K):
    from neural_compressor_amd import _lib, ops

    M, Kp = (1 if K == C.REREAD_K else 3), C.padded_k(K)
    x = C.quant_input(M, K, torch.bfloat16)
    codes = torch.full((M * Kp + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    scale = torch.full((M + 64,), -7.0, dtype=torch.float32, device="cuda")
    xd = x.cuda()
    rc = _lib.lib.inc_fp8_quant_rows(xd.data_ptr(), ops.dtype_code(xd.dtype), M, K, Kp, None, codes.data_ptr(), scale.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    wq, ws = C.quant_rows(x, None, Kp)
    assert torch.equal(codes[: M * Kp].view(M, Kp).cpu(), wq) and torch.equal(scale[:M].cpu(), ws)
    assert bool((codes[M * Kp:] == 0xA5).all()) and bool((scale[M:] == -7.0).all())


# ---- products on exact operands -------------------------------------------------------------------------------------------------------
def _exact_check(product, d, rows, out_dtype, with_bias):
    xq, rs = d["xq"][:rows].cuda(), d["rs"][:rows].cuda()
    bias = d["bias"].to(out_dtype).cuda() if with_bias else None
    assert not with_bias or bool((d["bias"].to(out_dtype).double() == d["bias"]).all())
    y = product(xq, rs, d["wq"].cuda(), d["al"].cuda(), bias, out_dtype)
    want = (d["yb"] if with_bias else d["y"])[:rows].to(out_dtype)
    assert y.dtype == out_dtype and torch.equal(y.cpu().view(torch.int16), want.view(torch.int16)), (
        f"{int((y.cpu() != want).sum())} of {want.numel()} outputs differ from the exact result")


@pytest.mark.parametrize("Kp", C.GEMM_KPS)
@pytest.mark.parametrize("shape", C.GEMM_SHAPES, ids=lambda s: f"m{s[0]}n{s[1]}")
def test_gemm_on_exact_operands_is_bit_equal(hip, shape, Kp):
    from neural_compressor_amd import ops

    d = C.exact_case(shape[0], shape[1], Kp)
    for out_dtype in C.OUT_DTYPES:
        for with_bias in (False, True):
            _exact_check(ops.fp8_gemm, d, shape[0], out_dtype, with_bias)


@pytest.mark.parametrize("tiles", C.GEMV_TILES)
@pytest.mark.parametrize("N", C.GEMV_NS)
def test_gemv_on_exact_operands_is_bit_equal(hip, N, tiles):
    from neural_compressor_amd import ops

    d = C.exact_case(16, N, 128 * tiles)
    for M in C.GEMV_MS:
        for out_dtype in C.OUT_DTYPES:
            for with_bias in (False, True):
                _exact_check(ops.fp8_gemv, d, M, out_dtype, with_bias)


def test_gemm_serves_decode_rows_like_the_gemv(hip):
    """The tile kernel on 1 .. 16 rows (what DECODE_GEMV = False runs) gives the GEMV's bits on exact operands."""
    from neural_compressor_amd import ops

    d = C.exact_case(16, 260, 128 * 9)
    for M in C.GEMV_MS:
        _exact_check(ops.fp8_gemm, d, M, torch.bfloat16, True)


# ---- cross-check against the pinned MX kernels ---------------------------------------------------------------------------------------------
def _cross(fp8_product, mx_product, M, N, Kp, seed):
    d = C.random_codes(M, N, Kp, seed)
    xq, wq = d["xq"].cuda(), d["wq"].cuda()
    ones_m, ones_n = torch.ones(M, device="cuda"), torch.ones(N, device="cuda")
    xs = torch.full((M, Kp // 32), 127, dtype=torch.uint8, device="cuda")
    ws = torch.full((N, Kp // 32), 127, dtype=torch.uint8, device="cuda")
    bias = C.gaussian_factors(M, N, seed)[2]
    for out_dtype in C.OUT_DTYPES:
        for b in (None, bias.to(out_dtype).cuda()):
            y = fp8_product(xq, ones_m, wq, ones_n, b, out_dtype)
            ref = mx_product(xq, xs, E4M3, wq, ws, E4M3, b, out_dtype)
            assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), f"{int((y != ref).sum())} outputs differ from the MX kernel"
    yb = fp8_product(xq, ones_m, wq, ones_n, None, torch.bfloat16).double().cpu()
    assert bool(torch.isfinite(yb).all()) and bool(((yb - d["acc"]).abs() <= C.ulp_of(d["acc"], torch.bfloat16) + 2.0 ** -8 * d["mass"]).all())


def test_gemm_is_the_mx_gemm_at_unit_scales(hip):
    from neural_compressor_amd import ops

    _cross(ops.fp8_gemm, ops.mx_gemm, *C.CROSS_GEMM, seed=31)


def test_gemv_is_the_mx_gemv_at_unit_scales(hip):
    from neural_compressor_amd import ops

    _cross(ops.fp8_gemv, ops.mx_gemv, *C.CROSS_GEMV, seed=32)


# ---- non-power-of-two factors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["gemm", "gemv"])
def test_products_with_gaussian_factors_are_within_the_allowance(hip, route):
    """|y - ((s a) acc64 + bias)| <= ulp(y) + 2^-8 * s a * sum |a_k b_k|: one rounding to the output type plus the project's allowance for
    the instruction's internal sum ("MX experts numerics").  Prints the worst ratio (a record, not a threshold)."""
    from neural_compressor_amd import ops

    (M, N, Kp), product = (C.CROSS_GEMM, ops.fp8_gemm) if route == "gemm" else (C.CROSS_GEMV, ops.fp8_gemv)
    d = C.random_codes(M, N, Kp, 31 if route == "gemm" else 32)
    rs, al, bias = C.gaussian_factors(M, N, 77)
    f = rs.double()[:, None] * al.double()[None, :]
    worst = 0.0
    for out_dtype in C.OUT_DTYPES:
        for b in (None, bias.to(out_dtype)):
            y = product(d["xq"].cuda(), rs.cuda(), d["wq"].cuda(), al.cuda(), None if b is None else b.cuda(), out_dtype).double().cpu()
            want = f * d["acc"] + (0.0 if b is None else b.double()[None, :])
            allow = C.ulp_of(want, out_dtype) + 2.0 ** -8 * f * d["mass"]
            assert bool(torch.isfinite(y).all())
            ratio = float(((y - want).abs() / allow).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (route, out_dtype, ratio)
    print(f"fp8 {route} {M}x{N}x{Kp}, gaussian factors: worst |err| / allowance = {worst:.4f}")


def test_products_reject_what_they_do_not_take(hip):
    from neural_compressor_amd import ops

    d = C.exact_case(17, 7, 128)
    args = (d["xq"].cuda(), d["rs"].cuda(), d["wq"].cuda(), d["al"].cuda())
    with pytest.raises(RuntimeError, match="inc_fp8_gemv"):
        ops.fp8_gemv(*args, None, torch.bfloat16)            # 17 rows
    with pytest.raises(TypeError):
        ops.fp8_gemm(*args, None, torch.float64)


# ---- module ---------------------------------------------------------------------------------------------------------------------------
_lin = {}


def _linear(dtype):
    if dtype not in _lin:
        g = torch.Generator().manual_seed(11)
        lin = torch.nn.Linear(600, 260, bias=True)
        lin.weight.data.copy_(torch.randn(260, 600, generator=g) * 0.05)
        lin.bias.data.copy_(torch.randn(260, generator=g))
        _lin[dtype] = lin.to(dtype)
    return _lin[dtype]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows", [1, 16, 17, 300])
def test_fp8_linear_is_the_chain_of_its_ops(hip, rows, dtype):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear

    lin = _linear(torch.bfloat16 if dtype == torch.bfloat16 else torch.float32)
    m = FP8Linear.from_float(lin, device="cuda")
    ft = torch.bfloat16 if dtype == torch.bfloat16 else torch.float16
    assert m.float_type == ft and m.qweight.shape == (260, 640) and m.w_scale.shape == (260,) and m.bias.dtype == ft
    wq, ws = C.quant_rows(lin.weight.detach())
    assert torch.equal(m.qweight.cpu(), wq) and torch.equal(m.w_scale.cpu(), ws)
    x = (torch.randn(rows, 600, generator=torch.Generator().manual_seed(rows)) * 2).to(dtype)
    y = m(x.cuda())
    xq, xs = ops.fp8_quant_rows(x.cuda(), None, 640)
    assert torch.equal(xq.cpu(), C.quant_rows(x)[0])
    chain = (ops.fp8_gemv if rows <= 16 else ops.fp8_gemm)(xq, xs, m.qweight, m.w_scale, m.bias, ft)
    assert y.dtype == dtype and y.shape == (rows, 260) and torch.equal(y, chain.to(dtype))
    try:
        FP8Linear.DECODE_GEMV = False
        y_tile = m(x.cuda())
    finally:
        FP8Linear.DECODE_GEMV = True
    assert torch.equal(y_tile, ops.fp8_gemm(xq, xs, m.qweight, m.w_scale, m.bias, ft).to(dtype))
    # against the float64 product of the dequantised operands: one output ulp + the instruction's allowance (as above)
    want = C.dequant(xq.cpu(), xs.cpu()) @ C.dequant(wq, ws).T + m.bias.double().cpu()[None, :]
    mass = C.dequant(xq.cpu(), xs.cpu()).abs() @ C.dequant(wq, ws).abs().T
    for got in (y, y_tile):
        assert bool(((got.double().cpu() - want).abs() <= C.ulp_of(want, ft) + 2.0 ** -8 * mass).all())
    assert m(x.cuda()[:0]).shape == (0, 260) and m(x.cuda().view(1, rows, 600)).shape == (1, rows, 260)
    assert "fp8_config=E4M3" in m.extra_repr() and "in_features=600" in m.extra_repr()


def test_both_routes_are_bit_equal_on_an_exact_module(hip):
    """Integer weights and activations whose row maxima make every scale a power of two: the two routes must agree bit for bit."""
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear

    g = torch.Generator().manual_seed(5)
    lin = torch.nn.Linear(600, 260, bias=True).to(torch.bfloat16)
    w = torch.randint(-3, 4, (260, 600), generator=g).float()
    w[:, 0] = 3.5                                              # row max 3.5 = 448 * 2^-7: scale 2^-7, the integers land on exact codes
    lin.weight.data.copy_(w)
    lin.bias.data.copy_(torch.randint(-64, 65, (260,), generator=g).float() / 8)
    m = FP8Linear.from_float(lin, device="cuda")
    assert bool((m.w_scale == 2.0 ** -7).all()) and torch.equal(m.recover(torch.float32).cpu(), w)
    x = torch.randint(-3, 4, (16, 600), generator=g).float()
    x[:, 1] = 3.5
    want = (x.double() @ w.double().T + lin.bias.double()[None, :]).to(torch.bfloat16)
    y_gemv = m(x.to(torch.bfloat16).cuda())
    try:
        FP8Linear.DECODE_GEMV = False
        y_tile = m(x.to(torch.bfloat16).cuda())
    finally:
        FP8Linear.DECODE_GEMV = True
    assert torch.equal(y_gemv, y_tile) and torch.equal(y_gemv.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_recover_is_the_oracle_dequantisation(hip, dtype):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear

    lin = _linear(torch.bfloat16)
    m = FP8Linear.from_float(lin, device="cuda")
    wq, ws = C.quant_rows(lin.weight.detach())
    want = C.dequant(wq, ws)[:, :600].float().to(dtype)        # table value * scale: one fp32 rounding, then the cast
    assert torch.equal(m.recover(dtype).cpu(), want) and m.recover().dtype == torch.bfloat16


def test_module_save_load_is_bit_identical(hip, tmp_path):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear, load, save

    net = torch.nn.Sequential(_linear(torch.bfloat16), torch.nn.ReLU(), torch.nn.Linear(260, 24, bias=False).to(torch.bfloat16))
    float_arch = torch.nn.Sequential(torch.nn.Linear(600, 260), torch.nn.ReLU(), torch.nn.Linear(260, 24, bias=False)).to(torch.bfloat16)
    import copy

    q = copy.deepcopy(net).cuda()
    q[0], q[2] = FP8Linear.from_float(q[0]), FP8Linear.from_float(q[2])
    x = torch.randn(20, 600, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    y0 = q(x)
    save(q, str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "qconfig.json")))
    assert saved["fp8_modules"] == ["0", "2"]
    r = load(str(tmp_path), float_arch)
    assert isinstance(r[0], FP8Linear) and isinstance(r[2], FP8Linear) and r[2].bias is None
    a, b = q.state_dict(), r.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(r(x), y0)


def rel_fro(a, b):
    return float((a - b).norm() / b.norm())


def test_tiny_llama_end_to_end_and_save_load(hip, tmp_path):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear, load
    from neural_compressor_amd.torch.quantization import FP8Config, convert, prepare, quantize

    ids = calib_ids(n=1, seq=32)
    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), FP8Config())
    q2 = convert(prepare(tiny_llama(dtype=torch.float16).to("cuda"), FP8Config()))
    a, b = q.state_dict(), q2.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    mods = {n: m for n, m in q.named_modules() if isinstance(m, FP8Linear)}
    n_linear = sum(isinstance(m, torch.nn.Linear) for m in tiny_llama(dtype=torch.float16).modules())
    assert len(mods) == n_linear - 1 == 14 and "lm_head" not in mods and isinstance(q.lm_head, torch.nn.Linear)
    with torch.no_grad():
        y0 = q(ids[0].to("cuda")).logits
        ref = tiny_llama(dtype=torch.float16).to("cuda")(ids[0].to("cuda")).logits.float()
        emu_model = tiny_llama(dtype=torch.float16).to("cuda").float()
        for name, mod in list(emu_model.named_modules()):
            if isinstance(mod, torch.nn.Linear) and name != "lm_head":
                parent = emu_model.get_submodule(name.rsplit(".", 1)[0])
                setattr(parent, name.rsplit(".", 1)[1], C.FakeQuantLinear(mod, torch.float32))
        emu = emu_model(ids[0].to("cuda")).logits.float()
    assert bool(torch.isfinite(y0).all())
    print(f"tiny_llama FP8 per-token: rel_fro native {rel_fro(y0.float(), ref):.5f}  float emulation {rel_fro(emu, ref):.5f}")
    q.save(str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "qconfig.json")))
    assert sorted(saved) == ["fp8_modules", "fp8_quant"] and len(saved["fp8_modules"]) == 14
    r = load(str(tmp_path), tiny_llama(dtype=torch.float16))
    ra = r.state_dict()
    assert ra.keys() == a.keys() and all(torch.equal(ra[k], a[k]) for k in a)
    with torch.no_grad():
        assert torch.equal(r(ids[0].to("cuda")).logits, y0)


def test_a_layer_opts_out_and_lm_head_opts_in(hip):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear
    from neural_compressor_amd.torch.quantization import FP8Config, quantize

    cfg = FP8Config(quant_lm_head=True)
    cfg.set_local(".*mlp.*", FP8Config(fp8_config="fp32"))
    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), cfg)
    names = [n for n, m in q.named_modules() if isinstance(m, FP8Linear)]
    assert len(names) == 9 and "lm_head" in names and all("mlp" not in n for n in names)
    with torch.no_grad():
        assert bool(torch.isfinite(q(calib_ids(n=1, seq=32)[0].to("cuda")).logits).all())
