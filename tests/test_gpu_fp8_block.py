"""GPU: the block-scaled FP8 cell (inc_fp8_quant_groups, inc_fp8_quant_blocks, inc_fp8_block_gemm, inc_fp8_block_gemv, FP8BlockLinear,
FP8Config's block pair) against the CPU oracle of tests/fp8_block_cases.py: the quantisers bit-exact, the products bit-equal to the
float64 result on exact operands and within one output ulp + 2^-8 of the mass on random codes, the module the chain of its ops."""

import pytest
import torch

from tests import fp8_block_cases as C
from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu
TABLE = C.code_table(C.FP8)


def _check_quant(ops, x, rb, xd=None):
    q, s = (ops.fp8_quant_groups if rb == 1 else ops.fp8_quant_blocks)(x.cuda() if xd is None else xd)
    wq, ws = C.quant_blocked(x, rb)
    assert q.dtype == torch.uint8 and s.dtype == torch.float32 and q.shape == wq.shape and s.shape == ws.shape
    assert torch.equal(s.cpu(), ws), "scales differ"
    assert torch.equal(q.cpu(), wq), f"{int((q.cpu() != wq).sum())} codes differ"
    return q, s


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("case", C.QUANT_CASES, ids=lambda c: f"rb{c[0]}r{c[1]}k{c[2]}")
def test_quantisers_are_bit_exact(hip, case, dtype):
    from neural_compressor_amd import ops

    rb, R, K = case
    _check_quant(ops, C.quant_input(R, K, dtype, rb), rb)


@pytest.mark.parametrize("rb", [1, 128], ids=["groups", "blocks"])
def test_quantisers_on_an_unaligned_input_zero_blocks_and_sentinels(hip, rb):
    """x one element off a 16-byte boundary (the element path); an all-zero group / block with one negative zero; sentinel bytes behind
    both outputs."""
    from neural_compressor_amd import _lib, ops

    x = C.quant_input(3, 600, torch.bfloat16, rb)
    view = torch.empty(3 * 600 + 1, dtype=torch.bfloat16, device="cuda")[1:].view(3, 600)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    _check_quant(ops, x, rb, view)
    z = C.quant_input(3, 600, torch.float32, rb).clone()
    z[:, 128:256] = 0.0
    z[1, 135] = -0.0
    q, s = _check_quant(ops, z, rb)
    assert bool((s[:, 1] == 2.0 ** -60).all()) and q[1, 128:256].cpu().tolist() == [0x80 if k == 7 else 0 for k in range(128)]
    R, K, Kp = 130, 600, 640
    x = C.quant_input(R, K, torch.bfloat16, rb)
    wq, ws = C.quant_blocked(x, rb)
    codes = torch.full((R * Kp + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    scales = torch.full((ws.numel() + 64,), -7.0, dtype=torch.float32, device="cuda")
    fn = _lib.lib.inc_fp8_quant_groups if rb == 1 else _lib.lib.inc_fp8_quant_blocks
    xd = x.cuda()
    assert fn(xd.data_ptr(), ops.dtype_code(xd.dtype), R, K, Kp, codes.data_ptr(), scales.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert torch.equal(codes[: R * Kp].view(R, Kp).cpu(), wq) and torch.equal(scales[: ws.numel()].cpu(), ws.flatten())
    assert bool((codes[R * Kp:] == 0xA5).all()) and bool((scales[ws.numel():] == -7.0).all())


def _exact_check(product, d, rows):
    for out_dtype in C.OUT_DTYPES:
        for bias, want in ((None, d["y"]), (d["bias"].to(out_dtype).cuda(), d["yb"])):
            y = product(d["xq"][:rows].cuda(), d["xs"][:rows].cuda(), d["wq"].cuda(), d["ws"].cuda(), bias, out_dtype)
            want = want[:rows].to(out_dtype)
            assert y.dtype == out_dtype and torch.equal(y.cpu().view(torch.int16), want.view(torch.int16)), (
                f"{int((y.cpu() != want).sum())} of {want.numel()} outputs differ from the exact result")


@pytest.mark.parametrize("Kp", C.GEMM_KPS)
@pytest.mark.parametrize("shape", C.GEMM_SHAPES, ids=lambda s: f"m{s[0]}n{s[1]}")
def test_gemm_on_exact_operands_is_bit_equal(hip, shape, Kp):
    from neural_compressor_amd import ops

    _exact_check(ops.fp8_block_gemm, C.exact_case(shape[0], shape[1], Kp), shape[0])


@pytest.mark.parametrize("tiles", C.GEMV_TILES)
@pytest.mark.parametrize("N", C.GEMV_NS)
def test_gemv_on_exact_operands_is_bit_equal_and_the_gemm_agrees(hip, N, tiles):
    from neural_compressor_amd import ops

    d = C.exact_case(16, N, 128 * tiles)
    for M in C.GEMV_MS:
        _exact_check(ops.fp8_block_gemv, d, M)
        _exact_check(ops.fp8_block_gemm, d, M)   # what DECODE_GEMV = False runs: the same bits


@pytest.mark.parametrize("route", ["gemm", "gemv"])
def test_products_on_random_codes_are_within_the_allowance(hip, route):
    """|y - want| <= ulp(want) + 2^-8 * mass: one rounding to the output type plus the project's allowance for the instruction's
    internal sum.  Prints the worst ratio (a record, not a threshold)."""
    from neural_compressor_amd import ops

    (M, N, Kp), product = (C.CROSS_GEMM, ops.fp8_block_gemm) if route == "gemm" else (C.CROSS_GEMV, ops.fp8_block_gemv)
    d = C.random_codes(M, N, Kp, 41 if route == "gemm" else 42)
    xs, ws, bias = C.random_scales(M, N, Kp, 78)
    y64, mass = C.product(TABLE[d["xq"].long()], xs, TABLE[d["wq"].long()], ws)
    worst = 0.0
    for out_dtype in C.OUT_DTYPES:
        for b in (None, bias.to(out_dtype)):
            y = product(d["xq"].cuda(), xs.cuda(), d["wq"].cuda(), ws.cuda(), None if b is None else b.cuda(), out_dtype).double().cpu()
            want = y64 + (0.0 if b is None else b.double()[None, :])
            ratio = float(((y - want).abs() / (C.ulp_of(want, out_dtype) + 2.0 ** -8 * mass)).max())
            worst = max(worst, ratio)
            assert bool(torch.isfinite(y).all()) and ratio <= 1.0, (route, out_dtype, ratio)
    print(f"fp8 block {route} {M}x{N}x{Kp}, random scales: worst |err| / allowance = {worst:.4f}")


def test_products_reject_what_they_do_not_take(hip):
    from neural_compressor_amd import ops

    d = C.exact_case(17, 130, 128)
    args = (d["xq"].cuda(), d["xs"].cuda(), d["wq"].cuda(), d["ws"].cuda())
    with pytest.raises(RuntimeError, match="inc_fp8_block_gemv"):
        ops.fp8_block_gemv(*args, None, torch.bfloat16)            # 17 rows
    with pytest.raises(TypeError):
        ops.fp8_block_gemm(*args, None, torch.float64)
    z, one = torch.zeros(1, 192, dtype=torch.uint8, device="cuda"), torch.ones(1, 1, device="cuda")
    for product in (ops.fp8_block_gemm, ops.fp8_block_gemv):
        with pytest.raises(RuntimeError, match="inc_fp8_block_gem"):
            product(z, one, z, one, None, torch.bfloat16)             # Kp % 128 != 0


def _linear(dtype):
    lin = torch.nn.Linear(600, 260, bias=True)
    lin.weight.data.copy_(C.quant_input(260, 600, torch.float32, 128) * 0.05)
    lin.bias.data.copy_(torch.randn(260, generator=torch.Generator().manual_seed(11)))
    return lin.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_block_linear_is_the_chain_of_its_ops(hip, dtype):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear

    lin = _linear(dtype)
    m = FP8BlockLinear.from_float(lin, device="cuda")
    ft = torch.bfloat16 if dtype == torch.bfloat16 else torch.float16
    wq, ws = C.quant_blocked(lin.weight.detach(), 128)
    assert m.float_type == ft and m.bias.dtype == ft and torch.equal(m.qweight.cpu(), wq) and torch.equal(m.w_scale.cpu(), ws)
    for rows in (1, 16, 17, 300):
        x = (torch.randn(rows, 600, generator=torch.Generator().manual_seed(rows)) * 2).to(dtype)
        xq, xs = ops.fp8_quant_groups(x.cuda(), 640)
        assert torch.equal(xq.cpu(), C.quant_blocked(x, 1)[0])
        y = m(x.cuda())
        chain = (ops.fp8_block_gemv if rows <= 16 else ops.fp8_block_gemm)(xq, xs, m.qweight, m.w_scale, m.bias, ft)
        assert y.dtype == dtype and y.shape == (rows, 260) and torch.equal(y, chain.to(dtype))
        try:
            FP8BlockLinear.DECODE_GEMV = False
            y_tile = m(x.cuda())
        finally:
            FP8BlockLinear.DECODE_GEMV = True
        assert torch.equal(y_tile, ops.fp8_block_gemm(xq, xs, m.qweight, m.w_scale, m.bias, ft).to(dtype))
        # against the float64 product of the dequantised operands: one output ulp + the instruction's allowance (as above)
        want, mass = C.product(TABLE[xq.cpu().long()], xs.cpu(), TABLE[wq.long()], ws)
        want = want + m.bias.double().cpu()[None, :]
        for got in (y, y_tile):
            assert bool(((got.double().cpu() - want).abs() <= C.ulp_of(want, ft) + 2.0 ** -8 * mass).all())
    assert m(x.cuda()[:0]).shape == (0, 260) and m(x.cuda().view(1, 300, 600)).shape == (1, 300, 260)
    assert "w_granularity=per_block" in m.extra_repr() and "in_features=600" in m.extra_repr() and m.recover().dtype == ft


def test_from_finegrained_runs_a_checkpoint_as_it_is(hip, tmp_path):
    """weight float8_e4m3fn [N, K] + weight_scale_inv fp32 [3, 5]: the buffers are the checkpoint's bytes, recover is its dequantisation,
    the forward is that of a from_float module with the same buffers; save / load next to a per-channel FP8Linear."""
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear, FP8Linear, load, save

    lin = _linear(torch.bfloat16)
    wq, s_inv = C.quant_blocked(lin.weight.detach(), 128)
    w8 = wq[:, :600].contiguous().view(torch.float8_e4m3fn)
    assert s_inv.shape == (3, 5)
    m = FP8BlockLinear.from_finegrained(w8, s_inv, lin.bias.detach(), float_type=torch.bfloat16)
    ref = FP8BlockLinear.from_float(lin, device="cuda")
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), ref.state_dict().values()))
    want = w8.float() * s_inv.repeat_interleave(128, 0)[:260].repeat_interleave(128, 1)[:, :600]
    assert torch.equal(m.recover(torch.float32).cpu(), want)
    x = torch.randn(20, 600, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    assert torch.equal(m(x), ref(x))
    q = torch.nn.Sequential(m, torch.nn.ReLU(), FP8Linear.from_float(torch.nn.Linear(260, 24, bias=False).to(torch.bfloat16)))
    y0 = q(x)
    save(q, str(tmp_path))
    r = load(str(tmp_path), torch.nn.Sequential(torch.nn.Linear(600, 260), torch.nn.ReLU(), torch.nn.Linear(260, 24, bias=False)).to(torch.bfloat16))
    assert type(r[0]) is FP8BlockLinear and type(r[2]) is FP8Linear
    a, b = q.state_dict(), r.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a) and torch.equal(r(x), y0)


def test_config_converts_tiny_llama_and_leaves_experts_float(hip, monkeypatch):
    from neural_compressor_amd.common.utils import logger
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear, FP8Experts, FP8Quantizer
    from neural_compressor_amd.torch.quantization import FP8Config, quantize
    from tests import moe_models

    cell = dict(act_granularity="per_group", w_granularity="per_block")
    q = quantize(tiny_llama(dtype=torch.float16).to("cuda"), FP8Config(**cell))
    mods = [n for n, m in q.named_modules() if isinstance(m, FP8BlockLinear)]
    assert len(mods) == 14 and "lm_head" not in mods and isinstance(q.lm_head, torch.nn.Linear)
    assert q.fp8_info == {"fp8_config": "E4M3", **cell}
    with torch.no_grad():
        assert bool(torch.isfinite(q(calib_ids(n=1, seq=32)[0].to("cuda")).logits).all())
    model = torch.nn.Module()
    model.experts = moe_models.experts_of(moe_models.tiny_mixtral(dtype=torch.bfloat16))[0][1]
    messages = []
    monkeypatch.setattr(logger, "warning", lambda fmt, *a: messages.append(fmt % a))
    out = FP8Quantizer(quant_config={"experts": {"fp8_config": "E4M3", **cell}}).convert(model)
    about = [t for t in messages if "stays in floating point" in t]
    assert not isinstance(out.experts, FP8Experts) and len(about) == 1 and "block-scaled" in about[0], messages
