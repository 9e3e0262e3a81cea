"""-m gpu: the fused forward of 4-bit row-packed modules (inc_woq_gemm_lut, DESIGN K4d) -- NF4 / FP4 code books and integer modules
packed with use_optimum_format=False, compression_dim = 1.  The weight the kernel decodes in registers is recover(x.dtype) bit for bit
(identity activations), the products match an fp32 referee to the bf16 output rounding at user sizes, repeated calls are
bit-identical, recover() never runs, and every module the kernel does not take keeps the dense route."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMATS = ["nf4", "fp4", "fp4_e2m1", "int_sym", "int_asym"]


def _module(hip, fmt, N, K, gs, scale_dtype=torch.float32, cdtype=torch.int32, bias=False, seed=0, compression_dim=1, g_idx=False, bits=4):
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    g = torch.Generator().manual_seed(seed)
    dtype = "int" if fmt.startswith("int") else fmt
    asym = fmt == "int_asym"
    m = MI355XWeightOnlyLinear(K, N, dtype=dtype, bits=bits, group_size=gs, zp=asym, bias=bias, scale_dtype=scale_dtype,
                               compression_dtype=cdtype, compression_dim=compression_dim, g_idx=g_idx, use_optimum_format=False, device=hip)
    G = m.scales.shape[1]
    lo, hi = (0, 2**bits) if asym else (-(2 ** (bits - 1)), 2 ** (bits - 1))
    iw = torch.randint(lo, hi, (N, K), generator=g, dtype=torch.int32)
    sc = (torch.rand(N, G, generator=g) * 0.02 + 0.001).to(scale_dtype)
    zp = torch.randint(0, 2**bits, (N, G), generator=g, dtype=torch.int32) if asym else None
    b = (torch.randn(N, generator=g) * 0.1) if bias else None
    gi = (torch.arange(K) // m.group_size).flip(0).to(torch.int32) if g_idx else None
    m.pack(iw, sc, zp, b, g_idx=gi)
    return m


def _plan(m):
    return m._forward_plan()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the decoded weight is recover(x.dtype) bit for bit: x = rows of the identity, no bias -> forward(x) == recover(x.dtype).T rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [32, 64, 128, -1])
@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sdt", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_rows_decode_bit_exact(hip, fmt, sdt, xdt, gs):
    for N, K, cdt in ((256, 512, torch.int32), (320, 1024, torch.int8 if gs == 64 else torch.int64)):
        m = _module(hip, fmt, N, K, gs, scale_dtype=sdt, cdtype=cdt, seed=N + K)
        assert _plan(m) == "fused_lut"
        wt = m.recover(dtype=xdt).T.contiguous()  # [K, N]
        eye = torch.eye(K, dtype=xdt, device=hip)
        for r0 in range(0, K, 64):  # the streaming form: <= 64 rows per call (the last slice of K = 1024 has 64 rows too)
            rows = eye[r0:r0 + 64] if r0 + 64 <= K else eye[r0:]
            assert torch.equal(m(rows), wt[r0:r0 + rows.shape[0]]), (fmt, sdt, xdt, gs, N, K, r0)
        for r0, r1 in ((0, 17), (5, 6), (K - 40, K)):  # ragged row counts
            assert torch.equal(m(eye[r0:r1].contiguous()), wt[r0:r1]), (fmt, sdt, xdt, gs, N, K, r0, r1)
        for r0 in range(0, K, 256):  # M > 64: 64-row tiles on the grid (256 = LUT_MAX_M rows per call)
            assert torch.equal(m(eye[r0:r0 + 256]), wt[r0:r0 + 256]), (fmt, sdt, xdt, gs, N, K, r0, "256 rows")
        assert torch.equal(m(eye[:100].contiguous()), wt[:100]), (fmt, sdt, xdt, gs, N, K, "100 rows")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. against the fp32 referee at user sizes
# ---------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _ref_module(hip, fmt, N, K):
    key = (fmt, N, K)
    if key not in _REF:
        _REF.clear()  # one (module, dense weight) pair alive at a time
        m = _module(hip, "nf4" if fmt == "nf4" else "int_asym", N, K, 32 if fmt == "nf4" else 128, bias=True, seed=7)
        _REF[key] = (m, m.recover(dtype=torch.bfloat16).float())
    return _REF[key]


@pytest.mark.parametrize("M", [1, 4, 16, 17, 64, 65, 512, 4096])
@pytest.mark.parametrize("N,K", [(4096, 4096), (11008, 4096), (4096, 11008)])
@pytest.mark.parametrize("fmt", ["nf4", "int_asym"])
def test_user_sizes_vs_fp32_referee(hip, fmt, N, K, M):
    m, w = _ref_module(hip, fmt, N, K)
    assert _plan(m) == "fused_lut"
    g = torch.Generator(device=hip).manual_seed(M)
    x = torch.randn(M, K, generator=g, device=hip).to(torch.bfloat16)
    y = m(x)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    b = m.bias.to(torch.bfloat16).float()
    ref = F.linear(x.float(), w, b)
    # the output is rounded to bf16 (half an ulp: 2^-9 relative) after an fp32 sum in another order than the referee's
    mag = F.linear(x.float().abs(), w.abs(), b.abs())
    err = (y.float() - ref).abs()
    bound = 2.0**-8 * ref.abs() + 2.0**-16 * mag + 1e-30
    assert bool((err <= bound).all()), (fmt, N, K, M, float((err / (mag + 1e-30)).max()))
    assert torch.equal(m(x), y)  # deterministic: a fixed-order split-K sum


def test_prefill_batches_take_the_dense_route(hip, monkeypatch):
    """Above LUT_MAX_M rows the forward is recover() + the library GEMM (the measured crossover); at LUT_MAX_M it is the fused kernel."""
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    m = _module(hip, "nf4", 256, 512, 32, seed=4)
    cap = MI355XWeightOnlyLinear.LUT_MAX_M
    x = torch.randn(cap + 1, 512, device=hip).to(torch.bfloat16)
    m(x[:1])  # a prepared call exists; it must not take the larger batch
    call = m.__dict__["_call"]
    assert call is not None and call.lut
    y_cap = m(x[:cap])
    assert m.__dict__["_call"] is call, "LUT_MAX_M rows rebuilt the prepared call"
    assert torch.equal(m(x), F.linear(x, m.recover(dtype=torch.bfloat16)))
    assert m.__dict__["_call"] is None, "a batch on the dense route kept the prepared call"
    calls = []
    real = m.recover
    monkeypatch.setattr(m, "recover", lambda *a, **k: calls.append(1) or real(*a, **k))
    assert torch.equal(m(x[:cap]), y_cap)
    assert not calls
    assert m.__dict__["_call"] is not None and m.__dict__["_call"] is not call  # rebuilt
    m(x)
    assert calls and m.__dict__["_call"] is None


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the forward does not materialise the weight
# ---------------------------------------------------------------------------------------------------------------------------------
def test_forward_never_calls_recover(hip, monkeypatch):
    m = _module(hip, "nf4", 512, 1024, 32, bias=True, seed=3)
    x = torch.randn(2, 9, 1024, device=hip).to(torch.bfloat16)  # 3-D input
    ref = F.linear(x.float(), m.recover(dtype=torch.bfloat16).float(), m.bias.to(torch.bfloat16).float())

    def boom(*a, **k):
        raise AssertionError("recover() called on the fused route")

    monkeypatch.setattr(m, "recover", boom)
    for _ in range(2):  # the first call builds the prepared call, the second goes through it
        y = m(x)
        assert y.shape == (2, 9, 512) and y.dtype == torch.bfloat16
        assert float((y.float() - ref).abs().max()) <= 2.0**-7 * float(ref.abs().max())
    # dtype contract of forward: fp32 in -> fp16 multiply -> fp32 out; empty batch
    y32 = m(x.float())
    assert y32.dtype == torch.float32 and y32.shape == (2, 9, 512)
    assert torch.equal(y32, m(x.half()).float())
    e = m(torch.empty(0, 1024, device=hip, dtype=torch.bfloat16))
    assert e.shape == (0, 512)


def test_prepared_call_follows_repack_and_switch(hip):
    """The cached call is dropped when the module is re-packed and when LUT_FUSED is switched off."""
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    m = _module(hip, "nf4", 256, 512, 32, seed=1)
    x = torch.randn(3, 512, device=hip).to(torch.float16)
    y0 = m(x)
    m2 = _module(hip, "nf4", 256, 512, 32, seed=2)
    m.pack(_ints_of(m2), m2.scales, None, None)
    y1 = m(x)
    assert torch.equal(y1, m2(x)) and not torch.equal(y0, y1)
    call = m.__dict__["_call"]
    assert call is not None and call.lut
    try:
        MI355XWeightOnlyLinear.LUT_FUSED = False
        yd = m(x)  # (the forward itself must notice the switch: its guard stands in front of the plan)
        assert m.__dict__["_call"] is None and _plan(m) == "dense"
        assert torch.equal(yd, F.linear(x, m.recover(dtype=torch.float16)))
    finally:
        MI355XWeightOnlyLinear.LUT_FUSED = True
    assert _plan(m) == "fused_lut"
    assert torch.equal(m(x), y1) and m.__dict__["_call"] not in (None, call)  # rebuilt
    w = m.recover(dtype=torch.float16).float()
    ref = F.linear(x.float(), w)
    assert float((yd.float() - ref).abs().max()) <= 2.0**-9 * float(ref.abs().max()) + 1e-6


def _ints_of(m):
    """The stored integers of a code-book module (the codes pack() takes)."""
    from neural_compressor_amd import ops

    return ops.unpack_rows(m.qweight, m.bits, m.compress_bits, False)[:, : m.in_features].to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. routing: what the kernel does not take keeps the dense route, with the dense route's outputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nf4", "int_sym", "int_asym", "fp4_e2m1_bnb"])
@pytest.mark.parametrize("cdt", [torch.int8, torch.int16, torch.int32, torch.int64])
def test_eligible_modules_take_the_fused_route(hip, fmt, cdt):
    m = _module(hip, fmt, 192, 384, 96, cdtype=cdt, bias=True, seed=5)  # group 96: a multiple of 32, not a power of two
    assert _plan(m) == "fused_lut"
    x = torch.randn(5, 384, device=hip).to(torch.bfloat16)
    w = m.recover(dtype=torch.bfloat16).float()
    ref = F.linear(x.float(), w, m.bias.to(torch.bfloat16).float())
    assert float((m(x).float() - ref).abs().max()) <= 2.0**-7 * float(ref.abs().max())


@pytest.mark.parametrize("case", ["compression_dim0", "g_idx", "k_not_32", "bits3", "group16"])
def test_ineligible_modules_keep_the_dense_route(hip, case):
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    if case == "compression_dim0":
        m = _module(hip, "nf4", 128, 256, 32, compression_dim=0)
    elif case == "g_idx":
        m = _module(hip, "int_asym", 128, 256, 32, g_idx=True)
    elif case == "k_not_32":
        m = _module(hip, "nf4", 128, 240, -1)
    elif case == "bits3":
        m = _module(hip, "int_sym", 128, 256, 32, bits=3)
    else:
        m = _module(hip, "int_asym", 128, 256, 16)
    assert _plan(m) == "dense"
    x = torch.randn(7, m.in_features, device=hip).to(torch.bfloat16)
    y = m(x)
    try:
        MI355XWeightOnlyLinear.LUT_FUSED = False
        yd = m(x)
    finally:
        MI355XWeightOnlyLinear.LUT_FUSED = True
    assert torch.equal(y, yd)
    assert torch.equal(y, F.linear(x, m.recover(dtype=torch.bfloat16)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. model level: RTN NF4 on tiny_llama
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rtn_nf4_tiny_llama_fused(hip, tmp_path):
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear
    from neural_compressor_amd.torch.algorithms.weight_only.save_load import load, save
    from neural_compressor_amd.torch.quantization import RTNConfig, quantize

    g = np.load(os.path.join(ROOT, "tests", "golden", "nf4_golden.npz"))
    q = quantize(tiny_llama(), RTNConfig(dtype="nf4", group_size=32, use_layer_wise=False))
    mods = [m for m in q.modules() if isinstance(m, MI355XWeightOnlyLinear)]
    assert len(mods) == 14 and all(_plan(m) == "fused_lut" for m in mods)
    ids = calib_ids()[0].to(hip)
    with torch.no_grad():
        y32 = q(ids).logits.float().cpu()
        try:
            MI355XWeightOnlyLinear.LUT_FUSED = False
            yd = q(ids).logits.float().cpu()
        finally:
            MI355XWeightOnlyLinear.LUT_FUSED = True
    assert float((y32 - yd).norm() / yd.norm()) <= 1e-2
    save(q, str(tmp_path))
    back = load(str(tmp_path), original_model=tiny_llama(), device=hip)
    with torch.no_grad():
        assert torch.equal(back(ids).logits.float().cpu(), y32)
        for mod in q.modules():  # fp16 compute, the gate of the reference golden (test_gpu_nf4)
            for p in mod.parameters(recurse=False):
                if p.is_floating_point():
                    p.data = p.data.half()
        y = q(ids).logits.float().cpu().numpy()
    ref = g["rtn_nf4_logits"]
    assert np.linalg.norm(y - ref) / np.linalg.norm(ref) <= 2e-2
