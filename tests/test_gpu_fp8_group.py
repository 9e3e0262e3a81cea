"""-m gpu: the decode group launches of the FP8 per-token / per-channel cell (inc_fp8_gemv_multi, inc_fp8_gemv_gated, fp8_linear_group,
fp8_gated_pair) against tests/fp8_group_cases.py.

  multi     every member's output bit-equal to inc_fp8_gemv's on random codes with Gaussian factors, 3 and 8 members, biases present
            and NULL mixed; the outputs as adjacent slices of one sentinel-filled buffer; a rejected call writes nothing;
  gated     bit-identical to inc_fp8_moe_gemm mode 0 for one expert that holds every row (no bias); on exact operands with biases
            within the mode-0 bound of fp8_moe_cases.check_output of the float64 reference;
  modules   fp8_linear_group == the single forwards bit for bit on a converted tiny_llama layer; fp8_gated_pair == the entry point on
            the quantised x bit for bit, every fallback == act_fn(g) * u exactly, fused against unfused within three roundings.
"""

import contextlib
from unittest import mock

import pytest
import torch

from tests import fp8_group_cases as G
from tests import moe_stage_cases as S
from tests.model_zoo import tiny_llama

pytestmark = pytest.mark.gpu

SENT16 = 0x7B5A
GUARD = 16
DTYPES16 = G.OUT_DTYPES
DTYPE_IDS = ["bf16", "fp16"]


def _code(dtype):
    from neural_compressor_amd import _lib

    return {torch.float32: _lib.INC_F32, torch.float16: _lib.INC_F16, torch.bfloat16: _lib.INC_BF16}[dtype]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype is torch.float32 else torch.int16)


def _assert_bit_equal(a, b, what):
    assert a.shape == b.shape and a.dtype is b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(_bits(a), _bits(b)), what


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


def _multi_on(hip, d, dtype):
    """The operands of a multi case on the device, the biases in `dtype`."""
    biases = [None if b is None else b.to(dtype).to(hip) for b in d["biases"]]
    return d["xq"].to(hip), d["rs"].to(hip), [w.to(hip) for w in d["wqs"]], [a.to(hip) for a in d["als"]], biases


# ---- multi --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", G.TILES)
@pytest.mark.parametrize("M_", G.MS)
def test_multi_is_the_single_launch_bit_for_bit(hip, M_, tiles):
    from neural_compressor_amd import ops

    for Ns in (G.MULTI_NS, G.MULTI_NS8):
        d = G.multi_case(M_, Ns, 128 * tiles)
        for dtype in DTYPES16:
            xq, rs, wqs, als, biases = _multi_on(hip, d, dtype)
            assert any(b is None for b in biases) and any(b is not None for b in biases)
            got = ops.fp8_gemv_multi(xq, rs, wqs, als, biases, dtype)
            assert len(got) == len(Ns)
            for i, y in enumerate(got):
                want = ops.fp8_gemv(xq, rs, wqs[i], als[i], biases[i], dtype)
                _assert_bit_equal(y.cpu(), want.cpu(), f"M {M_}, {tiles} tiles, {len(Ns)} members, member {i}, {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16, ids=DTYPE_IDS)
def test_multi_writes_only_its_outputs(hip, dtype):
    """The y[i] are adjacent slices of one sentinel-filled buffer (y[2], of N % 4 == 0, starts at an odd element offset: 2-byte stores
    where the single launch below stores 8 bytes): every slice holds the single launch's bits, which leaves nothing of a neighbour's,
    and the guards around them stay."""
    from neural_compressor_amd import ops

    M_, Ns, Kp = 15, G.MULTI_NS, 128 * 9
    d = G.multi_case(M_, Ns, Kp)
    xq, rs, wqs, als, biases = _multi_on(hip, d, dtype)
    total = sum(M_ * N for N in Ns)
    buf = torch.full((GUARD + total + GUARD,), SENT16, dtype=torch.int16, device=hip)
    outs, off = [], GUARD
    for N in Ns:
        outs.append(buf[off:off + M_ * N].view(dtype).view(M_, N))
        off += M_ * N
    got = ops.fp8_gemv_multi(xq, rs, wqs, als, biases, dtype, outs=outs)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, outs))
    assert bool((buf[:GUARD] == SENT16).all()) and bool((buf[GUARD + total:] == SENT16).all()), "wrote around the outputs"
    for i in range(len(Ns)):
        want = ops.fp8_gemv(xq, rs, wqs[i], als[i], biases[i], dtype)
        _assert_bit_equal(outs[i].cpu(), want.cpu(), f"member {i}")


def test_a_rejected_call_writes_nothing(hip):
    import ctypes

    from neural_compressor_amd import _lib

    M_, Ns, Kp = 16, G.MULTI_NS, 256
    d = G.multi_case(M_, Ns, Kp)
    xq, rs, wqs, als, _ = _multi_on(hip, d, torch.bfloat16)
    ys = [torch.full((M_ + 1, N), SENT16, dtype=torch.int16, device=hip) for N in Ns]
    h = torch.full((M_ + 1, Ns[2]), SENT16, dtype=torch.int16, device=hip)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    n64 = lambda v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    BF16 = _lib.INC_BF16

    def multi(n=3, ydtype=BF16, rows=M_, kp=Kp, Nv=Ns):
        return _lib.lib.inc_fp8_gemv_multi(n, xq.data_ptr(), rs.data_ptr(), arr(wqs), arr(als), None, arr(ys), ydtype, rows, n64(Nv), kp,
                                           stream)

    def gated(ydtype=BF16, rows=M_, kp=Kp, N=Ns[2]):
        return _lib.lib.inc_fp8_gemv_gated(xq.data_ptr(), rs.data_ptr(), wqs[2].data_ptr(), als[2].data_ptr(), None, wqs[2].data_ptr(),
                                           als[2].data_ptr(), None, h.data_ptr(), ydtype, rows, N, kp, stream)

    assert multi(n=1) == -2 and multi(n=9) == -2
    for fn in (multi, gated):
        assert fn(rows=17) == -2 and fn(kp=192) == -2 and fn(ydtype=_lib.INC_F32) == -2 and fn(rows=0) == -1
    assert multi(Nv=[4, 0, 260]) == -1 and gated(N=0) == -1
    torch.cuda.synchronize()
    assert all(bool((y == SENT16).all()) for y in ys + [h])


# ---- gated against the experts kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", G.TILES)
@pytest.mark.parametrize("M_", G.GATED_MS)
def test_gated_is_the_experts_kernel_on_one_expert(hip, M_, tiles):
    """inc_fp8_moe_gemm mode 0 with one expert, top_k = 1 and every row routed to it, weight cat(gate, up) and alpha cat(alpha_gate,
    alpha_up), no bias: the same sums and the same epilogue, so the same bits -- on random codes whose sums are not exact.  The experts
    entry takes every shape used here (N = 2 I even, E = 1, S <= 16)."""
    from neural_compressor_amd import ops

    ro = S.route_oracle(torch.zeros(M_, 1, dtype=torch.int64), 1)          # T = rows, k = 1, E = 1: position p is token p
    assert ro["order"].tolist() == list(range(M_))
    route = S.route_buffer(ro, fill=-1).to(hip)
    for N in G.GATED_NS:
        d = G.gated_random_case(M_, N, 128 * tiles)
        xq, wg, wu, rs, ag, au = (d[k].to(hip) for k in ("xq", "wg", "wu", "rs", "ag", "au"))
        wq = torch.cat([wg, wu])[None].contiguous()
        al = torch.cat([ag, au])[None].contiguous()
        for dtype in DTYPES16:
            got = ops.fp8_gemv_gated(xq, rs, wg, ag, None, wu, au, None, dtype).cpu()
            want = ops.fp8_moe_gemm(0, xq, rs, route, wq, al, M_, 1, out_dtype=dtype).cpu()
            assert bool(torch.isfinite(got.float()).all())
            _assert_bit_equal(got, want, f"M {M_}, N {N}, {tiles} tiles, {dtype}")


# ---- gated on exact operands with bias ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", ["both", "gate"])
@pytest.mark.parametrize("tiles", G.TILES)
@pytest.mark.parametrize("M_", [1, 16])
def test_gated_exact_operands_with_bias(hip, M_, tiles, bias):
    from neural_compressor_amd import ops

    worst = 0.0
    for N in (7, 260):
        d = G.gated_exact_case(M_, N, 128 * tiles, bias)
        min_g, _ = G.assert_gated_exact_condition(d)
        assert min_g >= -80.0
        xq, wg, wu = (t.to(hip) for t in G.gated_stored(d))
        rs, ag, au = d["rs"].to(hip), d["ag"].to(hip), d["au"].to(hip)
        for dtype in DTYPES16:
            bg = None if d["bg"] is None else d["bg"].to(dtype).to(hip)
            bu = None if d["bu"] is None else d["bu"].to(dtype).to(hip)
            h = ops.fp8_gemv_gated(xq, rs, wg, ag, bg, wu, au, bu, dtype).cpu()
            assert h.shape == (M_, N) and h.dtype is dtype
            g, u, _ = G.gated_reference(d)
            zero = torch.zeros(())
            ref, tol = S.mode0_tolerance(g, u, zero, zero, dtype)
            ok = 1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2
            r, _ = S.worst_ratio(torch.where(ok, h.double(), ref), ref, tol)
            worst = max(worst, r)
            why = G.gated_check(d, h, dtype)
            assert why is None, f"M {M_}, N {N}, {tiles} tiles, bias {bias}, {dtype}: {why}"
            again = ops.fp8_gemv_gated(xq, rs, wg, ag, bg, wu, au, bu, dtype).cpu()
            _assert_bit_equal(h, again, "repeated calls differ")
    print(f"gated exact M {M_} tiles {tiles} bias {bias}: worst ratio to the mode-0 bound {worst:.4f}")


# ---- modules ------------------------------------------------------------------------------------------------------------------------
_layer = {}


def _llama_layer(hip):
    """Layer 0 of tiny_llama (bf16) under FP8Config: q / k / v and gate / up are FP8Linear of 64 -> 64 and 64 -> 128.  Converted once."""
    if "m" not in _layer:
        from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear
        from neural_compressor_amd.torch.quantization import FP8Config, quantize

        q = quantize(tiny_llama(dtype=torch.bfloat16).to(hip), FP8Config())
        layer = q.model.layers[0]
        assert all(isinstance(m, FP8Linear) for m in (layer.self_attn.q_proj, layer.mlp.gate_proj, layer.mlp.up_proj))
        _layer["m"] = layer
    return _layer["m"]


def _fp8(hip, K, N, bias, dtype, seed):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear

    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(K, N, bias=bias)
    lin.weight.data.copy_(torch.randn(N, K, generator=g) * 0.05)
    if bias:
        lin.bias.data.copy_(torch.randn(N, generator=g) * 0.3)
    return FP8Linear.from_float(lin.to(dtype), device=hip)


def _switch_on(monkeypatch):
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear, fp8_quant

    monkeypatch.setattr(FP8Linear, "DECODE_GEMV", True)
    monkeypatch.setattr(FP8Linear, "DECODE_MAX_M", 16)
    monkeypatch.setattr(fp8_quant, "GATED_FUSED", True)
    return FP8Linear, fp8_quant


@pytest.mark.parametrize("xdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_linear_group_is_the_list_of_single_forwards(hip, xdtype, monkeypatch):
    from neural_compressor_amd.torch.algorithms.fp8_quant import fp8_linear_group

    FP8Linear, _ = _switch_on(monkeypatch)
    attn = _llama_layer(hip).self_attn
    biased = [_fp8(hip, 200, N, b, torch.bfloat16, 40 + N) for N, b in ((72, True), (24, False), (33, True))]
    g = torch.Generator().manual_seed(4)
    for mods, K in (([attn.q_proj, attn.k_proj, attn.v_proj], 64), (biased, 200)):
        for lead, rows in (((1,), 1), ((2, 8), 16), ((17,), 17), ((3, 100), 300)):
            x = (torch.randn(*lead, K, generator=g) * 1.2 + 0.3).to(xdtype).to(hip)
            with torch.no_grad():
                want = [m(x) for m in mods]
                with _counting("fp8_quant_rows", "fp8_gemv_multi", "fp8_gemv", "fp8_gemm") as calls:
                    got = fp8_linear_group(x, mods)
            decode = rows <= 16
            assert calls == {"fp8_quant_rows": 1, "fp8_gemv_multi": int(decode), "fp8_gemv": 0, "fp8_gemm": 0 if decode else 3}, (rows, calls)
            for i, (a, b) in enumerate(zip(got, want)):
                assert a.shape == (*lead, mods[i].out_features) and a.dtype is xdtype
                _assert_bit_equal(a.cpu(), b.cpu(), f"K {K}, {rows} rows, member {i}")
    monkeypatch.setattr(FP8Linear, "DECODE_GEMV", False)               # the switch off at decode size: exactly the single forwards
    x = torch.randn(16, 200, generator=g).to(xdtype).to(hip)
    with torch.no_grad(), _counting("fp8_gemv_multi", "fp8_gemv", "fp8_quant_rows", "fp8_gemm") as calls:
        got = fp8_linear_group(x, biased)
    assert calls == {"fp8_gemv_multi": 0, "fp8_gemv": 0, "fp8_quant_rows": 3, "fp8_gemm": 3}, calls
    with torch.no_grad():
        for i, (a, b) in enumerate(zip(got, [m(x) for m in biased])):
            _assert_bit_equal(a.cpu(), b.cpu(), f"switch off, member {i}")


@pytest.mark.parametrize("xdtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_gated_pair_is_the_entry_point_on_the_quantised_x(hip, xdtype, monkeypatch):
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import fp8_gated_pair

    _switch_on(monkeypatch)
    mlp = _llama_layer(hip).mlp
    ft = torch.float16 if xdtype is torch.float16 else torch.bfloat16
    biased = (_fp8(hip, 200, 72, True, ft, 51), _fp8(hip, 200, 72, True, ft, 52))
    g = torch.Generator().manual_seed(8)
    pairs = [(biased, 200)] + ([((mlp.gate_proj, mlp.up_proj), 64)] if ft is torch.bfloat16 else [])
    for (gate, up), K in pairs:
        for lead in ((1,), (2, 8)):
            x = (torch.randn(*lead, K, generator=g) * 1.2 + 0.3).to(xdtype).to(hip)
            for act in (None, torch.nn.SiLU()):
                with torch.no_grad(), _counting("fp8_quant_rows", "fp8_gemv_gated", "fp8_gemv_multi", "fp8_gemv") as calls:
                    got = fp8_gated_pair(x, gate, up, act)
                assert calls == {"fp8_quant_rows": 1, "fp8_gemv_gated": 1, "fp8_gemv_multi": 0, "fp8_gemv": 0}, calls
                xq, rs = ops.fp8_quant_rows(x.reshape(-1, K), None, gate.kp)
                want = ops.fp8_gemv_gated(xq, rs, gate.qweight, gate.w_scale, gate.bias, up.qweight, up.w_scale, up.bias, ft)
                want = (want.float() if xdtype is torch.float32 else want).reshape(*lead, gate.out_features)
                assert got.dtype is xdtype
                _assert_bit_equal(got.cpu(), want.cpu(), f"K {K}, lead {lead}, act {act}")


def test_gated_pair_fallbacks_are_the_unfused_form(hip, monkeypatch):
    from neural_compressor_amd.torch.algorithms.fp8_quant import fp8_gated_pair, fp8_linear_group

    _, mod = _switch_on(monkeypatch)
    ft = torch.bfloat16
    gate, up = _fp8(hip, 200, 72, True, ft, 51), _fp8(hip, 200, 72, False, ft, 52)
    one = _fp8(hip, 200, 1, False, ft, 53)
    dense = torch.nn.Linear(200, 72, bias=True).to(ft).to(hip)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 200, generator=g).to(ft).to(hip)
    x17 = torch.randn(17, 200, generator=g).to(ft).to(hip)
    silu, gelu = torch.nn.functional.silu, torch.nn.GELU()

    def check(what, inp, a, b, act_fn, act):
        with torch.no_grad():
            gg, uu = fp8_linear_group(inp, [a, b])
            with _counting("fp8_gemv_gated") as calls:
                got = fp8_gated_pair(inp, a, b, act_fn)
        assert calls == {"fp8_gemv_gated": 0}, what
        assert torch.equal(got, act(gg) * uu), what

    check("17 rows", x17, gate, up, None, silu)
    check("a GELU act_fn", x, gate, up, gelu, gelu)
    check("a non-FP8 member", x, gate, dense, None, silu)
    check("unequal out_features", x, gate, one, None, silu)            # an up of one column: act(g) * u broadcasts
    monkeypatch.setattr(mod, "GATED_FUSED", False)
    check("GATED_FUSED = False", x, gate, up, None, silu)


def test_fused_and_unfused_differ_by_three_roundings(hip, monkeypatch):
    """The unfused form rounds g, u and silu(g) to 16 bits before its product is rounded; the fused one rounds once:
        |dh| <= 1.5 (1.1 |g| |u| u_out + 3 u_out |h|)      (|silu'| <= 1.1; three roundings on the product; 1.5 covers second order)
    the bound test_both_routes_against_the_emulation_fed_the_fused_h (test_gpu_fp8_moe.py) uses for the experts.  bf16, as there."""
    from neural_compressor_amd.torch.algorithms.fp8_quant import fp8_gated_pair, fp8_linear_group

    _, mod = _switch_on(monkeypatch)
    cdt = torch.bfloat16
    u_out, _ = S.out_rounding(cdt)
    mlp = _llama_layer(hip).mlp
    worst = 0.0
    for (gate, up), K in (((mlp.gate_proj, mlp.up_proj), 64), ((_fp8(hip, 200, 260, True, cdt, 61), _fp8(hip, 200, 260, True, cdt, 62)), 200)):
        for rows in (1, 16):
            x = (torch.randn(rows, K, generator=torch.Generator().manual_seed(rows)) * 1.2 + 0.3).to(cdt).to(hip)
            with torch.no_grad():
                monkeypatch.setattr(mod, "GATED_FUSED", True)
                fused = fp8_gated_pair(x, gate, up).double().cpu()
                monkeypatch.setattr(mod, "GATED_FUSED", False)
                unfused = fp8_gated_pair(x, gate, up).double().cpu()
                gg, uu = (t.double().cpu() for t in fp8_linear_group(x, [gate, up]))
            tol = 1.5 * (1.1 * gg.abs() * uu.abs() * u_out + 3 * u_out * fused.abs())
            r, (i, j) = S.worst_ratio(unfused, fused, tol)
            worst = max(worst, r)
            assert r <= 1.0, (K, rows, r, i, j)
    print(f"fused against unfused: worst ratio to the three-roundings bound {worst:.4f}")
