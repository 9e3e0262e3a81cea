"""No GPU: the MX oracle of tests/mx_cases.py checks itself, the cases reach what they were written for, the config API, and the new
entry points exist and reject bad arguments before any HIP call."""

import pytest
import torch

from tests import mx_cases as C
from tests.model_zoo import tiny_llama

FMTS = [C.FP8, C.FP4]
QPARAMS = [pytest.param(c, dt, id=f"{c.name}-{C.DTYPE_IDS[C.DTYPES.index(dt)]}") for c in C.QCASES for dt in C.DTYPES]


def _scaled(x, s, Kp):
    """x * 2^(127 - byte) in float64, padded to Kp."""
    M, K = x.shape
    xp = torch.zeros(M, Kp, dtype=torch.float64)
    xp[:, :K] = x.double()
    return (xp.view(M, Kp // 32, 32) * torch.ldexp(torch.ones(s.shape, dtype=torch.float64), 127 - s.int())[:, :, None]).view(M, Kp)


@pytest.mark.parametrize("c,dtype", QPARAMS)
def test_oracle_fp8_codes_are_torchs_e4m3_cast(c, dtype):
    """The second, independent oracle: torch's float8_e4m3fn cast of the clamped, scaled values, byte for byte (the sign of a zero
    from x: the cast keeps it, the padding is +0)."""
    x = C.quant_inputs(c, dtype, C.FP8)
    q, s = C.quant_mx(x, C.FP8)
    Kp = C.padded_k(c.K)
    assert q.shape == (c.M, Kp) and s.shape == (c.M, Kp // 32) and int(s.max()) <= 254
    v = _scaled(x, s, Kp)
    assert bool((v.float().double() == v).all() | (v.abs() < 2.0 ** -20).all())       # the scaled values are fp32 values
    want = v.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q, want)
    assert not bool(((q & 0x7F) == 0x7F).any())                                        # no NaN code
    assert not bool(q[:, c.K:].any()) and (Kp - c.K < 32 or not bool(s[:, (c.K + 31) // 32:].any()))   # padding: code 0, byte 0


@pytest.mark.parametrize("c,dtype", QPARAMS)
def test_oracle_fp4_results_lie_on_the_grid_and_are_nearest(c, dtype):
    x = C.quant_inputs(c, dtype, C.FP4)
    q, s = C.quant_mx(x, C.FP4)
    Kp = C.padded_k(c.K)
    assert int(q.max()) < 16
    v = _scaled(x, s, Kp)
    got = C.code_table(C.FP4)[q.long()]
    grid = torch.tensor(C.FP4_GRID, dtype=torch.float64)
    assert bool(torch.isin(got.abs(), grid).all())
    nearest = (v.abs().clamp(max=6.0)[..., None] - grid).abs().min(dim=-1).values
    assert torch.equal((got.abs() - v.abs().clamp(max=6.0)).abs(), nearest)            # a nearest grid point (ties: the table below)
    assert torch.equal(torch.signbit(got)[:, :c.K], torch.signbit(x))                  # the sign of x, for zeros too
    assert torch.equal(C.unpack_fp4(C.pack_fp4(q)), q) and int(C.pack_fp4(q)[0, 0]) == int(q[0, 0]) | (int(q[0, 1]) << 4)


@pytest.mark.parametrize("fmt", FMTS, ids=["fp8", "fp4"])
def test_tie_tables(fmt):
    ties, to, anchor = C.ties_of(fmt)
    x = torch.zeros(1, 32)
    vals = [anchor] + ties + [-t for t in ties]
    x[0, :len(vals)] = torch.tensor(vals)
    q, s = C.quant_mx(x, fmt)
    assert int(s[0, 0]) == 127
    d = C.dequant_mx(q, s, fmt)[0]
    assert d[1:1 + len(ties)].tolist() == to and d[1 + len(ties):1 + 2 * len(ties)].tolist() == [-t for t in to]
    assert torch.signbit(d[1 + len(ties)])                                             # -tie that rounds to zero keeps its sign


@pytest.mark.parametrize("fmt", FMTS, ids=["fp8", "fp4"])
def test_special_rows_reach_their_boundaries(fmt):
    e = 8 if fmt == C.FP8 else 2
    c = C.QCASES[2]
    assert c.rows == ["zero", "pow2", "below", "sat", "ties"]
    for dtype in C.DTYPES:
        x = C.quant_inputs(c, dtype, fmt)
        q, s = C.quant_mx(x, fmt)
        sat_code = 0x7E if fmt == C.FP8 else 7
        mask = 0x7F if fmt == C.FP8 else 7
        assert int(s[0, 0]) == 0 and not bool((q[0, :32] & mask).any()) and int(q[0, 5]) == (0x80 if fmt == C.FP8 else 8)
        for b in range(6):
            j = (3 * b) % 21 - 10
            assert int(s[1, b]) == j + 127 - e and int(s[2, b]) == j - 1 + 127 - e    # 2^j against the value just below it
            assert int(s[3, b]) == j + 127 - e and int(q[3, 32 * b + b] & mask) == sat_code
        assert int(s[0, 7]) == 0 and not bool(q[:, 200:].any())                        # the fully padded block
    big = C.quant_inputs(C.QCASES[1], torch.float32, fmt)
    q, s = C.quant_mx(big, fmt)
    assert int(s[3, 0]) == 254 - e and int(s[2, 0]) == 0                               # FLT_MAX; fp32 subnormals


@pytest.mark.parametrize("fmt", FMTS, ids=["fp8", "fp4"])
def test_dequant_of_quant_is_idempotent(fmt):
    for c in C.QCASES[:4]:
        x = C.quant_inputs(c, torch.float32, fmt)
        q, s = C.quant_mx(x, fmt)
        d = C.dequant_mx(q, s, fmt)
        q2, s2 = C.quant_mx(d, fmt)
        assert torch.equal(C.dequant_mx(q2, s2, fmt), d)
    t = C.code_table(C.FP8)
    assert torch.equal(t[:127].float(), torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).float())
    assert C.code_table(C.FP4)[:8].tolist() == C.FP4_GRID


@pytest.mark.parametrize("c", C.GCASES, ids=C.GCASE_IDS)
def test_exact_operand_condition_holds(c):
    assert c.Kp % C.KTILE == 0 and c.Kp <= 1024
    for rule in C.SCALE_RULES:
        d = C.exact_operands(c, rule)
        C.assert_exact_condition(d)
        for fmt in FMTS:                                                               # the values are exact in both formats
            assert torch.equal(C.code_table(fmt)[C.encode_values(d["x"], fmt).long()], d["x"].double())
    blocky = C.exact_operands(c, "block")
    assert c.Kp == 128 and c.M == 1 or bool((blocky["xs"][:, 0] != blocky["xs"][:, 1]).any())


def test_gemm_cases_cover_the_tile_edges():
    Ms, Ns = {c.M for c in C.GCASES}, {c.N for c in C.GCASES}
    assert {1, C.TILE - 1, C.TILE, C.TILE + 1} <= Ms and {1, C.TILE - 1, C.TILE, C.TILE + 1} <= Ns
    assert any(c.N % 4 for c in C.GCASES) and any(c.y_misaligned and c.N % 4 == 0 for c in C.GCASES)
    tiles = {c.Kp // C.KTILE for c in C.GCASES}
    assert {1, 2} <= tiles and any(t % 2 == 1 and t > 1 for t in tiles)
    assert max(c.M for c in C.GCASES) <= 2 * C.TILE + 1


# ---- config API -----------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_pairs():
    from neural_compressor_amd.common.utils import MX_QUANT
    from neural_compressor_amd.torch.quantization import MXQuantConfig, get_default_mx_config

    d = get_default_mx_config()
    assert isinstance(d, MXQuantConfig) and d.name == MX_QUANT == "mx_quant"
    assert (d.w_dtype, d.act_dtype, d.blocksize, d.round_method, d.weight_only) == ("fp8_e4m3", "fp8_e4m3", 32, "nearest", False)
    for w, a in (("fp8_e4m3", "fp8_e4m3"), ("fp4", "fp8_e4m3"), ("fp4", "fp4")):
        c = MXQuantConfig(w_dtype=w, act_dtype=a, out_dtype="float16")
        assert (c.w_dtype, c.act_dtype) == (w, a)


@pytest.mark.parametrize("kw", [dict(w_dtype="int8", act_dtype="int8"), dict(w_dtype="fp8_e4m3", act_dtype="fp4"), dict(w_dtype="fp8_e5m2"),
                                dict(act_dtype="fp6_e2m3"), dict(blocksize=64), dict(round_method="floor"), dict(weight_only=True)],
                         ids=["mx_int8", "a4w8", "e5m2", "fp6", "blocksize", "round_method", "weight_only"])
def test_config_rejects_what_is_not_built(kw):
    from neural_compressor_amd.torch.quantization import MXQuantConfig

    with pytest.raises(NotImplementedError, match="MXQuant on MI355X"):
        MXQuantConfig(**kw)


def test_config_mapping_of_tiny_llama():
    from neural_compressor_amd.torch.quantization import MXQuantConfig

    model = tiny_llama(dtype=torch.float16)
    cfg = MXQuantConfig()
    mapping = cfg.to_config_mapping(model_info=cfg.get_model_info(model))
    chosen = [n for (n, _), c in mapping.items() if c.w_dtype != "fp32"]
    assert len(chosen) == 14 and "lm_head" not in chosen and mapping[("lm_head", "Linear")].w_dtype == "fp32"
    cfg = MXQuantConfig()
    cfg.set_local(".*mlp.*", MXQuantConfig(w_dtype="fp32"))
    cfg.set_local(".*self_attn.*", MXQuantConfig(w_dtype="fp4"))
    mapping = cfg.to_config_mapping(model_info=cfg.get_model_info(model))
    kinds = {n: c.w_dtype for (n, _), c in mapping.items()}
    assert sorted(set(kinds.values())) == ["fp32", "fp4"] and all((k == "fp4") == ("self_attn" in n) for n, k in kinds.items())


def test_entry_is_registered():
    from neural_compressor_amd.torch.quantization import algorithm_entry
    from neural_compressor_amd.torch.utils.utility import PRIORITY_MX_QUANT, algos_mapping

    assert algos_mapping["mx_quant"] is algorithm_entry.mx_quant_entry and isinstance(PRIORITY_MX_QUANT, int)


# ---- library ----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_exist_and_reject_bad_arguments():
    from neural_compressor_amd import _lib, ops

    lib = _lib.lib
    assert "inc_mx_quant" in _lib.SIGNATURES and "inc_mx_gemm" in _lib.SIGNATURES and _lib.ABI_VERSION == lib.inc_abi_version()
    assert (ops.MX_FP8_E4M3, ops.MX_FP4_E2M1, ops.MX_KTILE) == (C.FP8, C.FP4, C.KTILE) and ops.mx_padded_k(200) == C.padded_k(200) == 256
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr()
    assert p % 16 == 0
    assert lib.inc_mx_quant(None, _lib.INC_F32, 1, 32, 128, C.FP8, p, p, None) == -1
    assert lib.inc_mx_quant(p, _lib.INC_F32, 1, 32, 128, C.FP8, None, p, None) == -1
    assert lib.inc_mx_quant(p, _lib.INC_F32, 1, 32, 128, C.FP8, p, None, None) == -1
    assert lib.inc_mx_quant(p, _lib.INC_F32, 0, 32, 128, C.FP8, p, p, None) == -1
    assert lib.inc_mx_quant(p, _lib.INC_F32, 1, 200, 128, C.FP8, p, p, None) == -1            # Kp < K
    assert lib.inc_mx_quant(p, _lib.INC_F32, 1, 32, 96, C.FP8, p, p, None) == -2              # Kp not a tile multiple
    assert lib.inc_mx_quant(p, _lib.INC_F32, 1, 32, 128, 2, p, p, None) == -2                 # fp6: unknown here
    assert lib.inc_mx_quant(p, 7, 1, 32, 128, C.FP8, p, p, None) == -2
    assert lib.inc_mx_quant(p, _lib.INC_F32, 1, 32, 128, C.FP8, p + 4, p, None) == -1         # codes not 16-byte aligned
    g = (p, p, C.FP8, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 128, None)
    for i in (0, 1, 3, 4, 7):
        assert lib.inc_mx_gemm(*[None if j == i else a for j, a in enumerate(g)]) == -1
    assert lib.inc_mx_gemm(p, p, C.FP8, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 96, None) == -2
    assert lib.inc_mx_gemm(p, p, C.FP4, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 128, None) == -2
    assert lib.inc_mx_gemm(p, p, 1, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 128, None) == -2
    assert lib.inc_mx_gemm(p, p, C.FP8, p, p, C.FP8, None, p, _lib.INC_F32, 1, 1, 128, None) == -2
    assert lib.inc_mx_gemm(p, p, C.FP8, p, p, C.FP8, None, p, _lib.INC_BF16, 0, 1, 128, None) == -1
    assert lib.inc_mx_gemm(p + 4, p, C.FP8, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 128, None) == -1
    assert lib.inc_mx_gemm(p, p + 2, C.FP8, p, p, C.FP8, None, p, _lib.INC_BF16, 1, 1, 128, None) == -1


def test_module_needs_a_hip_device():
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear

    with pytest.raises(RuntimeError, match="HIP device"):
        MXLinear(64, 64, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        MXLinear.from_float(torch.nn.Linear(64, 64), device="cpu")
