"""CPU: the FP8 per-token / per-channel cell without a GPU -- the config surface, the argument validation of the three entry points
(it runs before any HIP call), the modules' refusal of a CPU device, and the oracle's own check against torch's e4m3 cast."""

import pytest
import torch

from tests import fp8_cases as C
from tests.model_zoo import tiny_llama


def test_config_defaults():
    from neural_compressor_amd.common.utils import FP8_QUANT
    from neural_compressor_amd.torch.quantization import FP8Config, get_default_fp8_config

    d = get_default_fp8_config()
    assert isinstance(d, FP8Config) and d.name == FP8_QUANT == "fp8_quant"
    assert (d.fp8_config, d.act_granularity, d.w_granularity, d.dynamic_quantization, d.quant_lm_head) == (
        "E4M3", "per_token", "per_channel", True, False)
    assert not hasattr(d, "quant_experts")


@pytest.mark.parametrize("kw, names", [
    (dict(fp8_config="E5M2"), "fp8_config"),
    (dict(dynamic_quantization=False), "dynamic_quantization"),
    (dict(act_granularity="per_tensor"), "act_granularity"),
    (dict(w_granularity="per_tensor"), "w_granularity"),
    (dict(act_granularity="per_channel", w_granularity="per_token"), "act_granularity.*w_granularity"),
], ids=["e5m2", "static", "act_per_tensor", "w_per_tensor", "swapped"])
def test_config_rejects_what_is_not_built(kw, names):
    from neural_compressor_amd.torch.quantization import FP8Config

    with pytest.raises(NotImplementedError, match="FP8 on MI355X: .*" + names):
        FP8Config(**kw)


def test_config_mapping_of_tiny_llama():
    from neural_compressor_amd.torch.quantization import FP8Config

    model = tiny_llama(dtype=torch.float16)
    cfg = FP8Config()
    mapping = cfg.to_config_mapping(model_info=cfg.get_model_info(model))
    chosen = [n for (n, _), c in mapping.items() if c.fp8_config != "fp32"]
    assert len(chosen) == 14 and "lm_head" not in chosen and mapping[("lm_head", "Linear")].fp8_config == "fp32"
    cfg = FP8Config(quant_lm_head=True)
    mapping = cfg.to_config_mapping(model_info=cfg.get_model_info(model))
    assert mapping[("lm_head", "Linear")].fp8_config == "E4M3"
    cfg = FP8Config()
    cfg.set_local(".*mlp.*", FP8Config(fp8_config="fp32"))
    mapping = cfg.to_config_mapping(model_info=cfg.get_model_info(model))
    kinds = {n: c.fp8_config for (n, _), c in mapping.items()}
    assert all((k == "E4M3") == ("self_attn" in n) for n, k in kinds.items())


def test_entry_is_registered_and_exported():
    import neural_compressor_amd.torch.quantization as Q
    from neural_compressor_amd.torch.algorithms import fp8_quant
    from neural_compressor_amd.torch.utils.utility import algos_mapping

    assert "fp8_quant" in algos_mapping
    assert "FP8Config" in Q.__all__ and "get_default_fp8_config" in Q.__all__
    assert sorted(fp8_quant.__all__) == ["FP8Linear", "FP8Quantizer", "load", "save"]


def test_entry_points_validate_their_arguments():
    """Null pointers and sizes <= 0 are INC_ERR_BAD_ARG (-1), what is not built INC_ERR_UNSUPPORTED (-2); fake non-null pointers are
    never dereferenced because every check runs before any HIP call."""
    from neural_compressor_amd import _lib

    L = _lib.lib
    p = 4096  # a non-null, 16-byte aligned "pointer"
    BF16, F16, F32 = _lib.INC_BF16, _lib.INC_F16, _lib.INC_F32
    # quantiser
    assert L.inc_fp8_quant_rows(None, BF16, 1, 128, 128, None, p, p, None) == -1
    assert L.inc_fp8_quant_rows(p, BF16, 1, 128, 128, None, None, p, None) == -1
    assert L.inc_fp8_quant_rows(p, BF16, 1, 128, 128, None, p, None, None) == -1
    assert L.inc_fp8_quant_rows(p, BF16, 0, 128, 128, None, p, p, None) == -1
    assert L.inc_fp8_quant_rows(p, BF16, 1, 0, 128, None, p, p, None) == -1
    assert L.inc_fp8_quant_rows(p, BF16, 1, 129, 128, None, p, p, None) == -1      # Kp < K
    assert L.inc_fp8_quant_rows(p, BF16, 1, 128, 128, None, p + 8, p, None) == -1  # codes not 16-byte aligned
    assert L.inc_fp8_quant_rows(p, BF16, 1, 100, 192, None, p, p, None) == -2
    assert L.inc_fp8_quant_rows(p, 77, 1, 128, 128, None, p, p, None) == -2
    # products: (xq, row_scale, wq, alpha, bias, y, ydtype, M, N, Kp, stream)
    for fn in (L.inc_fp8_gemm, L.inc_fp8_gemv):
        for hole in range(6):
            if hole == 4:
                continue  # bias may be NULL
            args = [p, p, p, p, None, p]
            args[hole] = None
            assert fn(*args, BF16, 1, 4, 128, None) == -1
        assert fn(p, p, p, p, None, p, BF16, 0, 4, 128, None) == -1
        assert fn(p, p, p, p, None, p, BF16, 1, 0, 128, None) == -1
        assert fn(p, p, p, p, None, p, BF16, 1, 4, 0, None) == -1
        assert fn(p, p, p, p, None, p, BF16, 1, 4, -128, None) == -1
        assert fn(p, p, p, p, None, p, BF16, 1, 4, 192, None) == -2
        assert fn(p, p, p, p, None, p, F32, 1, 4, 128, None) == -2
        assert fn(p + 8, p, p, p, None, p, F16, 1, 4, 128, None) == -1             # codes not 16-byte aligned
    assert L.inc_fp8_gemv(p, p, p, p, None, p, BF16, 17, 4, 128, None) == -2
    assert L.inc_fp8_gemv(p, p, p, p, None, p, F16, 17, 4, 192, None) == -2


def test_modules_and_ops_refuse_a_cpu_device():
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear

    with pytest.raises(RuntimeError, match="needs a HIP device"):
        FP8Linear(128, 8, device="cpu")
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        FP8Linear.from_float(torch.nn.Linear(128, 8), device="cpu")
    with pytest.raises(RuntimeError, match="HBM"):
        ops.fp8_quant_rows(torch.zeros(2, 16))
    z8, zf = torch.zeros(2, 128, dtype=torch.uint8), torch.ones(2)
    for product in (ops.fp8_gemm, ops.fp8_gemv):
        with pytest.raises(RuntimeError, match="HBM"):
            product(z8, zf, z8, zf, None, torch.bfloat16)


def test_oracle_codes_are_torchs_e4m3_cast():
    """The oracle's element rounding against torch's own float -> float8_e4m3fn conversion (round to nearest even, which turns values
    beyond the format into NaN -- hence the clamp, which is the specification's saturation)."""
    dense = torch.arange(-500 * 64 + 1, 500 * 64, dtype=torch.float64) / 64                    # step 2^-6 over (-500, 500)
    small = torch.arange(-2048, 2049, dtype=torch.float64) * 2.0 ** -14                        # step 2^-14 over the subnormals, ties included
    v = torch.cat([dense, small, torch.tensor(C.FP8_TIES, dtype=torch.float64), -torch.tensor(C.FP8_TIES, dtype=torch.float64)])
    assert float(v.min()) >= -500 and float(v.max()) <= 500                                     # FP8_TIES ends at 500 itself
    _, mag = C.round_to_format(v, C.FP8)
    code = (mag | (torch.signbit(v).to(torch.int32) * 0x80)).to(torch.uint8)
    want = v.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(code, want)
    assert int((code & 0x7F).max()) == 0x7E                                                      # no NaN code
    ties = torch.tensor(C.FP8_TIES, dtype=torch.float64)
    assert torch.equal(C.code_table(C.FP8)[C.round_to_format(ties, C.FP8)[1].long()], torch.tensor(C.FP8_TIES_TO, dtype=torch.float64))


def test_oracle_quantiser_follows_the_specification():
    """Scale rule, floor, padding, signs and the ties row, on the oracle itself."""
    x = torch.tensor([[0.0, -0.0, 0.0], [448.0, -1.0, 0.5], [3.0, -6.0, 1.5]])
    q, s = C.quant_rows(x)
    assert q.shape == (3, 128) and torch.equal(s, torch.tensor([2.0 ** -60, 1.0, torch.tensor(6.0) / 448]))
    assert q[0, :3].tolist() == [0x00, 0x80, 0x00] and int(q[:, 3:].max()) == 0
    assert q[1, :3].tolist() == [0x7E, 0xB8, 0x30] and q[2, 1] == 0xFE
    for j in (-20, 0, 7):
        row, to = C.ties_row(j)
        q, s = C.quant_rows(row[None, :])
        assert float(s[0]) == 2.0 ** j and torch.equal(C.code_table(C.FP8)[q[0].long()], to)
        assert torch.equal(q[0] >> 7, torch.signbit(row).to(torch.uint8))
    sc = C.in_scale_for(600)
    xa = C.quant_input(3, 600, torch.bfloat16)
    qa, sa = C.quant_rows(xa, sc)
    qb, sb = C.quant_rows(xa.float() * sc[None, :])
    assert torch.equal(qa, qb) and torch.equal(sa, sb)
    rel = (C.dequant(qa, sa)[:, :600] - (xa.float() * sc).double()).abs().max() / (xa.float() * sc).abs().max()
    assert float(rel) <= 2.0 ** -4                                                                # half a step of 3 mantissa bits at the top binade
