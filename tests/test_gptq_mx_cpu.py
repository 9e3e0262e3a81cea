"""CPU: what GPTQ on the MX grid refuses, and the argument checks of its two entry points (decided before any HIP call)."""

import pytest

CFG = {"dtype": "mx_fp4", "group_size": 32}


@pytest.mark.parametrize("kwargs", [dict(group_size=128), dict(act_order=True), dict(hybrid_order=True), dict(static_groups=True),
                                    dict(use_mse_search=True), dict(use_double_quant=True), dict(quant_experts=True)],
                         ids=lambda kw: next(iter(kw)))
@pytest.mark.parametrize("dtype", ["mx_fp4", "mx_fp8_e4m3"])
def test_unsupported_configurations_raise_at_prepare(dtype, kwargs):
    from neural_compressor_amd.torch.quantization import GPTQConfig, prepare
    from tests.model_zoo import tiny_llama

    with pytest.raises(NotImplementedError, match="MX grid"):
        prepare(tiny_llama(layers=1), GPTQConfig(dtype=dtype, **kwargs))


@pytest.mark.parametrize("layer", [dict(columns=48), dict(columns=64, is_conv1d=True), dict(columns=64, row_sharded=True)],
                         ids=lambda kw: list(kw)[-1])
def test_unsupported_layers_raise(layer):
    from neural_compressor_amd.torch.algorithms.weight_only.gptq import GPTQ

    GPTQ.check_mx(CFG, columns=64)
    with pytest.raises(NotImplementedError, match="MX grid"):
        GPTQ.check_mx(CFG, **layer)


def test_entry_points_exist_and_check_their_arguments():
    import ctypes
    import os

    from neural_compressor_amd import _lib

    L = _lib.lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "inc_mi355x.h")).read()
    for name in ("inc_gptq_quantize_layer_mx", "inc_gptq_quant_block_mx"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert L.inc_abi_version() == 12
    p = 4096  # never dereferenced: every case below is decided before a launch
    assert L.inc_gptq_quantize_layer_mx(None, None, None, None, None, 0, None, 8, 128, 128, 4, 0, None, None) == -1
    assert L.inc_gptq_quantize_layer_mx(p, p, p, p, p, 0, p, 0, 128, 128, 4, 0, None, None) == -1     # N < 1
    assert L.inc_gptq_quantize_layer_mx(p, p, p, p, p, 0, p, 8, 128, 128, 2, 0, None, None) == -2     # fmt
    assert L.inc_gptq_quantize_layer_mx(p, p, p, p, p, 0, p, 8, 100, 128, 4, 0, None, None) == -2     # K % 32
    assert L.inc_gptq_quantize_layer_mx(p, p, p, p, p, 0, p, 8, 160, 160, 0, 0, None, None) == -2     # Kp != 256
    assert L.inc_gptq_quant_block_mx(None, None, None, None, None, 0, None, 8, 128, 128, 0, 4, None) == -1
    assert L.inc_gptq_quant_block_mx(p, p, p, p, p, 0, p, 8, 256, 256, 64, 4, None) == -1             # i1 off the 128-column grid
