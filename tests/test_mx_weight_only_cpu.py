"""CPU: the surface of the weight-only MX cell -- what MXQuantConfig accepts and refuses, the config mapping, the two entry points in
header / exports / bindings, and their rejections before any HIP call (so this runs without a device)."""

import ctypes
import os

import pytest
import torch

from tests import mx_cases as C
from tests.model_zoo import tiny_llama
from tests.test_mx_gemv_cpu import _host_pointer

ENTRIES = ["inc_mx_wo_gemv", "inc_mx_wo_gemm"]


@pytest.mark.parametrize("w_dtype", ["fp4", "fp8_e4m3"])
def test_config_takes_the_weight_only_pairs_only_with_the_flag(w_dtype):
    from neural_compressor_amd.torch.quantization import MXQuantConfig

    cfg = MXQuantConfig(w_dtype=w_dtype, act_dtype="bf16", weight_only=True)
    assert (cfg.w_dtype, cfg.act_dtype, cfg.weight_only) == (w_dtype, "bf16", True)
    with pytest.raises(NotImplementedError, match="weight_only=True"):
        MXQuantConfig(w_dtype=w_dtype, act_dtype="bf16")
    with pytest.raises(NotImplementedError, match='act_dtype="bf16"'):
        MXQuantConfig(w_dtype=w_dtype, act_dtype="fp8_e4m3", weight_only=True)
    with pytest.raises(NotImplementedError):
        MXQuantConfig(w_dtype="int8", act_dtype="bf16", weight_only=True)


def test_config_mapping_of_tiny_llama():
    from neural_compressor_amd.torch.quantization import MXQuantConfig

    model = tiny_llama(dtype=torch.float16)
    cfg = MXQuantConfig(w_dtype="fp4", act_dtype="bf16", weight_only=True)
    mapping = cfg.to_config_mapping(model_info=cfg.get_model_info(model))
    picked = {name: (c.w_dtype, c.act_dtype, c.weight_only) for (name, _), c in mapping.items() if c.w_dtype != "fp32"}
    assert len(picked) == 14 and set(picked.values()) == {("fp4", "bf16", True)}
    assert [c.w_dtype for (name, _), c in mapping.items() if name == "lm_head"] == ["fp32"]


def test_entry_points_are_in_header_exports_and_bindings():
    from neural_compressor_amd import _lib, ops

    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "inc_mi355x.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 and _lib.lib.inc_abi_version() == 12
    assert callable(ops.mx_wo_gemv) and callable(ops.mx_wo_gemm)


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_points_reject_what_they_do_not_take_without_a_device(entry):
    from neural_compressor_amd import _lib

    f = getattr(_lib.lib, entry)
    keep, p = _host_pointer()
    bf16, f32 = _lib.INC_BF16, _lib.INC_F32
    assert f(None, p, p, C.FP4, None, p, bf16, 1, 1, 128, 128, None) == -1                  # a NULL operand
    assert f(p, None, p, C.FP4, None, p, bf16, 1, 1, 128, 128, None) == -1
    assert f(p, p, None, C.FP4, None, p, bf16, 1, 1, 128, 128, None) == -1
    assert f(p, p, p, C.FP4, None, None, bf16, 1, 1, 128, 128, None) == -1
    assert f(p, p, p, C.FP4, None, p, bf16, 0, 1, 128, 128, None) == -1                     # M, N < 1
    assert f(p, p, p, C.FP4, None, p, bf16, 1, 0, 128, 128, None) == -1
    if entry == "inc_mx_wo_gemv":
        assert f(p, p, p, C.FP8, None, p, bf16, 17, 1, 128, 128, None) == -2                # more than 16 rows
    assert f(p, p, p, C.FP4, None, p, bf16, 1, 1, 96, 96, None) == -2                       # Kp % 128
    assert f(p, p, p, C.FP4, None, p, bf16, 1, 1, 100, 128, None) == -2                     # K % 8
    assert f(p, p, p, C.FP4, None, p, bf16, 1, 1, 256, 128, None) == -2                     # K > Kp
    assert f(p, p, p, C.FP4, None, p, bf16, 1, 1, 128, 256, None) == -2                     # Kp - K >= 128
    assert f(p, p, p, 2, None, p, bf16, 1, 1, 128, 128, None) == -2                         # an unknown format
    assert f(p, p, p, C.FP8, None, p, f32, 1, 1, 128, 128, None) == -2                      # an fp32 y
    del keep
