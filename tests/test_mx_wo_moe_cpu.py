"""CPU: the surface of the weight-only MX experts -- the two routed entry points in header / exports / bindings, their rejections
before any HIP call, the config mapping with and without quant_experts, and the comparable share of the random mode-0 reference."""

import ctypes
import math
import os

import pytest
import torch

from tests import moe_models
from tests import mx_cases as C
from tests import mx_gpt_oss_cases as G
from tests import mx_moe_cases as M

ENTRIES = ["inc_mx_wo_moe_gemm", "inc_mx_wo_moe_gemm_glu"]


def test_entry_points_are_in_header_exports_and_bindings():
    from neural_compressor_amd import _lib, ops
    from neural_compressor_amd.torch.algorithms import mx_quant

    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "inc_mi355x.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 and _lib.lib.inc_abi_version() == 12
    assert callable(ops.mx_wo_moe_gemm) and callable(ops.mx_wo_moe_gemm_glu)
    assert {"MXWeightOnlyExperts", "MXWeightOnlyGptOssExperts"} <= set(mx_quant.__all__)


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_points_reject_what_they_do_not_take_without_a_device(entry):
    from neural_compressor_amd import _lib

    glu = entry.endswith("_glu")
    one = 16  # any non-NULL, 16-byte aligned address: rejected calls never touch it
    ok = dict(mode=2, x=one, route=one, wq=one, ws=one, wfmt=C.FP4, bias=one, alpha=1.702, limit=7.0, rw=None, wdt=_lib.INC_F32, out=one,
              odt=_lib.INC_F32, T=4, k=2, E=4, N=16, K=128, Kp=128)

    def call(**kw):
        a = dict(ok, **kw)
        epi = (a["bias"], a["alpha"], a["limit"]) if glu else ()
        return getattr(_lib.lib, entry)(a["mode"], a["x"], a["route"], a["wq"], a["ws"], a["wfmt"], *epi, a["rw"], a["wdt"], a["out"],
                                        a["odt"], a["T"], a["k"], a["E"], a["N"], a["K"], a["Kp"], None)

    bf16, f16 = _lib.INC_BF16, _lib.INC_F16
    bad = [dict(mode=3), dict(mode=-1), dict(x=None), dict(route=None), dict(wq=None), dict(ws=None), dict(out=None), dict(T=0), dict(k=0),
           dict(E=0), dict(N=0), dict(K=0), dict(Kp=0), dict(mode=1, rw=None), dict(x=24), dict(wq=24)]
    unsupported = [dict(wfmt=2), dict(wfmt=1), dict(K=96, Kp=96), dict(K=100), dict(K=256), dict(Kp=256), dict(E=513), dict(T=1 << 22),
                   dict(mode=0, N=15, odt=bf16), dict(mode=0, odt=f16), dict(mode=0, odt=_lib.INC_F32), dict(odt=bf16),
                   dict(mode=1, rw=one, odt=f16), dict(mode=1, rw=one, wdt=7)]
    if glu:
        bad += [dict(limit=0.0), dict(limit=-7.0), dict(limit=math.nan), dict(alpha=math.nan), dict(bias=18)]
        unsupported += [dict(bias=None, Kp=256), dict(limit=math.inf, Kp=256)]   # a NULL bias and limit = +inf pass the argument checks
    for kw in bad:
        assert call(**kw) == -1, kw
    for kw in unsupported:
        assert call(**kw) == -2, kw


def test_config_maps_the_experts_only_with_quant_experts():
    from neural_compressor_amd.torch.algorithms.mx_quant.experts import unsupported_reason
    from neural_compressor_amd.torch.quantization import MXQuantConfig
    from neural_compressor_amd.torch.quantization.quantize import _model_info

    with torch.device("meta"):
        models = [(moe_models.tiny_qwen3_moe(), moe_models.experts_of), (G.tiny_gpt_oss(), G.gpt_oss_experts_of)]
    for model, experts_of in models:
        experts, base, picked = [(n, type(m).__name__) for n, m in experts_of(model)], MXQuantConfig.get_model_info(model), {}
        for flag in (True, False):
            cfg = MXQuantConfig(w_dtype="fp4", act_dtype="bf16", weight_only=True, quant_experts=flag)
            mapping = cfg.to_config_mapping(model_info=_model_info(cfg, model))
            picked[flag] = {key: (c.w_dtype, c.act_dtype, c.weight_only) for key, c in mapping.items() if c.w_dtype != "fp32"}
        assert len(experts) == 2 and all(picked[True][e] == ("fp4", "bf16", True) for e in experts)
        assert set(picked[False]) == set(picked[True]) - set(experts) == set(base) - {("lm_head", "Linear")}
        for _, m in experts_of(model):
            assert unsupported_reason(m, dict(w_dtype="fp4", act_dtype="bf16", weight_only=True)) is None
            assert "not one of" in unsupported_reason(m, dict(w_dtype="fp4", act_dtype="bf16"))
            assert "not one of" in unsupported_reason(m, dict(w_dtype="fp4", act_dtype="fp8_e4m3", weight_only=True))


@pytest.mark.parametrize("wfmt", [C.FP4, C.FP8], ids=["fp4", "fp8"])
def test_random_mode0_reference_has_enough_outputs_bf16_can_hold(wfmt):
    d = M.random_case(0, C.FP8, wfmt)
    assert torch.equal(d["ad"].bfloat16().double(), d["ad"])                 # the activations of the GPU test are exact in bf16
    _, _, ok = M.random_gate(d, torch.bfloat16)
    assert float(ok.double().mean()) >= 0.5
