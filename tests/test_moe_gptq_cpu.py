"""CPU: GPTQ on fused MoE experts without a GPU -- the K5e entry point in header / exports / bindings, the config plumbing of
`GPTQConfig(quant_experts=True)`, `gptq_unsupported_reason`, and the argument checks of the ops wrapper that raise before any launch."""

import ctypes
import os
import re
import types

import pytest
import torch

from tests.moe_models import experts_of, tiny_mixtral, tiny_olmoe, tiny_qwen3_moe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(0x1000)
BAD_ARG, UNSUPPORTED = -1, -2


def test_routed_symbol_and_abi():
    from neural_compressor_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inc_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\binc_gptq_hessian_accum_routed\s*\(", header)
    assert "inc_gptq_hessian_accum_routed" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "inc_gptq_hessian_accum_routed")
    assert _lib.ABI_VERSION == 12 and _lib.lib.inc_abi_version() == 12


def test_routed_entry_rejects_before_any_launch():
    from neural_compressor_amd import _lib

    f = _lib.lib.inc_gptq_hessian_accum_routed
    ok = dict(a=FAKE, xdtype=2, mode=0, route=FAKE, T=4, top_k=2, E=8, K=64, H=FAKE, rows=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["a"], a["xdtype"], a["mode"], a["route"], a["T"], a["top_k"], a["E"], a["K"], a["H"], a["rows"], None)

    for kw in (dict(a=None), dict(route=None), dict(H=None), dict(rows=None), dict(T=0), dict(top_k=0), dict(E=0), dict(K=0), dict(mode=2)):
        assert call(**kw) == BAD_ARG, kw
    for kw in (dict(xdtype=7), dict(E=513), dict(K=48), dict(T=1 << 22, top_k=2), dict(a=ctypes.c_void_p(0x1008)),
               dict(H=ctypes.c_void_p(0x1004))):
        assert call(**kw) == UNSUPPORTED, kw


@pytest.mark.parametrize("make", [tiny_mixtral, tiny_qwen3_moe, tiny_olmoe])
def test_config_mapping_holds_the_experts_when_asked(make):
    from neural_compressor_amd.torch.quantization import GPTQConfig
    from neural_compressor_amd.torch.quantization.config import TorchBaseConfig
    from neural_compressor_amd.torch.quantization.quantize import preprocess_quant_config

    model = make()
    linears = TorchBaseConfig.get_model_info(model)
    experts = [(n, type(m).__name__) for n, m in experts_of(model)]
    assert len(experts) == 2
    # default: what GPTQ saw before
    _, mapping = preprocess_quant_config(model, GPTQConfig(bits=4, group_size=32))
    assert set(mapping) == set(linears)
    assert GPTQConfig.get_model_info(model) == linears
    assert GPTQConfig(quant_experts=True).get_model_info(model) == linears
    # opted in: the experts carry (name, type) keys and the global settings
    on = GPTQConfig(bits=4, group_size=32, quant_experts=True)
    _, mapping = preprocess_quant_config(model, on)
    assert set(mapping) == set(linears) | set(experts)
    assert all(mapping[e].dtype == "int" and mapping[e].group_size == 32 for e in experts)
    fresh = GPTQConfig(quant_experts=True)
    assert fresh.to_dict()["quant_experts"] is True and GPTQConfig.from_dict(fresh.to_dict()).quant_experts is True
    assert GPTQConfig().quant_experts is False
    # set_local by name and by type turns them off
    off = GPTQConfig(bits=4, group_size=32, quant_experts=True).set_local(".*experts", GPTQConfig(dtype="fp32"))
    _, mapping = preprocess_quant_config(model, off)
    assert all(mapping[e].dtype == "fp32" for e in experts) and mapping[linears[0]].dtype == "int"
    off = GPTQConfig(bits=4, group_size=32, quant_experts=True).set_local(type(experts_of(model)[0][1]), GPTQConfig(dtype="fp32"))
    _, mapping = preprocess_quant_config(model, off)
    assert all(mapping[e].dtype == "fp32" for e in experts) and mapping[linears[0]].dtype == "int"


def _stub(E=4, H=256, I=512, act=None):
    return types.SimpleNamespace(gate_up_proj=torch.empty(E, 2 * I, H, device="meta"), down_proj=torch.empty(E, H, I, device="meta"),
                                 act_fn=act if act is not None else torch.nn.SiLU())


def _cfg(**kw):
    base = dict(dtype="int", bits=4, sym=True, group_size=32, mse=False, use_double_quant=False, act_order=False, hybrid_order=False,
                fp8_aware=False, static_groups=False, percdamp=0.01, block_size=128)
    base.update(kw)
    return base


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("gs", [32, 128, -1])
def test_supported_settings(sym, gs):
    from neural_compressor_amd.torch.algorithms.weight_only.experts_gptq import gptq_unsupported_reason

    assert gptq_unsupported_reason(_stub(), _cfg(sym=sym, group_size=gs)) is None
    for make in (tiny_mixtral, tiny_qwen3_moe, tiny_olmoe):
        if gs != 128:  # (H = 64 in the tiny models)
            assert gptq_unsupported_reason(experts_of(make())[0][1], _cfg(sym=sym, group_size=gs)) is None


@pytest.mark.parametrize("kw, word", [
    (dict(bits=8), "INT4"), (dict(bits=3), "INT4"), (dict(dtype="nf4"), "INT4"), (dict(group_size=48), "group_size"),
    (dict(group_size=512), "group_size"), (dict(group_size=128, _H=192), "group_size"), (dict(act_order=True), "act_order"),
    (dict(static_groups=True), "static_groups"), (dict(hybrid_order=True), "hybrid_order"), (dict(mse=True), "use_mse_search"),
    (dict(use_double_quant=True), "double"), (dict(fp8_aware=True), "fp8_aware"), (dict(_act=torch.nn.GELU()), "SiLU"),
    (dict(group_size=-1, _H=48), "multiples of 32"), (dict(_E=513), "at most 512"),
])
def test_unsupported_settings(kw, word):
    from neural_compressor_amd.torch.algorithms.weight_only.experts_gptq import gptq_unsupported_reason

    kw = dict(kw)
    mod = _stub(E=kw.pop("_E", 4), H=kw.pop("_H", 256), act=kw.pop("_act", None))
    reason = gptq_unsupported_reason(mod, _cfg(**kw))
    assert reason is not None and word in reason, reason


def test_ops_wrapper_argument_checks():
    """Everything here raises before the library is called (host tensors, no GPU)."""
    from neural_compressor_amd import ops

    E, K, T, k = 4, 64, 8, 2
    H = torch.zeros(E, K, K)
    rows = torch.zeros(E, dtype=torch.int64)
    route = torch.zeros(1024, dtype=torch.int32)
    x = torch.zeros(T, K)
    with pytest.raises(ValueError, match="H must be"):
        ops.gptq_hessian_accum_routed(H[0], rows, x, route, T, k)
    with pytest.raises(ValueError, match="H must be"):
        ops.gptq_hessian_accum_routed(H.double(), rows, x, route, T, k)
    with pytest.raises(ValueError, match="rows must be"):
        ops.gptq_hessian_accum_routed(H, rows.int(), x, route, T, k)
    with pytest.raises(ValueError, match="rows must be"):
        ops.gptq_hessian_accum_routed(H, rows[:2], x, route, T, k)
    with pytest.raises(TypeError, match="route"):
        ops.gptq_hessian_accum_routed(H, rows, x, route.long(), T, k)
    with pytest.raises(ValueError, match="positive"):
        ops.gptq_hessian_accum_routed(H, rows, x, route, 0, k)
    with pytest.raises(ValueError, match="a must be"):
        ops.gptq_hessian_accum_routed(H, rows, x, route, T, k, sorted_rows=True)  # sorted input is [T * k, K]
    with pytest.raises(ValueError, match="a must be"):
        ops.gptq_hessian_accum_routed(H, rows, torch.zeros(T, K + 32), route, T, k)
    with pytest.raises(TypeError, match="floating dtype"):
        ops.gptq_hessian_accum_routed(H, rows, x.double(), route, T, k)
    with pytest.raises(ValueError, match="route is smaller"):
        ops.gptq_hessian_accum_routed(H, rows, x, route[:4], T, k)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.gptq_hessian_accum_routed(H, rows, x, route, T, k)
