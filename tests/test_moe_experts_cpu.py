"""CPU: the fused MoE experts feature without a GPU -- argument validation of the K4e entry points (every rejection happens before any
HIP call; nothing is launched), detection of transformers' fused `*Experts` modules, and the configs' op mappings."""

import pytest

from tests.moe_models import experts_of, tiny_gpt_oss_experts, tiny_mixtral, tiny_olmoe, tiny_qwen3_moe

BF16, F16, F32 = 2, 1, 0
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
FAKE = 1 << 20  # a 16-byte aligned address that is never dereferenced


@pytest.fixture(scope="module")
def L():
    from neural_compressor_amd import _lib

    return _lib.lib


def _gemm(L, mode=0, a=FAKE, xdtype=BF16, route=FAKE, qweight=FAKE, scales=FAKE, qzeros=FAKE, rw=None, wdt=F32, out=FAKE, T=1, k=2, E=8,
          N=2 * 14336, K=4096, G=32, gs=128, ws=None, ws_bytes=0):
    return L.inc_woq_moe_gemm(mode, a, xdtype, route, qweight, scales, qzeros, rw, wdt, out, T, k, E, N, K, G, gs, ws, ws_bytes, None)


def test_route_validation(L):
    assert L.inc_moe_route(None, 8, 1, 2, 8, FAKE, 1 << 20, None) == BAD_ARG
    assert L.inc_moe_route(FAKE, 8, 1, 2, 8, None, 1 << 20, None) == BAD_ARG
    assert L.inc_moe_route(FAKE, 2, 1, 2, 8, FAKE, 1 << 20, None) == BAD_ARG  # int16 ids
    assert L.inc_moe_route(FAKE, 8, 0, 2, 8, FAKE, 1 << 20, None) == BAD_ARG
    assert L.inc_moe_route(FAKE, 8, 1, 2, 513, FAKE, 1 << 20, None) == UNSUPPORTED  # more experts than the route kernel holds
    need = L.inc_moe_route_bytes(1, 2, 8)
    assert need > 0 and L.inc_moe_route_bytes(0, 2, 8) == 0
    assert L.inc_moe_route(FAKE, 8, 1, 2, 8, FAKE, need - 4, None) == WORKSPACE


def test_gemm_validation(L):
    W = L.inc_woq_moe_gemm_workspace_bytes
    ws = W(0, 1, 2, 8, 2 * 14336, 4096)
    assert ws > 0  # decode: split-K over the K range
    assert _gemm(L, mode=3) == BAD_ARG
    assert _gemm(L, a=None) == BAD_ARG and _gemm(L, route=None) == BAD_ARG and _gemm(L, qzeros=None) == BAD_ARG
    assert _gemm(L, mode=1, N=4096, K=14336, G=112) == BAD_ARG  # down needs routing weights
    assert _gemm(L, G=31, ws=FAKE, ws_bytes=ws) == BAD_ARG  # G must be K / group_size
    assert _gemm(L, xdtype=F32, ws=FAKE, ws_bytes=ws) == UNSUPPORTED
    assert _gemm(L, gs=48, G=86, ws=FAKE, ws_bytes=ws) == UNSUPPORTED  # groups: powers of two >= 32
    assert _gemm(L, K=4080, G=255, gs=16, ws=FAKE, ws_bytes=ws) == UNSUPPORTED  # K % 32 != 0
    assert _gemm(L, E=1024, ws=FAKE, ws_bytes=ws) == UNSUPPORTED
    assert _gemm(L, a=FAKE + 2, ws=FAKE, ws_bytes=ws) == UNSUPPORTED and _gemm(L, qweight=FAKE + 8, ws=FAKE, ws_bytes=ws) == UNSUPPORTED
    assert _gemm(L) == WORKSPACE and _gemm(L, ws=FAKE, ws_bytes=ws - 4) == WORKSPACE
    assert W(0, 4096, 2, 8, 2 * 14336, 4096) == 0  # prefill: enough tiles, no split
    assert W(3, 1, 2, 8, 1024, 1024) == 0 and W(0, 0, 2, 8, 1024, 1024) == 0


def test_combine_validation(L):
    assert L.inc_moe_combine(None, FAKE, FAKE, BF16, 1, 2, 8, 4096, None) == BAD_ARG
    assert L.inc_moe_combine(FAKE, FAKE, FAKE, F32, 1, 2, 8, 4096, None) == UNSUPPORTED
    assert L.inc_moe_combine(FAKE, FAKE, FAKE, BF16, 1, 2, 8, 4098, None) == UNSUPPORTED


@pytest.mark.parametrize("make", [tiny_mixtral, tiny_qwen3_moe, tiny_olmoe])
def test_fused_experts_detected(make):
    found = experts_of(make())
    assert [n for n, _ in found] == ["model.layers.0.mlp.experts", "model.layers.1.mlp.experts"]


def test_gpt_oss_and_dense_modules_rejected():
    import torch

    from neural_compressor_amd.torch.utils.utility import is_fused_experts

    assert not is_fused_experts(tiny_gpt_oss_experts())  # transposed [E, H, 2I] with biases
    assert not is_fused_experts(torch.nn.Linear(8, 8))
    m = tiny_mixtral()
    assert not any(is_fused_experts(x) for x in (m.model.layers[0].mlp, m.model.layers[0].mlp.gate, m.model.layers[0].self_attn))


@pytest.mark.parametrize("make", [tiny_mixtral, tiny_qwen3_moe])
def test_config_mappings(make):
    from neural_compressor_amd.torch.quantization import AWQConfig, GPTQConfig, RTNConfig
    from neural_compressor_amd.torch.quantization.config import TorchBaseConfig

    model = make()
    linears = TorchBaseConfig.get_model_info(model)
    experts = [(n, type(m).__name__) for n, m in experts_of(model)]
    assert experts and not set(experts) & set(linears)
    rtn = RTNConfig(bits=4, group_size=32)
    info = rtn.get_model_info(model)
    assert set(info) == set(linears) | set(experts)
    mapping = rtn.to_config_mapping(model_info=info)
    assert all(mapping[e].dtype == "int" for e in experts)
    # opt out by name or by op type
    off = RTNConfig(bits=4, group_size=32).set_local(".*experts", RTNConfig(dtype="fp32"))
    assert all(off.to_config_mapping(model_info=info)[e].dtype == "fp32" for e in experts)
    off = RTNConfig(bits=4, group_size=32).set_local(type(experts_of(model)[0][1]), RTNConfig(dtype="fp32"))
    assert all(off.to_config_mapping(model_info=info)[e].dtype == "fp32" for e in experts)
    # GPTQ / AWQ see what they saw before: the Linear modules only
    assert GPTQConfig.get_model_info(model) == linears
    assert AWQConfig.get_model_info(model) == linears
