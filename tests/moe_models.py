"""Tiny transformers MoE models (fused `*Experts` modules) for the MoE experts tests."""

import torch


def _build(config_cls, model_cls, seed, dtype, **kw):
    torch.manual_seed(seed)
    cfg = config_cls(vocab_size=128, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                     max_position_embeddings=128, **kw)
    m = model_cls(cfg).to(dtype).eval()
    with torch.no_grad():  # experts initialised like the rest of the model, whatever the library's own init does with 3-D parameters
        for mod in m.modules():
            for name in ("gate_up_proj", "down_proj"):
                p = getattr(mod, name, None)
                if isinstance(p, torch.nn.Parameter) and p.dim() == 3:
                    p.normal_(0.0, 0.05)
    return m


def tiny_mixtral(seed=0, dtype=torch.float32):
    from transformers import MixtralConfig, MixtralForCausalLM

    return _build(MixtralConfig, MixtralForCausalLM, seed, dtype, intermediate_size=128, num_local_experts=4, num_experts_per_tok=2)


def tiny_qwen3_moe(seed=0, dtype=torch.float32):
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM

    return _build(Qwen3MoeConfig, Qwen3MoeForCausalLM, seed, dtype, intermediate_size=128, moe_intermediate_size=64, num_experts=8,
                  num_experts_per_tok=2, head_dim=16, decoder_sparse_step=1, mlp_only_layers=[])


def tiny_olmoe(seed=0, dtype=torch.float32):
    from transformers import OlmoeConfig, OlmoeForCausalLM

    return _build(OlmoeConfig, OlmoeForCausalLM, seed, dtype, intermediate_size=64, num_experts=4, num_experts_per_tok=2)


def tiny_gpt_oss_experts():
    from transformers import GptOssConfig
    from transformers.models.gpt_oss.modeling_gpt_oss import GptOssExperts

    cfg = GptOssConfig(vocab_size=128, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=4,
                       num_key_value_heads=2, num_local_experts=4, num_experts_per_tok=2, head_dim=16)
    return GptOssExperts(cfg)


def experts_of(model):
    from neural_compressor_amd.torch.utils.utility import is_fused_experts

    return [(n, m) for n, m in model.named_modules() if is_fused_experts(m)]
