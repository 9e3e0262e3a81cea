"""fused_forward.FusedForward.around: what it substitutes, what it leaves alone and that it puts everything back (no GPU: the three op
wrappers are replaced by their eager formulas, so the plumbing is what is under test; tests/test_gpu_fused_forward.py has the kernels)."""

import logging

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers.models.llama import modeling_llama  # noqa: E402
from transformers.models.llama.configuration_llama import LlamaConfig  # noqa: E402

from neural_compressor_amd import _lib  # noqa: E402
from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff  # noqa: E402

ORIG_ROPE = modeling_llama.apply_rotary_pos_emb


def _tiny(seed=0):
    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                      vocab_size=32, max_position_embeddings=64)
    cfg._attn_implementation = "eager"
    block = modeling_llama.LlamaDecoderLayer(cfg, 0).eval()
    x = torch.randn(2, 8, 64)
    pos = torch.arange(8).unsqueeze(0)
    cos, sin = modeling_llama.LlamaRotaryEmbedding(cfg)(x, pos)
    return block, x, {"position_embeddings": (cos, sin), "attention_mask": None}


def _run(block, x, kw):
    with torch.no_grad():
        out = block(x, **kw)
    return out[0] if isinstance(out, tuple) else out


@pytest.fixture
def eager_ops(monkeypatch):
    """The op wrappers answer with eager's formulas, and count their calls."""
    calls = {"silu_mul": 0, "rmsnorm": 0, "rope": 0}

    def silu_mul(g, u):
        calls["silu_mul"] += 1
        return torch.nn.functional.silu(g) * u

    def rmsnorm(x, w, eps):
        calls["rmsnorm"] += 1
        h = x.to(torch.float32)
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
        return w * h.to(x.dtype)

    def rope(q, k, cos, sin):
        calls["rope"] += 1
        return ORIG_ROPE(q, k, cos, sin)

    monkeypatch.setattr(ff, "silu_mul", silu_mul)
    monkeypatch.setattr(ff, "rmsnorm", rmsnorm)
    monkeypatch.setattr(ff, "rope", rope)
    monkeypatch.delenv(ff.ENV_SWITCH, raising=False)
    return calls


def _unpatched(block):
    return modeling_llama.apply_rotary_pos_emb is ORIG_ROPE and not any("forward" in m.__dict__ for m in block.modules())


def test_substitutes_inside_and_restores(eager_ops):
    block, x, kw = _tiny()
    ref = _run(block, x, kw)
    state = ff.FusedForward()
    with state.around(block):
        assert "forward" in block.input_layernorm.__dict__ and "forward" in block.post_attention_layernorm.__dict__
        assert "forward" in block.mlp.__dict__
        assert modeling_llama.apply_rotary_pos_emb is ff._rope_entry
        out = _run(block, x, kw)
    assert _unpatched(block)
    assert torch.equal(out, ref)
    assert eager_ops == {"silu_mul": 1, "rmsnorm": 2, "rope": 1}
    assert not state.disabled and len(state.verified) == 3 and state.fused_calls == 4
    # a second forward of the same shapes is answered without the probe's eager twin
    with state.around(block):
        assert torch.equal(_run(block, x, kw), ref)
    assert state.fused_calls == 8 and len(state.verified) == 3 and _unpatched(block)


def test_hooks_fire_in_eager_order_and_exception_restores(eager_ops):
    block, x, kw = _tiny()
    fired = []

    class Stop(Exception):
        pass

    def note(name, stop=False):
        def hook(mod, args):
            fired.append(name)
            if stop:
                raise Stop

        return hook

    handles = [block.mlp.gate_proj.register_forward_pre_hook(note("gate")), block.mlp.up_proj.register_forward_pre_hook(note("up")),
               block.mlp.down_proj.register_forward_pre_hook(note("down", stop=True)),
               block.input_layernorm.register_forward_pre_hook(note("norm"))]
    with pytest.raises(Stop):
        with ff.FusedForward().around(block):
            _run(block, x, kw)
    assert fired == ["norm", "gate", "up", "down"]  # the norm's own __call__ (and its hooks) stay; gate, up, down as eager orders them
    assert _unpatched(block)
    for h in handles:
        h.remove()


def test_leaves_everything_else_alone(eager_ops, monkeypatch):
    block, x, kw = _tiny()

    class MyNorm(modeling_llama.LlamaRMSNorm):
        pass

    sub = MyNorm(64)
    block.post_attention_layernorm = sub
    with ff.FusedForward().around(block):
        assert "forward" not in sub.__dict__ and "forward" in block.input_layernorm.__dict__
    # a block of another family: nothing is touched, the module global included
    other = torch.nn.Sequential(torch.nn.LayerNorm(64), torch.nn.Linear(64, 64))
    with ff.FusedForward().around(other):
        assert modeling_llama.apply_rotary_pos_emb is ORIG_ROPE and _unpatched(other)
    # a module that already carries an instance-level forward is not the HF object any more
    block2, x2, kw2 = _tiny()
    mine = lambda h: h  # noqa: E731
    block2.input_layernorm.forward = mine
    with ff.FusedForward().around(block2):
        assert block2.input_layernorm.forward is mine
    assert block2.input_layernorm.forward is mine
    # a rotary function somebody else replaced stays theirs
    theirs = lambda *a, **k: ORIG_ROPE(*a, **k)  # noqa: E731
    monkeypatch.setattr(modeling_llama, "apply_rotary_pos_emb", theirs)
    with ff.FusedForward().around(block):
        assert modeling_llama.apply_rotary_pos_emb is theirs
    assert modeling_llama.apply_rotary_pos_emb is theirs
    # the switch
    monkeypatch.setattr(modeling_llama, "apply_rotary_pos_emb", ORIG_ROPE)
    monkeypatch.setenv(ff.ENV_SWITCH, "0")
    block3, x3, kw3 = _tiny()
    with ff.FusedForward().around(block3):
        assert _unpatched(block3)
        _run(block3, x3, kw3)
    assert eager_ops == {"silu_mul": 0, "rmsnorm": 0, "rope": 0}


def test_cpu_tensors_run_eager(monkeypatch):
    """The real wrappers: tensors that are not on the device are never handed to the library."""
    monkeypatch.delenv(ff.ENV_SWITCH, raising=False)
    block, x, kw = _tiny()
    ref = _run(block, x, kw)
    state = ff.FusedForward()
    with state.around(block):
        out = _run(block, x, kw)
    assert torch.equal(out, ref) and state.fused_calls == 0 and not state.verified and not state.disabled
    block16 = block.to(torch.bfloat16)
    kw16 = {"position_embeddings": tuple(t.to(torch.bfloat16) for t in kw["position_embeddings"]), "attention_mask": None}
    ref16 = _run(block16, x.to(torch.bfloat16), kw16)
    with state.around(block16):
        out16 = _run(block16, x.to(torch.bfloat16), kw16)
    assert torch.equal(out16, ref16) and state.fused_calls == 0


def test_probe_mismatch_disables_with_one_warning(eager_ops, monkeypatch, caplog):
    block, x, kw = _tiny()
    ref = _run(block, x, kw)
    monkeypatch.setattr(ff, "silu_mul", lambda g, u: torch.nn.functional.silu(g) * u + 1.0)  # a kernel that is wrong
    state = ff.FusedForward()
    logger = logging.getLogger("neural_compressor_amd")
    logger.addHandler(caplog.handler)
    try:
        with caplog.at_level(logging.WARNING):
            with state.around(block):
                out = _run(block, x, kw)
            with state.around(block):
                assert _unpatched(block)  # off for the rest of the run
                out2 = _run(block, x, kw)
    finally:
        logger.removeHandler(caplog.handler)
    assert torch.equal(out, ref) and torch.equal(out2, ref)  # the probing forward handed on eager's values
    assert state.disabled
    warnings = [r for r in caplog.records if "fused forward" in r.getMessage()]
    assert len(warnings) == 1 and "SiLU-mul" in warnings[0].getMessage()


def test_entry_points_reject_null_pointers_without_a_gpu():
    import ctypes

    lib = _lib.lib
    strides = (ctypes.c_int64 * 12)(*([8] * 12))
    assert lib.inc_fwd_silu_mul(None, None, None, 16, _lib.INC_BF16, None) == -1
    assert lib.inc_fwd_silu_mul(16, 16, 16, 0, _lib.INC_BF16, None) == -1
    assert lib.inc_fwd_rope(None, None, None, None, None, None, 1, 1, 1, 1, 16, strides, 1, _lib.INC_BF16, None) == -1
    assert lib.inc_fwd_rope(16, 16, 16, 16, 16, 16, 1, 1, 1, 1, 16, None, 1, _lib.INC_BF16, None) == -1
    assert lib.inc_fwd_rope(16, 16, 16, 16, 16, 16, 2, 1, 1, 1, 16, strides, 3, _lib.INC_BF16, None) == -1  # cos batch neither 1 nor B
    assert lib.inc_fwd_rmsnorm(None, None, None, 8, 256, 1e-6, _lib.INC_BF16, None) == -1
    assert lib.inc_fwd_rmsnorm(16, 16, 16, 8, 0, 1e-6, _lib.INC_BF16, None) == -1
    # what the kernels do not take is declined before any launch, so the caller runs eager
    assert lib.inc_fwd_silu_mul(16, 16, 16, 16, _lib.INC_F32, None) == -2
    assert lib.inc_fwd_rope(16, 16, 16, 16, 16, 16, 1, 1, 1, 1, 24, strides, 1, _lib.INC_BF16, None) == -2
    assert lib.inc_fwd_rmsnorm(16, 16, 16, 7, 4096, 1e-6, _lib.INC_BF16, None) == -2
    assert lib.inc_fwd_rmsnorm(16, 16, 16, 2048, 128, 1e-6, _lib.INC_BF16, None) == -2
