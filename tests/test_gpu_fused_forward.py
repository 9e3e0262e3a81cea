"""csrc/fwd_elementwise.hip against the eager Hugging Face code on the same device: every comparison is of bit patterns (and strides),
at the smallest shapes at which each kernel can go wrong; then GPTQ end to end with the substitution on and off."""

import logging

import pytest
import torch

from tests.model_zoo import calib_ids, tiny_llama

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _bits(t):
    return t.view(torch.int16)


def _assert_same(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    assert got.stride() == ref.stride(), f"{what}: strides {got.stride()} vs eager {ref.stride()}"
    assert torch.equal(_bits(got), _bits(ref)), f"{what}: {int((_bits(got) != _bits(ref)).sum())} elements differ"


# ---- SiLU * up ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_mul_every_gate_bit_pattern(hip, dtype):
    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    gate = torch.arange(-32768, 32768, dtype=torch.int32, device=hip).to(torch.int16).view(dtype)  # all 65 536 patterns, NaNs included
    g = torch.Generator(device="cpu").manual_seed(3)
    fi = torch.finfo(dtype)
    ups = [0.0, 1.0, -1.0, fi.smallest_normal / 4, fi.max] + torch.randn(3, generator=g).tolist()
    up = torch.tensor(ups, dtype=torch.float32).to(dtype).to(hip)
    assert float(up[3]) != 0.0  # a subnormal of the dtype
    G = gate.unsqueeze(0).expand(8, -1).contiguous()
    U = up.unsqueeze(1).expand(-1, 65536).contiguous()
    got = ff.silu_mul(G, U)
    assert got is not None
    _assert_same(got, torch.nn.functional.silu(G) * U, "silu_mul")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 11008), (5, 1001)])
def test_silu_mul_shapes(hip, dtype, shape):
    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    g = torch.Generator(device="cpu").manual_seed(5)
    a = (torch.randn(shape, generator=g) * 4).to(dtype).to(hip)
    b = (torch.randn(shape, generator=g) * 4).to(dtype).to(hip)
    got = ff.silu_mul(a, b)
    assert got is not None  # 5 * 1001 is no multiple of 8: the tail is the kernel's
    _assert_same(got, torch.nn.functional.silu(a) * b, f"silu_mul {shape}")


# ---- rotary embedding -----------------------------------------------------------------------------------------------------------
def _rope_operands(hip, dtype, B, Hq, Hk, T, D, cs_batch, model_layout, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)

    def make(H):
        x = (torch.randn(B, T, H * D, generator=g) * 3).to(dtype).to(hip)
        x = x.view(B, T, H, D).transpose(1, 2)  # the view LlamaAttention hands to apply_rotary_pos_emb
        return x if model_layout else x.contiguous()

    ang = torch.rand(cs_batch, T, D, generator=g) * 6.28
    return make(Hq), make(Hk), ang.cos().to(dtype).to(hip), ang.sin().to(dtype).to(hip)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model_layout", [True, False])
def test_rope_values_and_strides(hip, dtype, model_layout):
    from transformers.models.llama import modeling_llama

    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    n = 0
    for B in (1, 3):
        for Hq, Hk in ((4, 4), (4, 2)):
            for T in (1, 5, 130):
                for D in (64, 128):
                    for cs_batch in {1, B}:
                        q, k, cos, sin = _rope_operands(hip, dtype, B, Hq, Hk, T, D, cs_batch, model_layout, seed=n)
                        rq, rk = modeling_llama.apply_rotary_pos_emb(q, k, cos, sin)
                        got = ff.rope(q, k, cos, sin)
                        what = f"B={B} H=({Hq},{Hk}) T={T} D={D} cos batch {cs_batch}"
                        assert got is not None, what
                        _assert_same(got[0], rq, "q " + what)
                        _assert_same(got[1], rk, "k " + what)
                        n += 1
    assert n == 36


def test_rope_unsupported_head_dim_comes_back_through_eager(hip):
    from transformers.models.llama import modeling_llama

    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    q, k, cos, sin = _rope_operands(hip, torch.bfloat16, 2, 4, 2, 5, 24, 1, True, seed=7)
    assert ff.rope(q, k, cos, sin) is None
    state = ff.FusedForward()
    ff._tls.active = (state, torch.nn.Identity())
    try:
        got = ff._rope_entry(q, k, cos, sin)
    finally:
        ff._tls.active = None
    rq, rk = modeling_llama.apply_rotary_pos_emb(q, k, cos, sin)
    _assert_same(got[0], rq, "q")
    _assert_same(got[1], rk, "k")
    assert state.fused_calls == 0 and not state.disabled


# ---- RMSNorm --------------------------------------------------------------------------------------------------------------------
def _norm_rows(hip, dtype, rows, cols, seed):
    g = torch.Generator(device=hip).manual_seed(seed)
    x = torch.randn(rows, cols, generator=g, device=hip)
    x = x * torch.exp2(torch.randint(-10, 11, (rows, 1), generator=g, device=hip).float())  # per-row scales 2^-10 .. 2^10
    x = x.to(dtype)
    if rows >= 7:
        x[3] = 0  # an all-zero row
        x[5, cols // 3] = torch.finfo(dtype).max  # in bf16 its square overflows fp32
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [128, 4096, 5120, 8192])
def test_rmsnorm_bit_equal_whichever_route(hip, dtype, cols):
    from transformers.models.llama import modeling_llama

    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    g = torch.Generator(device="cpu").manual_seed(11)
    weight = (1 + 0.25 * torch.randn(cols, generator=g)).to(dtype).to(hip)
    for rows in (1, 7, 2048, 8192):
        x = _norm_rows(hip, dtype, rows, cols, seed=rows + cols)
        for eps in (1e-5, 1e-6):
            m = modeling_llama.LlamaRMSNorm(cols, eps=eps).to(hip).to(dtype)
            with torch.no_grad():
                m.weight.copy_(weight)
                ref = m(x)
                got, route = ff.rmsnorm_routed(m, x)
            what = f"rows={rows} cols={cols} eps={eps} route={route}"
            if cols == 4096 and rows >= 2048:
                assert route == "fused", what
            _assert_same(got, ref, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_model_shaped_input(hip, dtype):
    """[batch, tokens, hidden] as the block hands it over, and the fused routes on either side of torch's one-wave / eight-wave split."""
    from transformers.models.llama import modeling_llama

    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    for shape in ((4, 130, 4096), (2, 9, 256), (3, 8, 8128), (3, 8, 8136), (1, 8, 16384)):
        x = _norm_rows(hip, dtype, shape[0] * shape[1], shape[2], seed=shape[2]).view(shape)
        m = modeling_llama.LlamaRMSNorm(shape[2], eps=1e-5).to(hip).to(dtype)
        with torch.no_grad():
            m.weight.copy_((1 + 0.25 * torch.randn(shape[2])).to(dtype))
            ref = m(x)
            got, route = ff.rmsnorm_routed(m, x)
        assert route == "fused", shape
        _assert_same(got, ref, f"{shape}")


# ---- GPTQ end to end ------------------------------------------------------------------------------------------------------------
def test_gptq_is_identical_with_the_fused_forward_on_and_off(hip, monkeypatch, caplog):
    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff
    from neural_compressor_amd.torch.algorithms.weight_only import gptq as G
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear
    from neural_compressor_amd.torch.quantization import GPTQConfig, convert, prepare

    ids = calib_ids(n=8, seq=64)
    states = []

    class Recorded(ff.FusedForward):
        def __init__(self):
            super().__init__()
            states.append(self)

    monkeypatch.setattr(G, "FusedForward", Recorded)

    def run(switch):
        monkeypatch.setenv(ff.ENV_SWITCH, switch)
        del states[:]
        m = prepare(tiny_llama(hidden=256, inter=704, heads=4, layers=2, dtype=torch.bfloat16), GPTQConfig(bits=4, group_size=128))
        for x in ids:
            m(x)
        m = convert(m)
        mods = {n: mod for n, mod in m.named_modules() if isinstance(mod, MI355XWeightOnlyLinear)}
        with torch.no_grad():
            hidden = m(ids[0].to(hip), output_hidden_states=True).hidden_states[-1]
        return mods, hidden, list(states)

    logger = logging.getLogger("neural_compressor_amd")
    logger.addHandler(caplog.handler)
    try:
        with caplog.at_level(logging.WARNING):
            on_mods, on_hidden, on_states = run("1")
    finally:
        logger.removeHandler(caplog.handler)
    off_mods, off_hidden, off_states = run("0")

    assert len(on_mods) == 14 and on_mods.keys() == off_mods.keys()
    for n in on_mods:
        for buf in ("qweight", "scales", "qzeros"):
            assert torch.equal(getattr(on_mods[n], buf), getattr(off_mods[n], buf)), (n, buf)
    assert torch.equal(on_hidden, off_hidden)
    # the probe engaged for all three ops and passed; nothing ran fused with the switch off
    assert on_states and not any(s.disabled for s in on_states)
    assert {key[0] for s in on_states for key in s.verified} == {"RMSNorm", "SiLU-mul", "rotary embedding"}
    assert sum(s.fused_calls for s in on_states) > 0 and sum(s.fused_calls for s in off_states) == 0
    assert not [r for r in caplog.records if "fused forward" in r.getMessage()]
