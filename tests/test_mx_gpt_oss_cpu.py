"""No GPU: the oracle of tests/mx_gpt_oss_cases.py checks itself, and the host-side surface of the MX GPT-OSS experts
(inc_mx_moe_gemm_glu's argument checks, gpt_oss_rows, mxfp4_buffers, is_gpt_oss_experts, extend_model_info, the qconfig.json schema).

  * every exact case keeps its exactness with the bias added, at least 99 % of its mode-0 outputs are comparable, and the clamp
    regions are all populated at limit = 7;
  * the oracle's own output passes its gate and each mutation -- the bias of expert e + 1, the gate and up bias halves swapped, the
    lower clamp on u left out, g clamped on both sides, u for u + 1, alpha = 1, the bias added after the routing weight -- fails it;
  * the header's fp32 expression, evaluated in torch float32, stays inside the mode-0 bound.
"""

import json
import math

import pytest
import torch

from tests import moe_models
from tests import mx_cases as C
from tests import mx_gpt_oss_cases as G
from tests import mx_moe_cases as M

DTYPES16 = [torch.bfloat16, torch.float16]
TEETH_CASES = ("kW", "ragged_e8", "kW_plus1")


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def test_bias_differs_between_experts_and_halves():
    b = G.bias_of(6, 2 * 72)
    assert float(b.abs().max()) <= 2.0 and bool((b * 4 == torch.round(b * 4)).all())
    assert not torch.equal(b[0], b[1]) and not torch.equal(b[:, :72], b[:, 72:])


@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_exactness_and_share_conditions(cm):
    c, mode = cm
    for rule in M.RULES:
        d = M.exact_case(c, mode, rule)
        G.assert_exact_condition(d)
        if mode == 0:
            for _, alpha, limit in G.PARAMS:
                for dtype in DTYPES16:
                    _, _, _, share = G.exact_gate(d, alpha, limit, dtype)
                    print(f"{c.name} {rule} alpha {alpha} limit {limit} {dtype}: comparable share {share:.4f}")
                    assert share >= G.MIN_SHARE, (c.name, rule, alpha, limit, dtype, share)


@pytest.mark.parametrize("rule", M.RULES)
def test_every_clamp_region_is_populated(rule):
    shares = G.region_shares(rule, 7.0)
    print(f"{rule} limit 7.0: {shares}")
    assert all(v >= G.MIN_REGION for v in shares.values()), shares
    tight = G.region_shares(rule, 0.75)
    print(f"{rule} limit 0.75: {tight}")
    assert tight["inside"] < 0.5 and all(v >= G.MIN_REGION for v in tight.values()), tight      # the clamps dominate
    none = G.region_shares(rule, math.inf)
    assert none["inside"] == 1.0


@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_the_oracle_passes_its_own_gate(cm):
    c, mode = cm
    d = M.exact_case(c, mode, "block")
    for _, alpha, limit in G.PARAMS:
        for dtype in (DTYPES16 if mode == 0 else [None]):
            assert G.check_output(d, G.oracle_output(d, alpha, limit, dtype), alpha, limit, dtype) is None


def _caught(mutation, mode, alpha, limit):
    """The (case, rule, dtype) on which the right output fails the gate of the mutated reference -- the same as a kernel with that
    mistake failing the gate of the right reference."""
    hit = []
    for name in TEETH_CASES:
        c = M.case(name)
        if mode not in c.modes:
            continue
        for rule in M.RULES:
            d = M.exact_case(c, mode, rule)
            for dtype in (DTYPES16 if mode == 0 else [None]):
                if G.check_output(d, G.oracle_output(d, alpha, limit, dtype), alpha, limit, dtype, mutate=mutation) is not None:
                    hit.append((name, rule, dtype))
    return hit


def _cases_of(hit):
    return {h[0] for h in hit}


@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("mutation", G.MUTATIONS_ALL_MODES)
def test_bias_mutations_are_caught(mutation, mode):
    want = {"kW", "ragged_e8"} if mode != 2 else {"kW"}                       # ragged_e8 has no mode-2 case
    for _, alpha, limit in (G.PARAMS if mode == 0 else G.PARAMS[:1]):          # alpha and limit are mode 0's
        assert want <= _cases_of(_caught(mutation, mode, alpha, limit)), (mutation, mode, alpha, limit)


@pytest.mark.parametrize("mutation", G.MUTATIONS_MODE0)
def test_activation_mutations_are_caught(mutation):
    for name, alpha, limit in G.PARAMS:
        if (mutation == "alpha_1" and alpha == 1.0) or (mutation in ("no_lower_clamp_u", "g_clamped_both_sides") and limit == math.inf):
            continue                                                          # the mutation is the identity under these parameters
        assert {"kW", "ragged_e8"} <= _cases_of(_caught(mutation, 0, alpha, limit)), (mutation, name)


def test_bias_after_the_routing_weight_is_caught():
    assert {"kW", "ragged_e8"} <= _cases_of(_caught("bias_after_weight", 1, 1.702, 7.0))


@pytest.mark.parametrize("cm", [cm for cm in M.CASE_MODES if cm[1] == 0], ids=[i for i, cm in zip(M.CASE_MODE_IDS, M.CASE_MODES) if cm[1] == 0])
def test_the_fp32_expression_is_inside_the_bound(cm):
    """The specified expression in torch float32 (then rounded once) on every comparable element."""
    c, _ = cm
    for rule in M.RULES:
        d = M.exact_case(c, 0, rule)
        for _, alpha, limit in G.PARAMS:
            v = G.fp32_expression(d, alpha, limit)
            for dtype in DTYPES16:
                assert G.check_output(d, v.to(dtype), alpha, limit, dtype) is None, (c.name, rule, alpha, limit, dtype)


# ---- the entry point -----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound_and_validates_before_any_hip_call():
    from neural_compressor_amd import _lib, ops

    assert "inc_mx_moe_gemm_glu" in _lib.SIGNATURES and callable(ops.mx_moe_gemm_glu)
    L = _lib.lib
    one = 16  # any non-NULL, 16-byte aligned address: rejected calls never touch it
    ok = dict(mode=2, aq=one, as_=one, afmt=C.FP8, route=one, wq=one, ws=one, wfmt=C.FP8, bias=one, alpha=1.702, limit=7.0, rw=None,
              wdt=_lib.INC_F32, out=one, odt=_lib.INC_F32, T=4, k=2, E=4, N=16, Kp=128)

    def call(**kw):
        a = dict(ok, **kw)
        return L.inc_mx_moe_gemm_glu(a["mode"], a["aq"], a["as_"], a["afmt"], a["route"], a["wq"], a["ws"], a["wfmt"], a["bias"],
                                     a["alpha"], a["limit"], a["rw"], a["wdt"], a["out"], a["odt"], a["T"], a["k"], a["E"], a["N"],
                                     a["Kp"], None)

    BAD, UNSUPPORTED = -1, -2
    for kw in (dict(aq=None), dict(as_=None), dict(route=None), dict(wq=None), dict(ws=None), dict(out=None), dict(T=0), dict(k=0),
               dict(E=0), dict(N=0), dict(Kp=0), dict(mode=3), dict(mode=-1), dict(mode=1, rw=None), dict(limit=0.0), dict(limit=-7.0),
               dict(limit=math.nan), dict(alpha=math.nan), dict(bias=18), dict(mode=0, odt=_lib.INC_BF16, limit=0.0)):
        assert call(**kw) == BAD, kw
    for kw in (dict(afmt=C.FP4, wfmt=C.FP8), dict(afmt=2), dict(wfmt=1), dict(Kp=192), dict(E=513), dict(mode=0, N=15, odt=_lib.INC_BF16),
               dict(mode=0, odt=_lib.INC_F32), dict(odt=_lib.INC_BF16), dict(mode=1, rw=one, odt=_lib.INC_F16), dict(mode=1, rw=one, wdt=7),
               dict(bias=None, Kp=192), dict(limit=math.inf, Kp=192)):        # NULL bias and limit = +inf pass the argument checks
        assert call(**kw) == UNSUPPORTED, kw


# ---- layout helpers ------------------------------------------------------------------------------------------------------------------
def test_gpt_oss_rows_places_gate_and_up_and_round_trips():
    from neural_compressor_amd.torch.algorithms.mx_quant.experts import (
        gpt_oss_bias_rows, gpt_oss_bias_rows_inverse, gpt_oss_rows, gpt_oss_rows_inverse)

    E, H, I = 3, 5, 4
    w = torch.arange(E * H * 2 * I, dtype=torch.float32).view(E, H, 2 * I)
    r = gpt_oss_rows(w)
    assert tuple(r.shape) == (E, 2 * I, H)
    for j in range(I):
        assert torch.equal(r[:, j], w[:, :, 2 * j]) and torch.equal(r[:, I + j], w[:, :, 2 * j + 1])
    assert torch.equal(gpt_oss_rows_inverse(r), w)
    b = torch.arange(E * 2 * I, dtype=torch.float32).view(E, 2 * I)
    rb = gpt_oss_bias_rows(b)
    assert torch.equal(rb[:, :I], b[:, 0::2]) and torch.equal(rb[:, I:], b[:, 1::2]) and torch.equal(gpt_oss_bias_rows_inverse(rb), b)


def _dequant_fp4(q, s, K):
    """MXExperts.recover's arithmetic on CPU buffers [E, R, Kp/2], [E, R, Kp/32] -> fp32 [E, R, K]."""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant.mx_quant import _code_values

    kp = s.shape[2] * 32
    q = torch.stack([q & 0xF, q >> 4], dim=3).reshape(q.shape[0], q.shape[1], -1)
    vals = _code_values(ops.MX_FP4_E2M1)[q.long()]
    scale = torch.ldexp(torch.ones((), dtype=torch.float32), s.to(torch.int32) - 127)
    return (vals.view(q.shape[0], q.shape[1], kp // 32, 32) * scale[..., None]).view(q.shape[0], q.shape[1], kp)[..., :K]


def test_mxfp4_buffers_are_the_checkpoint_bytes():
    """K = 160: Kp = 256, so three padding blocks exist.  Dequantising the buffers and undoing the row order is bit-equal to
    transformers' own dequantiser of the checkpoint tensors."""
    from transformers.integrations.mxfp4 import convert_moe_packed_tensors

    from neural_compressor_amd.torch.algorithms.mx_quant.experts import gpt_oss_rows_inverse, mxfp4_buffers

    E, R, K = 3, 8, 160
    g = torch.Generator().manual_seed(5)
    blocks = torch.randint(0, 256, (E, R, K // 32, 16), generator=g, dtype=torch.uint8)
    scales = torch.randint(100, 140, (E, R, K // 32), generator=g, dtype=torch.uint8)
    want = convert_moe_packed_tensors(blocks, scales, dtype=torch.float32)      # [E, K, R]
    assert tuple(want.shape) == (E, K, R)
    q, s = mxfp4_buffers(blocks, scales, 256)
    assert tuple(q.shape) == (E, R, 128) and tuple(s.shape) == (E, R, 8)
    assert bool((q[:, :, K // 2:] == 0).all()) and bool((s[:, :, K // 32:] == 0).all())
    got = _dequant_fp4(q, s, K).transpose(1, 2)
    assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    qi, si = mxfp4_buffers(blocks, scales, 256, interleaved=True)
    assert torch.equal(qi[:, :R // 2], q[:, 0::2]) and torch.equal(si[:, R // 2:], s[:, 1::2])
    got = gpt_oss_rows_inverse(_dequant_fp4(qi, si, K))
    assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


# ---- recogniser, config, schema ------------------------------------------------------------------------------------------------------
def test_recogniser():
    from neural_compressor_amd.torch.utils import is_fused_experts, is_gpt_oss_experts

    oss = moe_models.tiny_gpt_oss_experts()
    assert is_gpt_oss_experts(oss) and not is_fused_experts(oss)
    with torch.device("meta"):
        others = [m for build in (moe_models.tiny_mixtral, moe_models.tiny_qwen3_moe, moe_models.tiny_olmoe)
                  for _, m in moe_models.experts_of(build())]
    assert len(others) == 6
    for m in others:
        assert is_fused_experts(m) and not is_gpt_oss_experts(m)
    lin = torch.nn.Linear(4, 4)
    assert not is_gpt_oss_experts(lin) and not is_fused_experts(lin)
    del oss.alpha
    assert not is_gpt_oss_experts(oss)


def test_extend_model_info_adds_the_gpt_oss_experts():
    from neural_compressor_amd.torch.quantization import MXQuantConfig
    from neural_compressor_amd.torch.quantization.quantize import _model_info

    with torch.device("meta"):
        model = G.tiny_gpt_oss()
    base = MXQuantConfig.get_model_info(model)
    experts = [(n, type(m).__name__) for n, m in G.gpt_oss_experts_of(model)]
    assert len(experts) == 2 and all(t == "GptOssExperts" for _, t in experts)
    assert _model_info(MXQuantConfig(), model) == base == _model_info(MXQuantConfig(quant_experts=False), model)
    info = _model_info(MXQuantConfig(quant_experts=True), model)
    assert info[:len(base)] == base and sorted(info[len(base):]) == sorted(experts)
    cfg = MXQuantConfig(quant_experts=True)
    cfg.set_local(experts[0][0], MXQuantConfig(w_dtype="fp32"))
    mapping = cfg.to_config_mapping(model_info=info)
    assert mapping[experts[0]].w_dtype == "fp32" and mapping[experts[1]].w_dtype == "fp8_e4m3"
    assert not any(e in MXQuantConfig().to_config_mapping(model_info=base) for e in experts)


def test_unsupported_reasons():
    from neural_compressor_amd.torch.algorithms.mx_quant.experts import unsupported_reason

    class Fake(torch.nn.Module):
        def __init__(self, E, H=8):
            super().__init__()
            mk = lambda *s: torch.nn.Parameter(torch.empty(*s, device="meta"))  # noqa: E731
            self.gate_up_proj, self.gate_up_proj_bias = mk(E, H, 8), mk(E, 8)
            self.down_proj, self.down_proj_bias = mk(E, 4, H), mk(E, H)
            self.alpha, self.limit = 1.702, 7.0

    ok = dict(w_dtype="fp4", act_dtype="fp8_e4m3")
    assert unsupported_reason(Fake(4), ok) is None and unsupported_reason(Fake(512), ok) is None
    assert "E=513" in unsupported_reason(Fake(513), ok)
    assert "H=6" in unsupported_reason(Fake(4, 6), ok)
    assert "not one of" in unsupported_reason(Fake(4), dict(w_dtype="fp8_e4m3", act_dtype="fp4"))


def test_module_needs_a_hip_device():
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts

    with pytest.raises(RuntimeError, match="HIP device"):
        MXGptOssExperts(2, 8, 8, device="cpu")


def test_qconfig_schema_lists_the_gpt_oss_experts(tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import MXGptOssExperts, save_load

    m = MXGptOssExperts.__new__(MXGptOssExperts)
    torch.nn.Module.__init__(m)
    for k, v in dict(w_dtype="fp4", act_dtype="fp8_e4m3", num_experts=3, hidden_dim=40, intermediate_dim=24, alpha=1.702,
                     limit=7.0).items():
        setattr(m, k, v)
    for prefix, N, K in (("gate_up", 48, 40), ("down", 40, 24)):
        m.register_buffer(f"{prefix}_qweight", torch.zeros(3, N, C.padded_k(K) // 2, dtype=torch.uint8))
        m.register_buffer(f"{prefix}_w_scale", torch.zeros(3, N, C.padded_k(K) // 32, dtype=torch.uint8))
        m.register_buffer(f"{prefix}_bias", torch.zeros(3, N))
    model = torch.nn.Module()
    model.layer = torch.nn.Module()
    model.layer.experts = m
    model.layer.norm = torch.nn.LayerNorm(40)
    model.mx_info = {"blocksize": 32, "round_method": "nearest"}
    cfg = save_load.qconfig_of(model)
    assert cfg["mx_gpt_oss_experts"] == {"layer.experts": ["fp4", "fp8_e4m3", 3, 40, 24, 1.702, 7.0]}
    assert "mx_experts" not in cfg and cfg["mx_modules"] == {}
    save_load.save(model, str(tmp_path))
    with open(tmp_path / save_load.QCONFIG_NAME) as f:
        assert json.load(f) == cfg
    state = torch.load(tmp_path / save_load.WEIGHT_NAME, weights_only=True)
    assert {"layer.experts.gate_up_bias", "layer.experts.down_bias", "layer.experts.gate_up_qweight"} <= set(state)
    plain = torch.nn.Module()
    plain.norm = torch.nn.LayerNorm(8)
    assert "mx_gpt_oss_experts" not in save_load.qconfig_of(plain)
