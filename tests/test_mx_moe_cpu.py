"""No GPU: the cases and the oracle of tests/mx_moe_cases.py check themselves, and the host-side surface of MX experts
(MXQuantConfig.quant_experts, extend_model_info, unsupported_reason, the qconfig.json schema).

  * every exact case meets its exactness condition, and in mode 0 at least 99 % of its outputs are comparable in bf16 and fp16;
  * the oracle's own output passes its gate, and each mutation of the weights -- expert e + 1, gate and up halves swapped, the scale of
    the neighbouring block, the routing weight by position where it should be by slot -- fails it on at least one case: the gates can
    tell a kernel with that mistake from a right one;
  * the entry point is bound and validates its arguments before any HIP call.
"""

import json
import os

import pytest
import torch

from tests import moe_models
from tests import moe_stage_cases as S
from tests import mx_cases as C
from tests import mx_moe_cases as M

DTYPES16 = [torch.bfloat16, torch.float16]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def test_case_table_keeps_every_pin():
    names = [c.name for c in M.CASES]
    assert len(set(names)) == len(names)
    for want in ("one_tile_n4", "kW", "kW_minus1", "kW_plus1", "ragged_e8", "i7", "max_e", "spread", "many_rows", "one_slot",
                 "short_waves", "all_invalid"):
        assert want in names, want
    assert M.case("kW").Kp == 128 * M.WAVES and M.case("kW_minus1").Kp == 128 * (M.WAVES - 1) and M.case("kW_plus1").Kp == 128 * (M.WAVES + 1)
    assert M.case("kW").Nout % M.STRIP == 4 and M.case("one_tile_n4").Nout < M.STRIP and M.case("i7").Nout % 4 != 0
    assert all(c.Kp % C.KTILE == 0 and c.routing in S.ROUTINGS for c in M.CASES)
    assert M.route_of("max_experts")["E"] == 512 > M.route_of("max_experts")["S"]
    assert M.route_of("all_invalid")["nvalid"] == 0 and M.route_of("all_invalid")["ntiles"] == 0


def test_routing_weights_tell_slot_from_position():
    for name in ("edges3", "edges", "many_rows"):
        ro = M.route_of(name)
        w = M.routing_weights(ro["T"], ro["k"]).reshape(-1)
        order = ro["order"].long()[:ro["nvalid"]]
        assert set(w.tolist()) == set(M.ROUTING_WEIGHTS)
        assert float((w[order] != w[:ro["nvalid"]]).double().mean()) > 0.25
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.equal(M.routing_weights(7, 2, dt).double(), M.routing_weights(7, 2, torch.float64))


@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_exactness_and_share_conditions(cm):
    c, mode = cm
    for rule in M.RULES:
        d = M.exact_case(c, mode, rule)
        M.assert_exact_condition(d)
        assert int(d["named"].sum()) <= d["ro"]["nvalid"] and (d["ro"]["nvalid"] == 0) == (not bool(d["named"].any()))
        if mode == 0:
            for dtype in DTYPES16:
                _, _, ok, share = M.mode0_gate(d, dtype)
                print(f"{c.name} {rule} {dtype}: comparable share {share:.4f}")
                assert share >= M.MIN_SHARE, (c.name, rule, dtype, share)


@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_the_oracle_passes_its_own_gate(cm):
    c, mode = cm
    d = M.exact_case(c, mode, "block")
    for dtype in (DTYPES16 if mode == 0 else [None]):
        assert M.check_output(d, M.oracle_output(d, dtype), dtype) is None


def _caught(mutation, mode, names):
    """The cases (of `names`) on which the output of the right weights fails the gate of the mutated reference -- the same as a kernel
    with that mistake failing the gate of the right reference."""
    hit = []
    for name in names:
        c = M.case(name)
        if mode not in c.modes:
            continue
        for rule in M.RULES:
            d = M.exact_case(c, mode, rule)
            for dtype in (DTYPES16 if mode == 0 else [None]):
                if M.check_output(d, M.oracle_output(d, dtype), dtype, mutate=mutation) is not None:
                    hit.append((name, rule, dtype))
    return hit


SMALL = ("one_tile_n4", "kW", "kW_plus1", "i7", "max_e", "spread", "short_waves")


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_reading_the_next_expert_is_caught(mode):
    assert _caught("expert_plus_1", mode, SMALL), mode


def test_swapped_gate_and_up_halves_are_caught():
    assert _caught("halves_swapped", 0, SMALL)


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_the_scale_of_the_neighbouring_block_is_caught(mode):
    hit = _caught("scale_of_next_block", mode, SMALL)
    assert any(rule == "block" for _, rule, _ in hit), hit      # the rule that moves with the block is the one that must catch it


def test_the_routing_weight_by_position_is_caught():
    assert _caught("weight_by_position", 1, ("kW", "kW_plus1", "short_waves"))


def test_random_cases_have_comparable_outputs():
    for pair in C.PAIRS:
        for dtype in DTYPES16:
            d = M.random_case(0, *pair)
            ref, tol, ok = M.random_gate(d, dtype)
            share = float(ok.double().mean())
            print(f"random mode 0 {pair} {dtype}: comparable share {share:.3f}")
            assert share >= 0.5 and bool(torch.isfinite(ref[ok]).all())


# ---- the entry point -----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound_and_validates_before_any_hip_call():
    from neural_compressor_amd import _lib, ops

    assert "inc_mx_moe_gemm" in _lib.SIGNATURES and callable(ops.mx_moe_gemm)
    L = _lib.lib
    one = 16  # any non-NULL, 16-byte aligned address: rejected calls never touch it
    ok = dict(mode=2, aq=one, as_=one, afmt=C.FP8, route=one, wq=one, ws=one, wfmt=C.FP8, rw=None, wdt=_lib.INC_F32, out=one,
              odt=_lib.INC_F32, T=4, k=2, E=4, N=16, Kp=128)

    def call(**kw):
        a = dict(ok, **kw)
        return L.inc_mx_moe_gemm(a["mode"], a["aq"], a["as_"], a["afmt"], a["route"], a["wq"], a["ws"], a["wfmt"], a["rw"], a["wdt"],
                                 a["out"], a["odt"], a["T"], a["k"], a["E"], a["N"], a["Kp"], None)

    BAD, UNSUPPORTED = -1, -2
    for kw in (dict(aq=None), dict(as_=None), dict(route=None), dict(wq=None), dict(ws=None), dict(out=None), dict(T=0), dict(k=0),
               dict(E=0), dict(N=0), dict(Kp=0), dict(mode=3), dict(mode=-1), dict(mode=1, rw=None)):
        assert call(**kw) == BAD, kw
    for kw in (dict(afmt=C.FP4, wfmt=C.FP8), dict(afmt=2), dict(wfmt=1), dict(Kp=192), dict(E=513), dict(mode=0, N=15, odt=_lib.INC_BF16),
               dict(mode=0, odt=_lib.INC_F32), dict(odt=_lib.INC_BF16), dict(mode=1, rw=one, odt=_lib.INC_F16), dict(mode=1, rw=one, wdt=7)):
        assert call(**kw) == UNSUPPORTED, kw


# ---- config surface ------------------------------------------------------------------------------------------------------------------
def test_quant_experts_is_a_stored_field_that_round_trips():
    from neural_compressor_amd.torch.quantization import MXQuantConfig

    cfg = MXQuantConfig(quant_experts=True)
    assert cfg.quant_experts is True and MXQuantConfig().quant_experts is False
    d = cfg.to_dict()
    assert d["quant_experts"] is True and MXQuantConfig().to_dict()["quant_experts"] is False
    back = MXQuantConfig.from_dict(d)
    assert back.quant_experts is True and back.to_dict() == d
    assert MXQuantConfig.from_dict(json.loads(json.dumps(d))).quant_experts is True


@pytest.mark.parametrize("build", [moe_models.tiny_mixtral, moe_models.tiny_qwen3_moe], ids=["mixtral", "qwen3_moe"])
def test_extend_model_info_adds_exactly_the_fused_experts(build):
    from neural_compressor_amd.torch.quantization import MXQuantConfig
    from neural_compressor_amd.torch.quantization.quantize import _model_info

    with torch.device("meta"):
        model = build()
    base = MXQuantConfig.get_model_info(model)
    experts = [(n, type(m).__name__) for n, m in moe_models.experts_of(model)]
    assert len(experts) == 2
    assert _model_info(MXQuantConfig(), model) == base == _model_info(MXQuantConfig(quant_experts=False), model)
    info = _model_info(MXQuantConfig(quant_experts=True), model)
    assert info[:len(base)] == base and sorted(info[len(base):]) == sorted(experts)
    mapping = MXQuantConfig(quant_experts=True).to_config_mapping(model_info=info)
    assert all(e in mapping and mapping[e].w_dtype == "fp8_e4m3" for e in experts)
    cfg = MXQuantConfig(quant_experts=True)
    cfg.set_local(experts[0][0], MXQuantConfig(w_dtype="fp32"))
    mapping = cfg.to_config_mapping(model_info=info)
    assert mapping[experts[0]].w_dtype == "fp32" and mapping[experts[1]].w_dtype == "fp8_e4m3"
    assert not any(e in MXQuantConfig().to_config_mapping(model_info=base) for e in experts)


def test_unsupported_reasons():
    from neural_compressor_amd.torch.algorithms.mx_quant.experts import unsupported_reason

    class Fake(torch.nn.Module):
        def __init__(self, E, act):
            super().__init__()
            self.gate_up_proj = torch.nn.Parameter(torch.empty(E, 8, 4, device="meta"))
            self.down_proj = torch.nn.Parameter(torch.empty(E, 4, 4, device="meta"))
            self.act_fn = act

    ok = dict(w_dtype="fp4", act_dtype="fp8_e4m3")
    assert unsupported_reason(Fake(4, torch.nn.SiLU()), ok) is None
    assert unsupported_reason(Fake(512, torch.nn.SiLU()), dict(w_dtype="fp4", act_dtype="fp4")) is None
    assert "GELU is not SiLU" in unsupported_reason(Fake(4, torch.nn.GELU()), ok)
    assert "E=513" in unsupported_reason(Fake(513, torch.nn.SiLU()), ok)
    assert "not one of" in unsupported_reason(Fake(4, torch.nn.SiLU()), dict(w_dtype="fp8_e4m3", act_dtype="fp4"))
    from neural_compressor_amd.torch.utils.utility import is_fused_experts

    assert is_fused_experts(Fake(4, torch.nn.SiLU())) and not is_fused_experts(moe_models.tiny_gpt_oss_experts())


def test_modules_need_a_hip_device():
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts

    with pytest.raises(RuntimeError, match="HIP device"):
        MXExperts(2, 8, 8, device="cpu")


# ---- save / load schema --------------------------------------------------------------------------------------------------------------
def _fabricated_experts(name_values):
    """An MXExperts without a device: the attributes save() reads and four CPU buffers."""
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts

    m = MXExperts.__new__(MXExperts)
    torch.nn.Module.__init__(m)
    for k, v in name_values.items():
        setattr(m, k, v)
    E, H, I = m.num_experts, m.hidden_dim, m.intermediate_dim
    for prefix, N, K in (("gate_up", 2 * I, H), ("down", H, I)):
        m.register_buffer(f"{prefix}_qweight", torch.zeros(E, N, C.padded_k(K), dtype=torch.uint8))
        m.register_buffer(f"{prefix}_w_scale", torch.zeros(E, N, C.padded_k(K) // 32, dtype=torch.uint8))
    return m


def test_qconfig_schema_lists_the_experts(tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import save_load

    model = torch.nn.Module()
    model.layer = torch.nn.Module()
    model.layer.experts = _fabricated_experts(dict(w_dtype="fp4", act_dtype="fp8_e4m3", num_experts=3, hidden_dim=40, intermediate_dim=24))
    model.layer.norm = torch.nn.LayerNorm(40)
    model.mx_info = {"blocksize": 32, "round_method": "nearest"}
    save_load.save(model, str(tmp_path))
    cfg = json.load(open(os.path.join(tmp_path, save_load.QCONFIG_NAME)))
    assert cfg == {"mx_quant": {"blocksize": 32, "round_method": "nearest"}, "mx_modules": {},
                   "mx_experts": {"layer.experts": ["fp4", "fp8_e4m3", 3, 40, 24]}}
    state = torch.load(os.path.join(tmp_path, save_load.WEIGHT_NAME), weights_only=True)
    assert {k for k in state if k.startswith("layer.experts.")} == {
        "layer.experts." + n for n in ("gate_up_qweight", "gate_up_w_scale", "down_qweight", "down_w_scale")}
    assert state["layer.experts.gate_up_qweight"].shape == (3, 48, 128) and state["layer.experts.down_w_scale"].shape == (3, 40, 4)


def test_a_directory_without_the_experts_key_still_loads(tmp_path):
    from neural_compressor_amd.torch.algorithms.mx_quant import save_load

    model = torch.nn.Sequential(torch.nn.LayerNorm(8))
    with open(os.path.join(tmp_path, save_load.QCONFIG_NAME), "w") as f:
        json.dump({"mx_quant": {"blocksize": 32, "round_method": "nearest"}, "mx_modules": {}}, f)      # the schema before MXExperts
    want = {k: v + 1.0 for k, v in model.state_dict().items()}
    torch.save(want, os.path.join(tmp_path, save_load.WEIGHT_NAME))
    back = save_load.load(str(tmp_path), torch.nn.Sequential(torch.nn.LayerNorm(8)), device="cpu")
    assert all(torch.equal(v, want[k]) for k, v in back.state_dict().items()) and back.mx_info["blocksize"] == 32
