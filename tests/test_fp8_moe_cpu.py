"""No GPU: the cases and the oracle of tests/fp8_moe_cases.py check themselves, and the host-side surface of FP8 experts
(FP8Config.moe_experts, extend_model_info, unsupported_reason, the qconfig.json schema).

  * every exact case meets its exactness condition, and in mode 0 at least 99 % of its outputs are comparable in bf16 and fp16;
  * the oracle's own output passes its gate, and each wrong read -- expert e + 1, gate and up halves swapped, the routing weight by
    position, the row scale of row p where it should be order[p] / top_k, alpha of expert e +- 1 -- fails it on at least one case;
  * the entry point is bound and validates its arguments before any HIP call.
"""

import json
import os

import pytest
import torch

from tests import fp8_moe_cases as M
from tests import moe_models

DTYPES16 = [torch.bfloat16, torch.float16]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_exactness_and_share_conditions(cm):
    c, mode = cm
    d = M.exact_case(c, mode)
    fig = M.assert_exact_condition(d)
    assert int(d["named"].sum()) <= d["ro"]["nvalid"] and (d["ro"]["nvalid"] == 0) == (not bool(d["named"].any()))
    if fig is not None:
        print(f"{c.name} mode 0: min g {fig['min_g']:.3f}, max |silu(g) u| {fig['max_ref']:.3f}, shares {list(fig['shares'].values())}")


def test_factors_differ_by_row_column_and_expert():
    d = M.exact_case(M.case("kW"), 2)
    assert len(set(d["rs"][:5].tolist())) == 5 and len(set(d["al"][0, :5].tolist())) == 5
    assert not torch.equal(d["al"][0], d["al"][1]) and not torch.equal(d["w"][0], d["w"][1])
    assert set(d["rs"].tolist()) <= {2.0 ** j for j in range(-3, 2)}
    d0 = M.exact_case(M.case("kW"), 0)
    assert set(d0["al"].reshape(-1).tolist()) <= {2.0 ** j for j in range(-6, -1)}
    assert set(d0["w"][:, :d0["N"] // 2].reshape(-1).tolist()) <= {-1, 0, 1}
    assert 0.6 < float((d0["w"][:, :d0["N"] // 2] == 0).double().mean()) < 0.72       # two zeros in three


@pytest.mark.parametrize("cm", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_the_oracle_passes_its_own_gate(cm):
    c, mode = cm
    d = M.exact_case(c, mode)
    for dtype in (DTYPES16 if mode == 0 else [None]):
        assert M.check_output(d, M.oracle_output(d, dtype), dtype) is None


def _caught(mutation, mode, names):
    """The cases (of `names`) on which the output of the right reads fails the gate of the mutated reference -- the same as a kernel
    with that mistake failing the gate of the right reference."""
    hit = []
    for name in names:
        c = M.case(name)
        if mode not in c.modes:
            continue
        d = M.exact_case(c, mode)
        for dtype in (DTYPES16 if mode == 0 else [None]):
            if M.check_output(d, M.oracle_output(d, dtype), dtype, mutate=mutation) is not None:
                hit.append((name, dtype))
    return hit


SMALL = ("one_tile_n4", "kW", "kW_plus1", "i7", "max_e", "spread", "short_waves")


def test_the_mutation_list_is_complete():
    assert set(M.MUTATIONS) == {"expert_plus_1", "halves_swapped", "weight_by_position", "row_scale_by_position",
                                "alpha_of_next_expert", "alpha_of_previous_expert"}


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_reading_the_next_expert_is_caught(mode):
    assert _caught("expert_plus_1", mode, SMALL), mode


def test_swapped_gate_and_up_halves_are_caught():
    assert _caught("halves_swapped", 0, SMALL)


def test_the_routing_weight_by_position_is_caught():
    assert _caught("weight_by_position", 1, ("kW", "kW_plus1", "short_waves"))


@pytest.mark.parametrize("mode", [2, 0])
def test_the_row_scale_by_position_is_caught(mode):
    assert _caught("row_scale_by_position", mode, SMALL), mode


@pytest.mark.parametrize("mutation", ["alpha_of_next_expert", "alpha_of_previous_expert"])
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_alpha_of_a_neighbouring_expert_is_caught(mode, mutation):
    assert _caught(mutation, mode, SMALL), (mode, mutation)


def test_random_cases_have_comparable_outputs():
    for dtype in DTYPES16:
        ref, tol, ok = M.random_gate(M.random_case(0), dtype)
        share = float(ok.double().mean())
        print(f"random mode 0 {dtype}: comparable share {share:.3f}")
        assert share >= 0.5 and bool(torch.isfinite(ref[ok]).all())
    d = M.random_case(0, small=True, unit=True)                     # the unit-factor case of the comparison with inc_mx_moe_gemm
    I = d["N"] // 2
    ref = M.S.silu64(d["val"][:, :I]) * d["val"][:, I:]
    assert float(d["val"][:, :I].min()) >= M.MODE0_MIN_G
    for dtype in DTYPES16:
        assert float((ref.abs() < float(torch.finfo(dtype).max) / 2).double().mean()) >= M.MIN_SHARE


# ---- the entry point -----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound_and_validates_before_any_hip_call():
    from neural_compressor_amd import _lib, ops

    assert "inc_fp8_moe_gemm" in _lib.SIGNATURES and callable(ops.fp8_moe_gemm)
    assert _lib.ABI_VERSION == _lib.lib.inc_abi_version()
    L = _lib.lib
    one = 4096  # any non-NULL, 16-byte aligned address: rejected calls never touch it
    ok = dict(mode=2, aq=one, rs=one, route=one, wq=one, al=one, rw=None, wdt=_lib.INC_F32, out=one, odt=_lib.INC_F32, T=4, k=2, E=4,
              N=16, Kp=128)

    def call(**kw):
        a = dict(ok, **kw)
        return L.inc_fp8_moe_gemm(a["mode"], a["aq"], a["rs"], a["route"], a["wq"], a["al"], a["rw"], a["wdt"], a["out"], a["odt"],
                                  a["T"], a["k"], a["E"], a["N"], a["Kp"], None)

    BAD, UNSUPPORTED = -1, -2
    for kw in (dict(aq=None), dict(rs=None), dict(route=None), dict(wq=None), dict(al=None), dict(out=None), dict(T=0), dict(k=0),
               dict(E=0), dict(N=0), dict(Kp=0), dict(Kp=-128), dict(mode=3), dict(mode=-1), dict(mode=1, rw=None),
               dict(aq=one + 8), dict(wq=one + 4), dict(rs=one + 2), dict(al=one + 1)):
        assert call(**kw) == BAD, kw
    for kw in (dict(Kp=192), dict(E=513), dict(T=2 ** 21 + 1), dict(mode=0, N=15, odt=_lib.INC_BF16), dict(mode=0, odt=_lib.INC_F32),
               dict(odt=_lib.INC_BF16), dict(odt=77), dict(mode=1, rw=one, odt=_lib.INC_F16), dict(mode=1, rw=one, wdt=7)):
        assert call(**kw) == UNSUPPORTED, kw


def test_ops_refuses_cpu_tensors():
    from neural_compressor_amd import ops

    z8, zf = torch.zeros(2, 128, dtype=torch.uint8), torch.ones(2)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.fp8_moe_gemm(2, z8, zf, torch.zeros(64, dtype=torch.int32), z8[None], zf[None], 2, 1)


# ---- config surface ------------------------------------------------------------------------------------------------------------------
def test_moe_experts_is_a_stored_field_that_round_trips():
    from neural_compressor_amd.torch.quantization import FP8Config

    cfg = FP8Config(moe_experts=True)
    assert cfg.moe_experts is True and FP8Config().moe_experts is False and not hasattr(cfg, "quant_experts")
    d = cfg.to_dict()
    assert d["moe_experts"] is True and FP8Config().to_dict()["moe_experts"] is False
    back = FP8Config.from_dict(json.loads(json.dumps(d)))
    assert back.moe_experts is True and back.to_dict() == d


@pytest.mark.parametrize("build", [moe_models.tiny_mixtral, moe_models.tiny_qwen3_moe, moe_models.tiny_olmoe],
                         ids=["mixtral", "qwen3_moe", "olmoe"])
def test_extend_model_info_adds_exactly_the_fused_experts(build):
    from neural_compressor_amd.torch.quantization import FP8Config
    from neural_compressor_amd.torch.quantization.quantize import _model_info

    with torch.device("meta"):
        model = build()
    base = FP8Config.get_model_info(model)
    experts = [(n, type(m).__name__) for n, m in moe_models.experts_of(model)]
    assert len(experts) == 2
    assert _model_info(FP8Config(), model) == base == _model_info(FP8Config(moe_experts=False), model)
    info = _model_info(FP8Config(moe_experts=True), model)
    assert info[:len(base)] == base and sorted(info[len(base):]) == sorted(experts)
    mapping = FP8Config(moe_experts=True).to_config_mapping(model_info=info)
    assert all(e in mapping and mapping[e].fp8_config == "E4M3" for e in experts)
    cfg = FP8Config(moe_experts=True)
    cfg.set_local(experts[0][0], FP8Config(fp8_config="fp32"))
    mapping = cfg.to_config_mapping(model_info=info)
    assert mapping[experts[0]].fp8_config == "fp32" and mapping[experts[1]].fp8_config == "E4M3"
    assert not any(e in FP8Config().to_config_mapping(model_info=base) for e in experts)


def test_unsupported_reasons():
    from neural_compressor_amd.torch.algorithms.fp8_quant.experts import unsupported_reason
    from neural_compressor_amd.torch.utils.utility import is_fused_experts

    class Fake(torch.nn.Module):
        def __init__(self, E, act):
            super().__init__()
            self.gate_up_proj = torch.nn.Parameter(torch.empty(E, 8, 4, device="meta"))
            self.down_proj = torch.nn.Parameter(torch.empty(E, 4, 4, device="meta"))
            self.act_fn = act

    ok = dict(fp8_config="E4M3")
    assert unsupported_reason(Fake(4, torch.nn.SiLU()), ok) is None and unsupported_reason(Fake(512, torch.nn.SiLU()), ok) is None
    assert "GELU is not SiLU" in unsupported_reason(Fake(4, torch.nn.GELU()), ok)
    assert "E=513" in unsupported_reason(Fake(513, torch.nn.SiLU()), ok)
    assert is_fused_experts(Fake(4, torch.nn.SiLU())) and not is_fused_experts(moe_models.tiny_gpt_oss_experts())


def test_modules_need_a_hip_device():
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts

    with pytest.raises(RuntimeError, match="HIP device"):
        FP8Experts(2, 8, 8, device="cpu")


# ---- save / load schema --------------------------------------------------------------------------------------------------------------
def _fabricated_experts(E, H, I):
    """An FP8Experts without a device: the attributes save() reads and four CPU buffers."""
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Experts

    m = FP8Experts.__new__(FP8Experts)
    torch.nn.Module.__init__(m)
    m.num_experts, m.hidden_dim, m.intermediate_dim = E, H, I
    for prefix, N, K in (("gate_up", 2 * I, H), ("down", H, I)):
        m.register_buffer(f"{prefix}_qweight", torch.zeros(E, N, M.F.padded_k(K), dtype=torch.uint8))
        m.register_buffer(f"{prefix}_w_scale", torch.zeros(E, N, dtype=torch.float32))
    return m


def test_qconfig_schema_lists_the_experts(tmp_path):
    from neural_compressor_amd.torch.algorithms.fp8_quant import save_load

    info = {"fp8_config": "E4M3", "act_granularity": "per_token", "w_granularity": "per_channel"}
    model = torch.nn.Module()
    model.layer = torch.nn.Module()
    model.layer.experts = _fabricated_experts(3, 40, 24)
    model.layer.norm = torch.nn.LayerNorm(40)
    model.fp8_info = dict(info)
    save_load.save(model, str(tmp_path))
    cfg = json.load(open(os.path.join(tmp_path, save_load.QCONFIG_NAME)))
    assert cfg == {"fp8_quant": info, "fp8_modules": [], "fp8_experts": {"layer.experts": [3, 40, 24]}}
    state = torch.load(os.path.join(tmp_path, save_load.WEIGHT_NAME), weights_only=True)
    assert {k for k in state if k.startswith("layer.experts.")} == {
        "layer.experts." + n for n in ("gate_up_qweight", "gate_up_w_scale", "down_qweight", "down_w_scale")}
    assert state["layer.experts.gate_up_qweight"].shape == (3, 48, 128) and state["layer.experts.down_w_scale"].shape == (3, 40)
    assert state["layer.experts.down_w_scale"].dtype is torch.float32


def test_qconfig_of_a_model_without_experts_keeps_its_two_keys():
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear, save_load

    lin = FP8Linear.__new__(FP8Linear)
    torch.nn.Module.__init__(lin)
    model = torch.nn.Module()
    model.proj = lin
    model.norm = torch.nn.LayerNorm(8)
    model.fp8_info = {"fp8_config": "E4M3"}
    assert save_load.qconfig_of(model) == {"fp8_quant": {"fp8_config": "E4M3"}, "fp8_modules": ["proj"]}


def test_a_directory_without_the_experts_key_still_loads(tmp_path):
    from neural_compressor_amd.torch.algorithms.fp8_quant import save_load

    model = torch.nn.Sequential(torch.nn.LayerNorm(8))
    with open(os.path.join(tmp_path, save_load.QCONFIG_NAME), "w") as f:
        json.dump({"fp8_quant": {"fp8_config": "E4M3"}, "fp8_modules": []}, f)                         # the schema before FP8Experts
    want = {k: v + 1.0 for k, v in model.state_dict().items()}
    torch.save(want, os.path.join(tmp_path, save_load.WEIGHT_NAME))
    back = save_load.load(str(tmp_path), torch.nn.Sequential(torch.nn.LayerNorm(8)), device="cpu")
    assert all(torch.equal(v, want[k]) for k, v in back.state_dict().items()) and back.fp8_info["fp8_config"] == "E4M3"
