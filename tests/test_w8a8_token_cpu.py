"""CPU: the dynamic per-token int8 activation cell of SmoothQuant W8A8 without a GPU -- the config accepts the cell and nothing near it,
the oracle of tests/w8a8_token_cases.py checks itself on hand-made rows, its comparator rejects the three mistakes a row-wise quantiser
makes most easily, the tuner's torch op is the oracle's q * s, the two new entry points validate before any HIP call, and the accuracy
condition the cell exists for holds in the fake-quant arithmetic alone."""

import pytest
import torch

from tests import w8a8_token_cases as T


def test_the_cell_is_accepted_and_its_near_misses_are_not():
    from neural_compressor_amd.torch.quantization import SmoothQuantConfig

    cfg = SmoothQuantConfig(act_dtype="int8", act_sym=True, act_granularity="per_token", act_algo="minmax")
    assert (cfg.act_dtype, cfg.act_sym, cfg.act_granularity, cfg.act_algo) == ("int8", True, "per_token", "minmax")
    assert (cfg.w_dtype, cfg.w_sym, cfg.w_granularity, cfg.w_algo) == ("int8", True, "per_channel", "minmax")
    d = SmoothQuantConfig()   # the default stays the static cell
    assert (d.act_dtype, d.act_sym, d.act_granularity, d.act_algo) == ("uint8", False, "per_tensor", "minmax")
    for miss in (dict(act_dtype="uint8", act_sym=True, act_granularity="per_token"),
                 dict(act_dtype="int8", act_sym=False, act_granularity="per_token"),
                 dict(act_dtype="int8", act_sym=True, act_granularity="per_tensor"),
                 dict(act_dtype="int8", act_sym=True, act_granularity="per_token", act_algo="kl")):
        with pytest.raises(NotImplementedError, match="activations must be uint8 / asymmetric / per_tensor / minmax"):
            SmoothQuantConfig(**miss)


def test_the_act_fields_reach_the_per_layer_dict_and_set_local_mixes_cells():
    from neural_compressor_amd.torch.algorithms.smooth_quant import SmoothQuantQuantizer
    from neural_compressor_amd.torch.quantization import SmoothQuantConfig
    from neural_compressor_amd.torch.quantization import algorithm_entry as E

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = torch.nn.Linear(8, 8), torch.nn.Linear(8, 8), torch.nn.Linear(8, 8)

    cfg = SmoothQuantConfig(act_dtype="int8", act_sym=True, act_granularity="per_token")
    cfg.set_local("b", SmoothQuantConfig())
    cfg.set_local("c", SmoothQuantConfig(w_dtype="fp32"))
    net = Net()
    mapping = cfg.to_config_mapping(model_info=SmoothQuantConfig.get_model_info(net))
    seen = {}

    class Spy(SmoothQuantQuantizer):
        def execute(self, model, mode=None, **kwargs):
            seen.update(self.quant_config)
            return model

    real = E.get_quantizer
    E.get_quantizer = lambda model, quantizer_cls, quant_config: Spy(quant_config)
    try:
        E.smooth_quant_entry(net, mapping)
    finally:
        E.get_quantizer = real
    assert {k: seen["a"][k] for k in ("act_dtype", "act_sym", "act_granularity", "act_algo")} == dict(
        act_dtype="int8", act_sym=True, act_granularity="per_token", act_algo="minmax")
    assert seen["b"]["act_granularity"] == "per_tensor" and seen["b"]["act_dtype"] == "uint8" and seen["c"]["w_dtype"] == "fp32"
    q = SmoothQuantQuantizer(seen)
    assert (q._act_quant("a"), q._act_quant("b")) == ("per_token", "static") and q._selected(net) == ["a", "b"]


def test_oracle_on_hand_made_rows():
    x = torch.zeros(3, 16)
    x[0, :len(T.TIES)] = torch.tensor(T.TIES)      # amax exactly 127 -> s == 1, ties go to even
    x[1, 5] = -3.0                                 # s = 3 / 127, the amax maps to -127
    q, s = T.quant_token(x, None, 32)
    assert float(s[0]) == 1.0 and q[0, :len(T.TIES)].tolist() == T.TIES_Q and not bool(q[0, len(T.TIES):].any())
    assert float(s[1]) == float(torch.tensor(3.0) / torch.tensor(127.0)) and int(q[1, 5]) == -127 and int(q[1].abs().sum()) == 127
    assert float(s[2]) == T.EPS and not bool(q[2].any())                         # a zero row
    assert q.shape == (3, 32) and not bool(q[:, 16:].any())                      # the padding is the code 0
    # in_scale: the multiply comes first, the scale follows the smoothed row
    q2, s2 = T.quant_token(x, torch.full((16,), 0.5), 32)
    assert float(s2[0]) == 0.5 and q2[0, 0] == 127 and float(s2[2]) == T.EPS


def test_comparator_rejects_the_three_row_wise_mistakes():
    c = T.QCASES[1]                                                              # M = 3, K = 100 -> Kp 128
    x, _ = T.quant_inputs(c, torch.float32, False)
    q, s = T.quant_token(x, None, c.Kp)
    T.assert_quant_equal(q.clone(), s.clone(), q, s)
    with pytest.raises(AssertionError, match="row scales differ"):               # a neighbour row's scale
        T.assert_quant_equal(q, torch.roll(s, 1), q, s)
    bad = q.clone()
    bad[0, c.K] = -128                                                           # the static cell's padding byte, 0x80
    with pytest.raises(AssertionError, match=rf"first at \(0, {c.K}\)"):
        T.assert_quant_equal(bad, s, q, s)
    xp = torch.zeros(c.M, c.Kp)
    xp[:, :c.K] = x
    xp[:, c.K:] = 1e3                                                            # amax taken over the padding (whatever lies there)
    qp, sp = T.quant_token(xp)
    qp[:, c.K:] = 0
    with pytest.raises(AssertionError, match="row scales differ"):
        T.assert_quant_equal(qp, sp, q, s)


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.DTYPE_IDS)
def test_quant_dequant_x_token_is_the_oracle(dtype):
    from neural_compressor_amd.torch.algorithms.smooth_quant.utility import quant_dequant_x_token

    for c in T.QCASES[:4]:
        x, in_scale = T.quant_inputs(c, dtype, True)
        for t in (x.float(), x.float() * in_scale.view(1, -1)):
            q, s = T.quant_token(t)
            assert torch.equal(quant_dequant_x_token(t), T.dequant(q, s, c.K))
    x3 = T.outlier_input(0, dtype).view(4, 16, T.OUT_K)                         # leading dimensions: one scale per token
    assert torch.equal(quant_dequant_x_token(x3).view(T.OUT_T, T.OUT_K), T.token_qdq(x3.view(T.OUT_T, T.OUT_K)))


def test_wrapper_layer_uses_the_token_op_for_a_per_token_layer():
    from neural_compressor_amd.torch.algorithms.smooth_quant.utility import WrapperLayer, quant_dequant_x_token, quant_dequant_x_v1

    lin = torch.nn.Linear(T.OUT_K, 8)
    x = T.outlier_input(1, torch.float32)
    mn, mx = x.min(dim=0)[0], x.max(dim=0)[0]
    sc = 0.5 + torch.rand(1, T.OUT_K, generator=torch.Generator().manual_seed(0))
    for cell, fq in (("per_token", lambda t, s: quant_dequant_x_token(t if s is None else s * t)),
                     ("static", lambda t, s: quant_dequant_x_v1(t if s is None else s * t, mn if s is None else mn * s, mx if s is None else mx * s))):
        w = WrapperLayer(lin, mn, mx, act_quant=cell)
        w._bw_weight = lin.weight.detach().float()
        for s in (None, sc):
            want = torch.nn.functional.linear(fq(x, s), w._bw_weight, lin.bias.float())
            assert torch.equal(w.q_dq_forward_blockwise(x, s), want), (cell, s is None)
    assert WrapperLayer(lin, mn, mx).act_quant == "static"


def test_new_entry_points_validate_before_any_hip_call():
    from neural_compressor_amd import _lib

    L = _lib.lib
    assert L.inc_sq_quant_act_token(None, 2, 1, 16, 16, None, None, None, None) == -1                       # null pointers
    assert L.inc_sq_quant_act_token(4096, 2, 1, 16, 24, None, 4096, 4096, None) == -1                       # Kp % 16
    assert L.inc_sq_quant_act_token(4096, 2, 1, 32, 16, None, 4096, 4096, None) == -1                       # Kp < K
    assert L.inc_sq_quant_act_token(4096, 2, 1, 16, 16, None, 4100, 4096, None) == -1                       # xq not 16-byte aligned
    assert L.inc_w8a8_gemm_rowscale(4096, 4096, None, 4096, None, 4096, 2, 1, 1, 128, None, 0, None) == -1  # no row_scale
    assert L.inc_w8a8_gemm_rowscale(None, None, 4096, None, None, None, 2, 1, 1, 128, None, 0, None) == -1
    assert L.inc_w8a8_gemm_rowscale(4096, 4096, 4096, 4096, None, 4096, 0, 1, 1, 128, None, 0, None) == -2  # fp32 output
    assert L.inc_w8a8_gemm_rowscale(4096, 4096, 4096, 4096, None, 4096, 2, 1, 1, 100, None, 0, None) == -2  # K % 128
    assert len(_lib.SIGNATURES["inc_w8a8_gemm_rowscale"][1]) == len(_lib.SIGNATURES["inc_w8a8_gemm"][1]) == 13


def test_ops_refuse_host_tensors():
    from neural_compressor_amd import ops

    with pytest.raises(RuntimeError, match="HBM"):
        ops.sq_quant_act_token(torch.zeros(2, 16), None, 16)
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    with pytest.raises(RuntimeError, match="HIP device"):
        W8A8Linear(128, 8, device="cpu", act_quant="per_token")


@pytest.mark.parametrize("dtype", T.DTYPES[:2], ids=T.DTYPE_IDS[:2])
@pytest.mark.parametrize("seed", T.ACC_SEEDS)
def test_accuracy_condition_in_the_fake_quant_arithmetic(seed, dtype):
    """One token 64 times larger than the other 63: under the static cell it sets everybody's step.  The per-token error over the 63
    ordinary tokens is at most 0.1 of the static cell's.  The definition alone gives a ratio <= 0.021 on these inputs (static 0.35 .. 0.48,
    per-token 0.007): a margin of more than 4x, none of it for a kernel."""
    x = T.outlier_input(seed, dtype)
    e_static = T.rel_err(T.ordinary(T.static_qdq(x)), T.ordinary(x.float()))
    e_token = T.rel_err(T.ordinary(T.token_qdq(x)), T.ordinary(x.float()))
    print(f"seed {seed} {dtype}: static {e_static:.4f}  per-token {e_token:.5f}  ratio {e_token / e_static:.4f}")
    assert e_token <= T.ACC_RATIO * e_static
