"""The frame of the quantised linear modules (neural_compressor_amd/torch/algorithms/quant_linear.py) on a stub subclass, no GPU: the
forward contract (rows, the empty batch, the compute type, the cast back), the decode rule, the device refusal, the MX pair tables,
the group body without a plan, the e4m3 table and the shared save / load.  The kernels behind the five real subclasses are in
tests/test_gpu_w8a8_token.py, test_gpu_sq.py, test_gpu_fp8.py, test_gpu_fp8_block.py, test_gpu_mx.py and test_gpu_mx_weight_only.py."""

import json
import os

import pytest
import torch

from neural_compressor_amd import ops
from neural_compressor_amd.torch.algorithms.fp8_quant.fp8_quant import fp8_gated_pair, fp8_linear_group
from neural_compressor_amd.torch.algorithms.mx_quant.mx_quant import MXLinear, MXWeightOnlyLinear, _code_values, check_pair, mx_linear_group
from neural_compressor_amd.torch.algorithms import quant_linear
from neural_compressor_amd.torch.algorithms.quant_linear import QuantLinear, e4m3_table, linear_group
from neural_compressor_amd.torch.utils import utility

K, N = 5, 3
HALVES = (torch.bfloat16, torch.float16)


def _stub_class():
    """A fresh subclass per call, so that a class attribute set on one is not seen by another."""

    class Stub(QuantLinear):
        DECODE_GEMV = True
        DECODE_MAX_M, GEMV_LIMIT = 16, "FP8_GEMV_MAX_M"  # the kernel's limit is whatever ops says at the call: 16

        def __init__(self, in_features=K, out_features=N, bias=False, device="cpu", float_type=torch.float16):
            super().__init__(in_features, out_features, float_type)
            g = torch.Generator().manual_seed(0)
            self.register_buffer("qweight", torch.randint(-2, 3, (out_features, in_features), generator=g).float())
            self._register_bias(bias, torch.device(device))
            self.calls = []

        def _quantize_weight(self, w):
            self.qweight.copy_(w.round())

        def _product(self, x2d, out_dtype):
            """Small integers: every product and sum is exact in fp32, bf16 and fp16."""
            self.calls.append((tuple(x2d.shape), x2d.dtype, out_dtype))
            y = x2d.float() @ self.qweight.t()
            return (y if self.bias is None else y + self.bias.float()).to(out_dtype)

        # the pieces a group uses (linear_group): the "codes" are x itself
        def _group_key(self):
            return self.in_features, self.qweight.device

        def _quantize_rows(self, x2d):
            self.calls.append(("quantize_rows", tuple(x2d.shape)))
            return x2d, "scales"

        def _gemm(self, xq, xs, out_dtype):
            self.calls.append(("gemm", xs, out_dtype))
            return (xq @ self.qweight.t()).to(out_dtype)

        @staticmethod
        def _gemv_multi(xq, xs, mods, out_dtype):
            mods[0].calls.append(("gemv_multi", xs, out_dtype, len(mods)))
            return [(xq @ m.qweight.t()).to(out_dtype) for m in mods]

    return Stub


def _ints(*shape, seed=1):
    return torch.randint(-2, 3, shape, generator=torch.Generator().manual_seed(seed)).float()


def test_construction_needs_no_device():
    m = _stub_class()(float_type=torch.bfloat16, bias=True)
    assert (m.in_features, m.out_features, m.kp, m.float_type) == (K, N, 128, torch.bfloat16)
    assert list(m.state_dict()) == ["qweight", "bias"] and m.bias.dtype is torch.bfloat16 and tuple(m.bias.shape) == (N,)
    assert _stub_class()().bias is None and "bias" not in _stub_class()().state_dict()
    assert QuantLinear(300, 7).kp == 384 and QuantLinear.DECODE_GEMV is False
    assert QuantLinear.K_ALIGN == 128 == ops.MX_KTILE and all(QuantLinear(k, 7).kp == ops.mx_padded_k(k) for k in (1, 128, 129, 5120))


@pytest.mark.parametrize("float_type", HALVES)
@pytest.mark.parametrize("lead", [(0,), (2, 0)])
def test_empty_batch(lead, float_type):
    m = _stub_class()(float_type=float_type)
    for dtype, want in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16)):
        x = torch.zeros((*lead, K), dtype=dtype)
        y = m(x)
        assert m.calls == []
        assert tuple(y.shape) == (*lead, N) and y.dtype is want and y.device == x.device


@pytest.mark.parametrize("float_type", HALVES)
def test_compute_dtype(float_type):
    m = _stub_class()(float_type=float_type)
    x = _ints(3, K)
    want = x @ m.qweight.t()
    for dtype in HALVES:
        y = m(x.to(dtype))
        assert m.calls[-1] == ((3, K), dtype, dtype)  # a 16-bit x is handed over as it is and asks for its own type
        assert y.dtype is dtype and torch.equal(y.float(), want)
    y = m(x)
    assert m.calls[-1] == ((3, K), torch.float32, float_type)  # an fp32 x asks for float_type and comes back fp32
    assert y.dtype is torch.float32 and torch.equal(y, want)


@pytest.mark.parametrize("lead,rows", [((), 1), ((3,), 3), ((2, 3), 6)])
def test_leading_dimensions(lead, rows):
    m = _stub_class()(bias=True)
    m.bias.copy_(_ints(N, seed=2))
    x = _ints(*lead, K)
    y = m(x)
    assert m.calls == [((rows, K), torch.float32, torch.float16)]
    assert tuple(y.shape) == (*lead, N)
    assert torch.equal(y, (x.reshape(rows, K) @ m.qweight.t() + m.bias.float()).reshape(*lead, N))


def test_decodes():
    A, B = _stub_class(), _stub_class()
    a, b = A(), B()
    assert a._decodes(1) and a._decodes(16) and not a._decodes(17)
    A.DECODE_MAX_M = 4
    assert a._decodes(4) and not a._decodes(5)
    assert b._decodes(16) and B.DECODE_MAX_M == 16  # set on A only
    A.DECODE_MAX_M = 64  # above the kernel's limit: clipped to it
    assert a._decodes(16) and not a._decodes(17)
    A.DECODE_GEMV = False
    assert not any(a._decodes(r) for r in (1, 4, 16, 17))
    assert b._decodes(1) and QuantLinear.DECODE_GEMV is False and not QuantLinear(K, N)._decodes(1)


def test_the_kernel_limit_is_read_from_ops_at_the_call(monkeypatch):
    b = _stub_class()()
    monkeypatch.setattr(ops, "FP8_GEMV_MAX_M", 8)
    assert b._decodes(8) and not b._decodes(9)  # DECODE_MAX_M is still 16: clipped to the limit of the moment


def test_the_real_classes_keep_their_own_switches():
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear, FP8Linear
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    for cls, limit in ((FP8Linear, ops.FP8_GEMV_MAX_M), (FP8BlockLinear, ops.FP8_GEMV_MAX_M), (MXLinear, ops.MX_GEMV_MAX_M),
                       (MXWeightOnlyLinear, ops.MX_GEMV_MAX_M)):
        assert issubclass(cls, QuantLinear) and cls.DECODE_GEMV is True and cls.DECODE_MAX_M == limit == getattr(ops, cls.GEMV_LIMIT) == 16
        assert "DECODE_MAX_M" in vars(cls)
    assert "DECODE_GEMV" in vars(FP8Linear) and "DECODE_GEMV" in vars(FP8BlockLinear) and "DECODE_GEMV" in vars(MXLinear)
    assert issubclass(W8A8Linear, QuantLinear) and W8A8Linear.DECODE_GEMV is False and W8A8Linear.K_ALIGN == 128
    for cls in (W8A8Linear, FP8Linear, FP8BlockLinear, MXLinear, MXWeightOnlyLinear):  # one forward, one _decodes
        assert cls.forward is QuantLinear.forward and cls._decodes is QuantLinear._decodes


@pytest.mark.parametrize("device", ["cpu", torch.device("cpu"), "meta"])
def test_device_refusal(device):
    Stub = _stub_class()
    with pytest.raises(RuntimeError) as e:
        Stub._hip_device(device)
    assert str(e.value) == f"Stub needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation."
    assert Stub._hip_device("cuda:1") == torch.device("cuda", 1)


def test_real_classes_refuse_the_cpu_under_their_own_names():
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockLinear, FP8Linear
    from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

    for cls in (W8A8Linear, FP8Linear, FP8BlockLinear, MXLinear, MXWeightOnlyLinear):
        with pytest.raises(RuntimeError, match=f"^{cls.__name__} needs a HIP device \\('cuda\\[:N\\]'\\), got 'cpu'. There is no CPU"):
            cls(K, N, device="cpu")


def test_mx_pair_tables():
    pairs = (("fp8_e4m3", "fp8_e4m3"), ("fp4", "fp8_e4m3"), ("fp4", "fp4"))
    wo = (("fp4", "bf16"), ("fp8_e4m3", "bf16"))
    assert MXLinear.PAIRS == pairs and MXWeightOnlyLinear.PAIRS == wo
    for p in pairs:
        check_pair(MXLinear, *p)
    for p in wo:
        check_pair(MXWeightOnlyLinear, *p)
    with pytest.raises(NotImplementedError) as e:
        check_pair(MXLinear, "fp4", "bf16")
    assert str(e.value) == f"MXQuant on MI355X: (w_dtype, act_dtype) must be one of {pairs}, got ('fp4', 'bf16')"
    with pytest.raises(NotImplementedError) as e:
        check_pair(MXWeightOnlyLinear, "fp8_e4m3", "fp8_e4m3")
    assert str(e.value) == f"MXQuant on MI355X, weight-only: (w_dtype, act_dtype) must be one of {wo}, got ('fp8_e4m3', 'fp8_e4m3')"


def test_mx_experts_take_their_table_from_the_class():
    from neural_compressor_amd.torch.algorithms.mx_quant import MXExperts, MXGptOssExperts, MXWeightOnlyExperts, MXWeightOnlyGptOssExperts

    assert MXExperts.PAIRS is MXLinear.PAIRS and MXGptOssExperts.PAIRS is MXLinear.PAIRS
    assert MXWeightOnlyExperts.PAIRS is MXWeightOnlyLinear.PAIRS and MXWeightOnlyGptOssExperts.PAIRS is MXWeightOnlyLinear.PAIRS
    assert MXExperts.CELL == MXGptOssExperts.CELL == MXLinear.CELL == ""
    assert MXWeightOnlyExperts.CELL == MXWeightOnlyGptOssExperts.CELL == MXWeightOnlyLinear.CELL == ", weight-only"
    with pytest.raises(NotImplementedError, match="^MXQuant on MI355X, weight-only: .*got \\('fp4', 'fp4'\\)$"):
        check_pair(MXWeightOnlyGptOssExperts, "fp4", "fp4")


def test_from_float_skeleton():
    Stub = _stub_class()
    for dtype, ft in ((torch.float32, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16)):
        lin = torch.nn.Linear(K, N, bias=True)
        with torch.no_grad():
            lin.weight.copy_(_ints(N, K, seed=3))
            lin.bias.copy_(_ints(N, seed=4))
        lin.to(dtype)
        m = Stub.from_float(lin, device="cpu")
        assert m.float_type is ft and m.bias.dtype is ft
        assert torch.equal(m.qweight, lin.weight.float()) and torch.equal(m.bias.float(), lin.bias.float())
    assert Stub.from_float(torch.nn.Linear(K, N, bias=False), "cpu").bias is None


def test_group_functions_without_a_plan_are_the_single_forwards():
    mods = [_stub_class()(out_features=n) for n in (3, 4, 2)]
    x = _ints(2, 3, K)
    want = [m(x) for m in mods]
    for got in (fp8_linear_group(x, mods), mx_linear_group(x, iter(mods)), linear_group(x, mods, type(mods[0]), 8, 16)):
        assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))
    gate, up = mods[0], _stub_class()(out_features=3)
    assert torch.equal(fp8_gated_pair(x, gate, up), torch.nn.functional.silu(gate(x)) * up(x))


def test_group_body_under_a_plan(monkeypatch):
    """One _quantize_rows, by the first member, then one `_gemv_multi` where every member decodes, else one `_gemm` per member; the
    cast back and the reshape.  A plan needs x on the device, so the plan of this test is handed in."""
    Stub = _stub_class()
    mods = [Stub(out_features=n) for n in (3, 4)]
    x = _ints(2, 3, K)
    want = [m(x) for m in mods]
    for decode, calls in ((True, [[("gemv_multi", "scales", torch.float16, 2)], []]),
                          (False, [[("gemm", "scales", torch.float16)], [("gemm", "scales", torch.float16)]])):
        asked = []
        monkeypatch.setattr(quant_linear, "linear_group_plan", lambda *a: asked.append(a) or (x.reshape(-1, K), torch.float16, decode))
        for m in mods:
            m.calls.clear()
        got = linear_group(x, mods, Stub, 8, 16)
        assert asked == [(x, mods, Stub, 8, 16)]
        assert [m.calls for m in mods] == [[("quantize_rows", (6, K))] + calls[0], calls[1]]
        assert all(g.dtype is torch.float32 and torch.equal(g, w) for g, w in zip(got, want))


def test_e4m3_table():
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    for got in (e4m3_table(), e4m3_table("cpu"), _code_values(ops.MX_FP8_E4M3)):
        assert got.dtype is torch.float32 and got.device.type == "cpu"
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))  # bits: the two NaN codes included
    assert _code_values(ops.MX_FP4_E2M1).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def test_save_and_load_with_a_stub_model(tmp_path):
    Stub = _stub_class()

    def floats():
        torch.manual_seed(5)
        return torch.nn.Sequential(torch.nn.Linear(K, N), torch.nn.LayerNorm(N), torch.nn.Linear(N, 2, bias=False))

    model = floats()
    model[0], model[2] = Stub.from_float(model[0].to(torch.bfloat16), "cpu"), Stub.from_float(model[2], "cpu")
    qconfig = {"stub_quant": {"b": 1, "a": [2, 3]}, "stub_modules": ["0", "2"]}
    utility.save_quantized(model, str(tmp_path), qconfig)
    assert sorted(os.listdir(tmp_path)) == sorted([utility.QCONFIG_NAME, utility.WEIGHT_NAME])
    assert (tmp_path / utility.QCONFIG_NAME).read_text() == json.dumps(qconfig, indent=2)

    cfg, state, dev = utility.open_saved(str(tmp_path), "cpu")
    assert cfg == qconfig and list(cfg) == list(qconfig) and dev == torch.device("cpu")
    assert list(state) == list(model.state_dict()) == ["0.qweight", "0.bias", "1.weight", "1.bias", "2.qweight"]
    loaded = floats()
    with torch.no_grad():
        loaded[1].weight.zero_()
    for name in cfg["stub_modules"]:
        utility.take_linear(state, loaded, name, dev, Stub)
    assert list(state) == ["1.weight", "1.bias"]  # what is left is the float modules'
    assert utility.finish_load(loaded, state, dev) is loaded and not loaded.training
    # float_type: the saved bias's type where there is one, else what the float weight's type gives
    assert isinstance(loaded[0], Stub) and loaded[0].float_type is torch.bfloat16 and loaded[2].float_type is torch.float16
    assert list(loaded.state_dict()) == list(model.state_dict())
    assert all(torch.equal(a, b) and a.dtype is b.dtype for a, b in zip(loaded.state_dict().values(), model.state_dict().values()))
    with pytest.raises(AssertionError, match="1: expected nn.Linear in the float architecture, got LayerNorm"):
        utility.take_linear({}, floats(), "1", dev, Stub)


def test_save_load_modules_keep_their_names():
    from neural_compressor_amd.torch.algorithms.fp8_quant import save_load as f
    from neural_compressor_amd.torch.algorithms.mx_quant import save_load as m
    from neural_compressor_amd.torch.algorithms.smooth_quant import save_load as s

    for mod in (f, m, s):
        assert (mod.WEIGHT_NAME, mod.QCONFIG_NAME) == ("quantized_weight.pt", "qconfig.json")
        assert all(callable(getattr(mod, n)) for n in ("save", "load", "qconfig_of"))
