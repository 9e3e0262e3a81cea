"""The frame of the fused MoE experts modules (neural_compressor_amd/torch/algorithms/fused_experts.py) on a stub subclass, no GPU: the
choice between the two routes, the types the fused route is handed, the dense route's loop against a plain double loop, empty inputs
and the output's dtype and shape.  The kernels behind the four real subclasses are in tests/test_gpu_moe_experts.py, test_gpu_fp8_moe.py,
test_gpu_mx_moe.py and test_gpu_mx_gpt_oss.py."""

import pytest
import torch

from neural_compressor_amd.torch.algorithms.fused_experts import MAX_EXPERTS, FusedExperts, is_silu

E, H, I = 4, 8, 4
SHAPES = [(1, 2), (5, 1), (7, 2)]
MARK = 7.0


def _ints(shape, g, lo=-2, hi=3):
    """Small integers as fp32: every product and sum below is exact in fp32, so equality cannot depend on the order of a sum."""
    return torch.randint(lo, hi, shape, generator=g).float()


def _stub_class():
    """A fresh subclass per test, so that a class attribute set in one test is not seen by another."""

    class Stub(FusedExperts):
        MOE_MAX_ROWS = 256

        def __init__(self):
            super().__init__(E, H, I)
            g = torch.Generator().manual_seed(0)
            self.a, self.b = _ints((E, H, I), g), _ints((E, I, H), g)
            self.fusable = True
            self.fused_calls, self.mlp_calls = [], []

        def _compute_dtype(self, x):
            return torch.float32

        def _fusable(self):
            return self.fusable

        def _fused_forward(self, x2d, idx, w, cdt):
            self.fused_calls.append((x2d, idx, w, cdt))
            return torch.full((x2d.shape[0], self.hidden_dim), MARK, dtype=cdt)

        def _expert_mlp(self, rows, e, cdt):
            self.mlp_calls.append(e)
            return (rows.to(cdt) @ self.a[e]) @ self.b[e]

    return Stub


def _inputs(T, k, seed=1):
    """x [T, H], distinct expert ids per token with a -1 and (past one token, which keeps a real expert) an E planted, weights in
    quarters."""
    g = torch.Generator().manual_seed(seed)
    x = _ints((T, H), g)
    idx = torch.rand(T, E, generator=g).topk(k, dim=-1).indices
    idx[0, 0] = -1
    if T > 1:
        idx[T // 2, k - 1] = E
    w = torch.randint(1, 5, (T, k), generator=g).float() / 4
    return x, idx, w


def _reference(m, x, idx, w):
    out = torch.zeros(x.shape[0], H)
    for t in range(idx.shape[0]):
        for s in range(idx.shape[1]):
            e = int(idx[t, s])
            if 0 <= e < E:
                out[t] += ((x[t].float() @ m.a[e]) @ m.b[e]) * w[t, s]
    return out


def _route(m, x, idx, w):
    m.fused_calls.clear()
    m.mlp_calls.clear()
    y = m(x, idx, w)
    assert not (m.fused_calls and m.mlp_calls)
    return "fused" if m.fused_calls else "dense" if m.mlp_calls else None, y


def test_module_level_pieces():
    assert MAX_EXPERTS == 512 and FusedExperts.MOE_FUSED is True
    assert is_silu(torch.nn.SiLU()) and is_silu(torch.nn.SiLU(inplace=True)) and not is_silu(torch.nn.GELU()) and not is_silu(None)
    assert is_silu(type("SiLUActivation", (), {})())
    m = _stub_class()()
    assert (m.num_experts, m.hidden_dim, m.intermediate_dim) == (E, H, I) and isinstance(m.act_fn, torch.nn.SiLU)
    act = torch.nn.GELU()
    assert FusedExperts(E, H, I, act_fn=act).act_fn is act


def test_route_choice_boundary():
    Stub = _stub_class()
    Stub.MOE_MAX_ROWS = 1  # T * k <= 1 * E = 4 routed rows: fused
    m = Stub()
    route, y = _route(m, *_inputs(4, 1))
    assert route == "fused" and torch.equal(y, torch.full((4, H), MARK))
    assert _route(m, *_inputs(2, 2))[0] == "fused"
    x, idx, w = _inputs(5, 1)  # one row more
    route, y = _route(m, x, idx, w)
    assert route == "dense" and torch.equal(y, _reference(m, x, idx, w))


def test_route_choice_overrides():
    Stub = _stub_class()
    m = Stub()
    x, idx, w = _inputs(7, 2)
    assert _route(m, x, idx, w)[0] == "fused"
    m.fusable = False
    assert _route(m, x, idx, w)[0] == "dense"
    m.fusable = True
    assert _route(m, x, idx, w)[0] == "fused"
    Stub.MOE_FUSED = False
    assert _route(m, x, idx, w)[0] == "dense"
    assert FusedExperts.MOE_FUSED is True  # set on the stub class only


@pytest.mark.parametrize("T,k", SHAPES)
def test_fused_route_argument_types(T, k):
    m = _stub_class()()
    x, idx, w = _inputs(T, k)
    for idt, want_idt in ((torch.int16, torch.int64), (torch.int32, torch.int32), (torch.int64, torch.int64)):
        for wdt, want_wdt in ((torch.float64, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
                              (torch.float32, torch.float32)):
            # a flat id vector and a transposed (non-contiguous) weight view: the route sees [T, k], contiguous
            route, _ = _route(m, x, idx.to(idt).reshape(-1), w.to(wdt).t().contiguous().t())
            assert route == "fused"
            x2d, fi, fw, cdt = m.fused_calls[0]
            assert fi.dtype is want_idt and fw.dtype is want_wdt and cdt is torch.float32
            assert tuple(fi.shape) == (T, k) and tuple(fw.shape) == (T, k) and fi.is_contiguous() and fw.is_contiguous()
            assert torch.equal(fi.long(), idx) and torch.equal(fw.double(), w.to(wdt).double()) and torch.equal(x2d, x)


@pytest.mark.parametrize("T,k", SHAPES)
def test_dense_route_is_the_double_loop(T, k):
    Stub = _stub_class()
    Stub.MOE_FUSED = False
    m = Stub()
    x, idx, w = _inputs(T, k)
    assert (idx == -1).any() and ((idx == E).any() or T == 1)
    route, y = _route(m, x, idx, w)
    assert route == "dense" and y.dtype is torch.float32
    assert torch.equal(y, _reference(m, x, idx, w))
    assert sorted(m.mlp_calls) == sorted({int(e) for e in idx.flatten() if 0 <= int(e) < E})  # once per expert that was hit


@pytest.mark.parametrize("fused", [True, False])
def test_empty_inputs(fused):
    Stub = _stub_class()
    Stub.MOE_FUSED = fused
    m = Stub()
    x, idx, w = _inputs(5, 1)
    for xs, ids, ws in ((x[:0], idx[:0], w[:0]), (x.half(), idx[:, :0], w[:, :0]), (x.reshape(1, 5, H)[:, :0], idx[:0], w[:0])):
        route, y = _route(m, xs, ids, ws)
        assert route is None
        assert y.shape == xs.shape and y.dtype is xs.dtype and not y.any()


@pytest.mark.parametrize("fused", [True, False])
def test_output_has_the_inputs_dtype_and_shape(fused):
    Stub = _stub_class()
    Stub.MOE_FUSED = fused
    m = Stub()
    x, idx, w = _inputs(6, 2)
    for dtype in (torch.float64, torch.bfloat16):
        x3 = x.to(dtype).reshape(2, 3, H)
        route, y = _route(m, x3, idx, w)
        assert route == ("fused" if fused else "dense")
        assert y.dtype is dtype and y.shape == x3.shape
        want = torch.full((6, H), MARK) if fused else _reference(m, x, idx, w)
        assert torch.equal(y, want.to(dtype).reshape(2, 3, H))
