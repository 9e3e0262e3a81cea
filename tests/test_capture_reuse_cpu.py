"""The GPTQ block driver remembers what a capture pass learns about a block class (gptq.py, RAWGPTQuantizer.quantize_block): the order
in which the hooked modules fire (later blocks stop their FIRST forward at the last hooked module too) and the zero-copy verdict of
the Hessian accumulators (later blocks skip the first staging copy).  Host logic only: the driver runs on the CPU with the device
kernels replaced by torch stand-ins -- a Hessian update, a solve that depends on the Hessian, a module that keeps what it is given."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from neural_compressor_amd.torch.algorithms.weight_only import gptq as G  # noqa: E402
from neural_compressor_amd.torch.algorithms.weight_only.fused_forward import FusedForward  # noqa: E402
from tests.model_zoo import calib_ids, tiny_llama  # noqa: E402

SEQ, SAMPLES = 32, 4  # STAGE_TOKENS = 64 below: two samples per stacked forward, two stacked forwards per pass


class _Packed(torch.nn.Module):
    def __init__(self, in_features, out_features, **kw):
        super().__init__()
        self.kept = None

    def pack_codes(self, codes, scale, zero, bias, g_idx=None):
        self.kept = (codes.clone(), scale.clone())


def _hessian_accum(H, x2d, beta, alpha):
    x = x2d.float()
    H.mul_(beta).add_(alpha * (x.t() @ x))


def _solve(self, W, **kw):
    """4-bit round to nearest of W scaled column-wise by a function of diag(H): any change of a Hessian changes codes and scales."""
    d = torch.diagonal(self.H)
    Wf = W.float() * (1.0 + 0.25 * torch.tanh(d))[None, :]
    scale = Wf.abs().amax(dim=1, keepdim=True).clamp_min(1e-8) / 7.0
    codes = torch.clamp(torch.round(Wf / scale) + 8, 0, 15).to(torch.uint8)
    self.codes, self.export_perm = codes, None
    return scale, None, torch.full_like(scale, 8.0), ((codes.float() - 8) * scale).to(W.dtype)


@pytest.fixture
def cpu_driver(monkeypatch):
    made = []

    class Acc(G.HessianAccumulator):
        def __init__(self, columns, device):
            super().__init__(columns, device)
            self.staged = False
            made.append(self)

        def add_batch(self, inp):
            super().add_batch(inp)
            self.staged = self.staged or self._stage is not None

    monkeypatch.setattr(G.HessianAccumulator, "STAGE_TOKENS", 2 * SEQ)
    monkeypatch.setattr(G, "HessianAccumulator", Acc)
    monkeypatch.setattr(G.ops, "gptq_hessian_accum", _hessian_accum)
    monkeypatch.setattr(G.ops, "gptq_hessian_accum_multi", lambda items: False)
    monkeypatch.setattr(G.GPTQ, "fasterquant", _solve)
    monkeypatch.setattr(G, "MI355XWeightOnlyLinear", _Packed)
    monkeypatch.delenv("INC_MI355X_GPTQ_FORWARD_BATCH", raising=False)
    return made


def _quantizer(layers=3, weight_config=None):
    model = tiny_llama(layers=layers)
    rq = object.__new__(G.RAWGPTQuantizer)  # the constructor wants an accelerator; everything quantize_block reads is set here
    rq.model = model
    rq.gptq_related_blocks = G.trace_gptq_target_blocks(model)
    rq.weight_config = weight_config if weight_config is not None else {".*": {"sym": True}}
    rq.check_layer_config()
    rq.device = torch.device("cpu")
    rq.share_hessians, rq.factor_streams, rq._fstreams, rq._late_stream = True, 1, [], None
    rq._block_writes_input, rq._fused, rq._stacks = None, FusedForward(), {}
    rq._capture_order, rq._zero_copy_ok = {}, set()
    rq.hessian_allreduce = rq.row_shard_solve = rq.dist_ctx = rq.layer_ctx = None
    rq.prepare_for_calibration()
    with torch.no_grad():
        for ids in calib_ids(n=SAMPLES, seq=SEQ):
            model(ids)
    rq.remove_prepare_for_calibration()
    return rq


def _run(rq, before_block=None):
    """Quantise every block; returns per block: down_proj calls in the capture pass and in the second forward, the packed codes and scales
    of every layer, and the block's outputs."""
    blocks = rq.gptq_related_blocks["transformers"]
    phase, calls = {"capture": None}, []
    run_block = rq._run_block

    def tracked(block, on_output=None, capture=False):
        phase["capture"] = capture
        try:
            return run_block(block, on_output=on_output, capture=capture)
        finally:
            phase["capture"] = None

    rq._run_block = tracked
    out = []
    for i, block in enumerate(blocks):
        calls.append({True: 0, False: 0})
        h = block.mlp.down_proj.register_forward_hook(lambda *a, i=i: calls[i].__setitem__(phase["capture"], calls[i][phase["capture"]] + 1))
        if before_block is not None:
            before_block(rq, i)
        rq.quantize_block(block, i)
        h.remove()
        packed = {n: m.kept for n, m in block.named_modules() if isinstance(m, _Packed)}
        hidden = rq.cache_key_arguments["hidden_states"] if "hidden_states" in rq.cache_key_arguments else rq.cache_positional_arguments[0]
        out.append(dict(capture_calls=calls[i][True], second_calls=calls[i][False], packed=packed, hidden=[t.clone() for t in hidden]))
    return out


def _forget(rq, i):
    rq._capture_order.clear()
    rq._zero_copy_ok.clear()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["packed"].keys() == y["packed"].keys() and len(x["packed"]) > 0
        for n in x["packed"]:
            assert torch.equal(x["packed"][n][0], y["packed"][n][0]), n
            assert torch.equal(x["packed"][n][1], y["packed"][n][1]), n
        assert all(torch.equal(s, t) for s, t in zip(x["hidden"], y["hidden"]))


FORWARDS = SAMPLES * SEQ // (2 * SEQ)


def test_later_blocks_neither_probe_nor_copy(cpu_driver):
    made = cpu_driver
    got = _run(_quantizer())
    assert FORWARDS >= 2
    # block 0 learns the order with one complete forward; every later block stops all of its forwards in front of down_proj
    assert [b["capture_calls"] for b in got] == [1, 0, 0]
    assert all(b["second_calls"] == FORWARDS for b in got)
    per_block = len(made) // 3
    fed = [[a for a in made[i * per_block:(i + 1) * per_block] if a._n] for i in range(3)]
    assert all(len(f) == 4 for f in fed)  # q/k/v share one Hessian, gate/up another, o_proj and down_proj have their own
    assert all(a.staged for a in fed[0])                        # the verdict is earned with a copy ...
    assert not any(a.staged for f in fed[1:] for a in f)        # ... and carried: no later accumulator allocates a staging buffer
    n0 = len(made)
    ref = _run(_quantizer(), before_block=_forget)
    assert [b["capture_calls"] for b in ref] == [1, 1, 1]
    assert all(a.staged for a in made[n0:] if a._n)
    _same(got, ref)


def test_switches_still_switch_everything_off(cpu_driver, monkeypatch):
    made = cpu_driver
    ref = _run(_quantizer(), before_block=_forget)
    n0 = len(made)
    monkeypatch.setattr(G, "CAPTURE_EARLY_STOP", False)
    monkeypatch.setattr(G.HessianAccumulator, "ZERO_COPY", False)
    rq = _quantizer()
    got = _run(rq)
    assert [b["capture_calls"] for b in got] == [FORWARDS] * 3 and not rq._capture_order
    assert all(a.staged for a in made[n0:] if a._n)
    _same(got, ref)


def test_another_set_of_hooked_names_probes_again(cpu_driver):
    # block 1 leaves o_proj out: its key differs from block 0's, block 2's is block 0's again
    class Q(G.RAWGPTQuantizer):
        def get_layer_config(self, name):
            return None if name.endswith("layers.1.self_attn.o_proj") else super().get_layer_config(name)

    rq = _quantizer()
    rq.__class__ = Q
    got = _run(rq)
    assert [b["capture_calls"] for b in got] == [1, 1, 0]
    assert len(rq._capture_order) == 2
    assert "self_attn.o_proj" not in got[1]["packed"] and "self_attn.o_proj" in got[2]["packed"]


def test_a_remembered_order_that_never_stops_is_dropped(cpu_driver):
    def poison(rq, i):
        if i == 1:  # as if block 1 ran its modules in another order: the remembered last module fires first, the guard never lets it stop
            (key, order), = rq._capture_order.items()
            rq._capture_order[key] = tuple(reversed(order))

    rq = _quantizer()
    got = _run(rq, before_block=poison)
    # block 1 runs every forward to its end and forgets the order, block 2 probes again and remembers
    assert [b["capture_calls"] for b in got] == [1, FORWARDS, 1]
    assert len(rq._capture_order) == 1 and next(iter(rq._capture_order.values()))[-1] == "mlp.down_proj"
    _same(got, _run(_quantizer(), before_block=_forget))
