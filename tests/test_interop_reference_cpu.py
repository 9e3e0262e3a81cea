"""CPU: checkpoints saved by THIS repository on the MI355X (tests/golden/ckpt/ours_*, produced by scripts/make_our_checkpoints.py)
read back with the reference's load() semantics -- the drop-in claim for the on-disk formats in the direction
reference <- this repository, self-contained in the repository:

* layout: our files hold the same tensors (names, shapes, dtypes) and the same per-module settings as the checkpoints the
  UNMODIFIED reference's save() wrote for the same model (tests/golden/ckpt/ref_*, tests/golden/make_golden_checkpoints.py),
  which are exactly what its load() consumes;
* values: the reference's load + forward restated (oracle.woq_recover = INCWeightOnlyLinear.recover, then the fp32 forward of
  the model with the recovered weights) must reproduce the reference's OWN logits on its own checkpoint (ref_logits.npz), and
  on our checkpoint the logits this repository's model produced (ours_logits.npz)."""

import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CKPT = os.path.join(ROOT, "tests", "golden", "ckpt")


def _load_restated(state, bits, group_size, model):
    """The reference's load() restated: every module with a `qweight` becomes its recovered fp16 weight (fp32 compute); the
    packed module's bias buffer must be zero where the float model has no bias."""
    from oracle import woq_oracle as O

    packed = sorted(k[: -len(".qweight")] for k in state if k.endswith(".qweight"))
    sd = {k: v.float() for k, v in state.items() if k.rsplit(".", 1)[0] not in packed}
    params = dict(model.named_parameters())
    for m in packed:
        qw, sc, qz = state[m + ".qweight"], state[m + ".scales"], state[m + ".qzeros"]
        N, K = sc.shape[1], qw.shape[0] * 32 // bits
        g_idx = state.get(m + ".g_idx")
        w = O.woq_recover(qw.numpy(), sc.numpy(), qz.numpy(), N, K, bits, group_size, None if g_idx is None else g_idx.numpy())
        sd[m + ".weight"] = torch.from_numpy(w.astype(np.float32))
        if m + ".bias" in params:
            sd[m + ".bias"] = state[m + ".bias"].float()
        elif m + ".bias" in state:
            assert not state[m + ".bias"].any(), f"{m}: non-zero bias for a Linear without bias"
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing, missing
    assert all(k.rsplit(".", 1)[0] in packed for k in unexpected), unexpected
    return model, packed


def _logits(model):
    from tests.model_zoo import calib_ids

    with torch.no_grad():
        return model(calib_ids()[0]).logits.float().numpy()


def _same_layout(ours, ref):
    assert sorted(ours) == sorted(ref)
    for k in ref:
        assert tuple(ours[k].shape) == tuple(ref[k].shape) and ours[k].dtype == ref[k].dtype, (k, ours[k].shape, ours[k].dtype, ref[k].dtype)


def _rel(y, ref):
    return float(np.linalg.norm(y - ref) / np.linalg.norm(ref))


def test_reference_loads_our_default_format():
    from tests.model_zoo import tiny_llama

    states = {t: torch.load(os.path.join(CKPT, f"{t}_rtn_default", "quantized_weight.pt"), map_location="cpu", weights_only=True)
              for t in ("ours", "ref")}
    _same_layout(states["ours"], states["ref"])
    qcfg = {t: json.load(open(os.path.join(CKPT, f"{t}_rtn_default", "qconfig.json"))) for t in ("ours", "ref")}
    assert sorted(qcfg["ours"]) == sorted(qcfg["ref"])
    # the reference also stores its config object's bookkeeping (`non_tunable_params`, `_is_initialized`); load() does not read it
    bookkeeping = ("non_tunable_params", "_is_initialized")
    for k, v in qcfg["ref"].items():
        assert sorted(qcfg["ours"][k]) == sorted(v), k
        for algo, params in v.items():
            assert qcfg["ours"][k][algo] == {p: x for p, x in params.items() if p not in bookkeeping}, k
    ref = np.load(os.path.join(CKPT, "ref_logits.npz"))["rtn_default"]  # the reference's model, fp32 CPU
    model, packed = _load_restated(states["ref"], 4, 32, tiny_llama())
    assert len(packed) == 14
    assert _rel(_logits(model), ref) <= 1e-5, "the restated load no longer reproduces the reference's own logits"
    ours = np.load(os.path.join(CKPT, "ours_logits.npz"))["rtn_default"]  # MI355X, fp16 compute
    model, packed = _load_restated(states["ours"], 4, 32, tiny_llama())
    assert len(packed) == 14
    assert _rel(_logits(model), ours) <= 2e-2


def test_reference_loads_our_huggingface_format():
    from safetensors.torch import load_file
    from transformers import AutoConfig, LlamaForCausalLM

    states = {t: load_file(os.path.join(CKPT, f"{t}_gptq_hf", "model.safetensors")) for t in ("ours", "ref")}
    _same_layout(states["ours"], states["ref"])
    qcfg = {t: json.load(open(os.path.join(CKPT, f"{t}_gptq_hf", "quantize_config.json"))) for t in ("ours", "ref")}
    assert qcfg["ours"] == qcfg["ref"]

    def model_of(tag):  # load(format="huggingface") builds the model from the checkpoint's own config.json
        torch.manual_seed(0)
        m = LlamaForCausalLM(AutoConfig.from_pretrained(os.path.join(CKPT, f"{tag}_gptq_hf"))).float().eval()
        return _load_restated(states[tag], qcfg[tag]["bits"], qcfg[tag]["group_size"], m)

    model, packed = model_of("ref")
    assert len(packed) == 14
    assert _rel(_logits(model), np.load(os.path.join(CKPT, "ref_logits.npz"))["gptq_hf"]) <= 1e-5
    model, packed = model_of("ours")
    assert len(packed) == 14
    assert _rel(_logits(model), np.load(os.path.join(CKPT, "ours_logits.npz"))["gptq_hf"]) <= 2e-2
