"""SHA-256 of what the four fused experts modules and the two linear groups give, one line per case: run it in two trees and diff the
listings to see whether a change of the Python side (fused_experts.py, the modules, ops.py's routed wrappers, save_load) moved a bit.
The modules are built by the GPU tests' own small builders:

  int4      tests/test_gpu_moe_experts._experts(E 8, H 256, I 512, group 32, asym)            MI355XWeightOnlyExperts
  fp8       tests/test_gpu_fp8_moe._fp8_experts(E 6, H 200, I 72: both K paddings)            FP8Experts
  mx        tests/test_gpu_mx_moe._mx_experts, the same sizes x the three format pairs        MXExperts
  gpt_oss   tests/test_gpu_mx_gpt_oss._mx_experts, the same sizes x the three pairs           MXGptOssExperts

x input dtype bf16 / fp16 / fp32 x (T, k) in (1, 2), (37, 2), (5, 1) with the -1 / E sentinel ids of the tests' `_inputs` x route (fused,
dense).  A line hashes the forward output, recover() (and recover_biases()), the sorted state-dict keys with shapes and dtypes and, for
MX and FP8, the qconfig_of JSON text of a model that holds the module.  `mx_group` / `fp8_group` lines: mx_linear_group / fp8_linear_group
of three members at M = 1 and M = 17.

Every call is made twice; the two results must agree before they enter the digest (a line that does not repeat says so instead).
usage: python scripts/experts_outputs_digest.py > listing.txt"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd.torch.algorithms.fp8_quant import FP8Linear  # noqa: E402
from neural_compressor_amd.torch.algorithms.fp8_quant import save_load as fp8_save_load  # noqa: E402
from neural_compressor_amd.torch.algorithms.fp8_quant.fp8_quant import fp8_linear_group  # noqa: E402
from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear  # noqa: E402
from neural_compressor_amd.torch.algorithms.mx_quant import save_load as mx_save_load  # noqa: E402
from neural_compressor_amd.torch.algorithms.mx_quant.mx_quant import mx_linear_group  # noqa: E402
from tests import mx_cases as C  # noqa: E402
from tests import test_gpu_fp8_moe as TF  # noqa: E402
from tests import test_gpu_moe_experts as TI  # noqa: E402
from tests import test_gpu_mx_gpt_oss as TG  # noqa: E402
from tests import test_gpu_mx_moe as TM  # noqa: E402

dev = torch.device("cuda:0")
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
TKS = ((1, 2), (37, 2), (5, 1))
GROUP_NS = (33, 17, 260)
GROUP_K = 200


def raw(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def emit(name, fn, *texts):
    """One line: the tensors of fn() (called twice) and the given texts."""
    outs = [fn(), fn()]
    torch.cuda.synchronize()
    if not all(a.dtype == b.dtype and a.shape == b.shape and raw(a) == raw(b) for a, b in zip(*outs)):
        print(f"{name} NOT-REPEATABLE", flush=True)
        return
    h = hashlib.sha256()
    for o in outs[0]:
        h.update(f"{o.dtype} {tuple(o.shape)}".encode())
        h.update(raw(o))
    for t in texts:
        h.update(t.encode())
    print(f"{name} {h.hexdigest()}", flush=True)


def holder(m):
    model = torch.nn.Module()
    model.experts = m
    return model


def experts_lines(name, m, qconfig_of=None):
    E, H = m.num_experts, m.hidden_dim
    keys = json.dumps(sorted((k, list(v.shape), str(v.dtype)) for k, v in m.state_dict().items()))
    cfg = "" if qconfig_of is None else json.dumps(qconfig_of(holder(m)), indent=2)
    extra = m.recover_biases if hasattr(m, "recover_biases") else lambda: ()
    for dtype in DTYPES:
        for T, k in TKS:
            x, idx, w = TM._inputs(dev, T, k, E, H, dtype, seed=T)
            for fused in (True, False):
                def fn():
                    m.MOE_FUSED = fused
                    return [m(x, idx, w), *m.recover(), *extra()]

                emit(f"{name} {str(dtype)[6:]} T{T} k{k} {'fused' if fused else 'dense'}", fn, keys, cfg, m.extra_repr())
    m.MOE_FUSED = True


def group_lines(name, cls, group, from_float):
    g = torch.Generator().manual_seed(31)
    lins = []
    for i, N in enumerate(GROUP_NS):
        lin = torch.nn.Linear(GROUP_K, N, bias=i != 1).to(torch.bfloat16)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(N, GROUP_K, generator=g) * 0.08)
            if lin.bias is not None:
                lin.bias.copy_(torch.randn(N, generator=g) * 0.5)
        lins.append(lin)
    mods = [from_float(lin) for lin in lins]
    assert all(isinstance(m, cls) for m in mods)
    for dtype in DTYPES:
        for M in (1, 17):
            x = (torch.randn(M, GROUP_K, generator=g) * 1.5).to(dtype).to(dev)
            emit(f"{name} {str(dtype)[6:]} m{M}", lambda: group(x, mods))


if __name__ == "__main__":
    with torch.no_grad():
        experts_lines("int4", TI._experts(dev, 8, 256, 512, 32, asym=True, seed=4))
        experts_lines("fp8", TF._fp8_experts(dev)[1], fp8_save_load.qconfig_of)
        for pair, pid in zip(C.PAIRS, C.PAIR_IDS):
            experts_lines(f"mx {pid}", TM._mx_experts(dev, pair)[1], mx_save_load.qconfig_of)
        for pair, pid in zip(C.PAIRS, C.PAIR_IDS):
            experts_lines(f"gpt_oss {pid}", TG._mx_experts(dev, pair)[1], mx_save_load.qconfig_of)
        group_lines("fp8_group", FP8Linear, fp8_linear_group, lambda lin: FP8Linear.from_float(lin, device=dev))
        for pair, pid in zip(C.PAIRS, C.PAIR_IDS):
            afmt, wfmt = pair
            group_lines(f"mx_group {pid}", MXLinear, mx_linear_group,
                        lambda lin: MXLinear.from_float(lin, w_dtype=C.FMT_NAMES[wfmt], act_dtype=C.FMT_NAMES[afmt], device=dev))
