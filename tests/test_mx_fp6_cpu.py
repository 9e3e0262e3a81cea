"""No GPU: the MXFP6 pairs in the config and module tables, the fp6 entry point in the C ABI and what it and the products reject
before any HIP call, and the fp6 packing of tests/mx_fp6_cases.py."""

import pytest
import torch

from tests import mx_cases as C
from tests import mx_fp6_cases as F


def test_pairs_construct_and_the_rest_raises():
    from neural_compressor_amd.torch.algorithms.mx_quant import mx_quant
    from neural_compressor_amd.torch.quantization import MXQuantConfig

    for a, w in F.PAIRS:
        cfg = MXQuantConfig(w_dtype=F.FMT_NAMES[w], act_dtype=F.FMT_NAMES[a])
        assert (cfg.w_dtype, cfg.act_dtype) == (F.FMT_NAMES[w], F.FMT_NAMES[a])
        assert (F.FMT_NAMES[w], F.FMT_NAMES[a]) in mx_quant.MXLinear.FP6_PAIRS and mx_quant.FORMATS[F.FMT_NAMES[w]] == w
    for kw in (dict(w_dtype="fp6_e2m3", act_dtype="fp4"), dict(w_dtype="fp6_e3m2", act_dtype="fp6_e2m3"),
               dict(w_dtype="fp6_e2m3", act_dtype="fp6_e3m2"), dict(w_dtype="fp6_e2m3", act_dtype="fp6_e2m3", weight_only=True),
               dict(w_dtype="fp6_e2m3", act_dtype="bf16", weight_only=True)):
        with pytest.raises(NotImplementedError, match="MXQuant on MI355X"):
            MXQuantConfig(**kw)
    # the experts and weight-only classes keep their tables: no fp6
    assert not any("fp6" in d for p in mx_quant.PAIRS + mx_quant.WEIGHT_ONLY_PAIRS for d in p) and mx_quant.MXWeightOnlyLinear.FP6_PAIRS == ()


def test_fp6_entry_point_is_declared_bound_and_rejects_bad_arguments():
    import os

    from neural_compressor_amd import _lib, ops

    lib = _lib.lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "inc_mi355x.h")).read()
    assert "int inc_mx_quant_fp6(" in header and "inc_mx_quant_fp6" in _lib.SIGNATURES and callable(lib.inc_mx_quant_fp6)
    assert (ops.MX_FP6_E2M3, ops.MX_FP6_E3M2) == (F.E2M3, F.E3M2) == (2, 3)
    assert "#define INC_MX_FP6_E2M3 2" in header and "#define INC_MX_FP6_E3M2 3" in header
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr()
    assert p % 16 == 0
    q = lib.inc_mx_quant_fp6
    assert q(None, _lib.INC_F32, 1, 32, 128, F.E2M3, p, p, None) == -1
    assert q(p, _lib.INC_F32, 1, 32, 128, F.E2M3, None, p, None) == -1
    assert q(p, _lib.INC_F32, 1, 32, 128, F.E3M2, p, None, None) == -1
    assert q(p, _lib.INC_F32, 1, 32, 128, F.E3M2, p + 8, p, None) == -1          # codes not 16-byte aligned
    for fmt in (C.FP8, C.FP4, 1):
        assert q(p, _lib.INC_F32, 1, 32, 128, fmt, p, p, None) == -2
    assert q(p, 7, 1, 32, 128, F.E2M3, p, p, None) == -2
    assert q(p, _lib.INC_F32, 1, 32, 96, F.E2M3, p, p, None) == -2               # Kp not a tile multiple
    for entry in (lib.inc_mx_gemm, lib.inc_mx_gemv):
        for xf, wf in ((F.E2M3, C.FP8), (F.E2M3, F.E3M2), (F.E3M2, F.E2M3), (C.FP4, F.E2M3), (F.E3M2, C.FP4), (C.FP8, F.E3M2)):
            assert entry(p, p, xf, p, p, wf, None, p, _lib.INC_BF16, 1, 1, 128, None) == -2, (xf, wf)


@pytest.mark.parametrize("fmt", [F.E2M3, F.E3M2], ids=["e2m3", "e3m2"])
def test_pack_round_trip_and_value_codes(fmt):
    c = torch.arange(64, dtype=torch.uint8).repeat(3, 2)
    c[1] = c[1].flip(0)
    packed = F.pack_fp6(c)
    assert packed.shape == (3, 96) and torch.equal(F.unpack_fp6(packed), c)
    assert packed[0, :3].tolist() == [0 | (1 << 6) & 0xFF, (1 >> 2) | (2 << 4) & 0xFF, (2 >> 4) | (3 << 2)]
    v = torch.arange(-3, 4)[None, :]
    assert torch.equal(C.code_table(fmt)[C.encode_values(v, fmt).long()], v.double())
    assert float(C.code_table(fmt).max()) == C._F[fmt]["sat"]
