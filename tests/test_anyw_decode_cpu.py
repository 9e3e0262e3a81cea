"""CPU: the decode GEMV of the 1 / 2 / 3 / 5 / 6 / 7-bit modules (inc_woq_gemv_anyw) -- everything that needs no GPU.

  pins      the edges every case of tests/anyw_decode_cases.py is written for are still in its layer;
  contract  an fp32 torch emulation of the kernel's arithmetic (rn16(int8(q - z) * scale) decoded from the packed words, exact products,
            fp32 sums per K-slice) meets the element-wise bound of tests/gemm_route_cases.py on every case and dtype, and reproduces
            the oracle's weight bit for bit on one-hot rows;
  C-ABI     header, library and ctypes table agree on the three new symbols, the ABI version stays 12;
  host      inc_woq_gemv_anyw_slices / _workspace_bytes and the entry point's refusals are pure host code;
  ops       ops.woq_gemv_anyw raises ValueError before anything touches a device.
"""

import ctypes
import os
import re

import pytest
import torch

from tests import anyw_decode_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("inc_woq_gemv_anyw", "inc_woq_gemv_anyw_workspace_bytes", "inc_woq_gemv_anyw_slices")
INC_ERR_BAD_ARG, INC_ERR_UNSUPPORTED, INC_ERR_WORKSPACE = -1, -2, -4


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.CASES, ids=A.CASE_IDS)
def test_case_pins_are_in_the_layer(c):
    assert A.pins_of(c) == c.pins
    assert A.has_zero_zp(c), "no zp = 0 entry (the stored all-ones field that wraps)"
    assert 1 <= c.M <= A.MAX_M and c.K % 32 == 0 and c.N % 4 == 0 and c.N >= 64
    assert c.name.endswith(("_long", "_long_m16")) == c.pins.splits


def test_table_covers_every_width_and_edge():
    assert {c.bits for c in A.CASES} == set(A.BITS)
    assert {c.M for c in A.CASES} >= {1, 16}
    for bits in A.BITS:
        mine = [c for c in A.CASES if c.bits == bits]
        assert any(c.pins.splits for c in mine) and any(not c.pins.splits for c in mine), bits
    for bits in (3, 5, 6):  # n_pack = 10 / 6 / 5: words straddle groups, quads straddle qzeros words, the last word is padded
        mine = [c for c in A.CASES if c.bits == bits]
        assert any(c.pins.straddle_words for c in mine) and any(c.pins.straddle_quads for c in mine) and any(c.pins.padding for c in mine), bits
    assert any(c.pins.ragged_group and not c.pins.splits for c in A.CASES)
    # a split whose last slice is shorter than the others
    assert all(c.K % A.SLICE_K[c.bits] != 0 for c in A.CASES if c.pins.splits)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the contract, emulated
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", A.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", A.CASES, ids=A.CASE_IDS)
def test_emulated_contract_meets_the_bound(c, dtype):
    L = A.layer_of(c)
    w64 = A.dense_weight64(L, dtype)
    assert torch.equal(A.emulated_weight(c, dtype).double(), w64), "decoding the packed words by the layout rules is not the oracle's weight"
    x, bias = A.make_x(c.M, c.K, dtype), A.make_bias(c.N, dtype)
    for b in (bias, None):
        ref, S = A.reference(x, w64, b if b is not None else torch.zeros(c.N, dtype=dtype))
        A.assert_elementwise(A.emulate(c, x, b, dtype), ref, S, c.K, dtype, f"{c.name} emulated")


@pytest.mark.parametrize("dtype", A.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", A.CASES, ids=A.CASE_IDS)
def test_one_hot_rows_return_the_oracle_weight(c, dtype):
    w = A.dense_weight64(A.layer_of(c), dtype).to(dtype)
    x, ks = A.one_hot(c, dtype)
    assert len(ks) <= A.MAX_M
    y = A.emulate(c, x, None, dtype)
    for i, k in enumerate(ks):
        assert torch.equal(y[i], w[:, k]), (c.name, k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_bindings():
    from neural_compressor_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inc_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(inc_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/inc_mi355x.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert len(_lib.SIGNATURES["inc_woq_gemv_anyw"][1]) == 16
    assert _lib.SIGNATURES["inc_woq_gemv_anyw_slices"][1] == _lib.SIGNATURES["inc_woq_gemv_anyw_workspace_bytes"][1]
    assert _lib.lib.inc_abi_version() == 12 == _lib.ABI_VERSION


@pytest.mark.parametrize("c", A.CASES, ids=A.CASE_IDS)
def test_slices_and_workspace_are_host_code(c):
    from neural_compressor_amd import _lib

    L = _lib.lib
    s = L.inc_woq_gemv_anyw_slices(c.M, c.N, c.K, c.bits)
    assert s == A.slices_of(c)
    assert (s >= 2) if c.pins.splits else (s == 1)
    assert L.inc_woq_gemv_anyw_workspace_bytes(c.M, c.N, c.K, c.bits) == (16384 + s * c.M * c.N * 4 if s > 1 else 0)


def test_entry_point_refuses_on_the_host():
    """Every refusal comes before the launch, so it shows without a GPU (the pointers are never dereferenced)."""
    from neural_compressor_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(M=1, N=64, K=64, G=2, gs=32, bits=3, dt=_lib.INC_BF16, x=p, y=p, qw=p, ws=None, wsb=0):
        return L.inc_woq_gemv_anyw(x, dt, qw, p, p, None, y, M, N, K, G, gs, bits, ws, wsb, None)

    for bits in (4, 8, 0, 9):
        assert call(bits=bits) == INC_ERR_UNSUPPORTED
        assert L.inc_woq_gemv_anyw_slices(1, 64, 64, bits) == 0 and L.inc_woq_gemv_anyw_workspace_bytes(1, 64, 64, bits) == 0
    assert call(dt=_lib.INC_F32) == INC_ERR_UNSUPPORTED
    assert call(M=0) == INC_ERR_UNSUPPORTED and call(M=17) == INC_ERR_UNSUPPORTED
    assert call(K=48, G=2) == INC_ERR_UNSUPPORTED            # K % 32
    assert call(N=66) == INC_ERR_UNSUPPORTED and call(N=60) == INC_ERR_UNSUPPORTED
    assert call(K=96, gs=48, G=2) == INC_ERR_UNSUPPORTED     # not a power of two
    assert call(gs=16, G=4) == INC_ERR_UNSUPPORTED           # below 32
    assert call(x=p + 8) == INC_ERR_UNSUPPORTED and call(y=p + 2) == INC_ERR_UNSUPPORTED and call(qw=p + 4) == INC_ERR_UNSUPPORTED
    assert call(G=3) == INC_ERR_BAD_ARG                      # G must be ceil(K / group_size)
    assert call(x=None) == INC_ERR_BAD_ARG
    # a split without its workspace
    assert L.inc_woq_gemv_anyw_slices(1, 64, 2080, 3) == 4
    need = L.inc_woq_gemv_anyw_workspace_bytes(1, 64, 2080, 3)
    assert call(K=2080, gs=128, G=17) == INC_ERR_WORKSPACE
    assert call(K=2080, gs=128, G=17, ws=p, wsb=need - 1) == INC_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------------------------------------------
# ops.woq_gemv_anyw: ValueError before any launch
# ---------------------------------------------------------------------------------------------------------------------------------------
def _module_tensors(N, K, gs, bits, device="cpu"):
    npk, G = 32 // bits, -(-K // gs)
    return (torch.zeros(-(-K // npk), N, dtype=torch.int32, device=device), torch.zeros(G, N, dtype=torch.float16, device=device),
            torch.zeros(G, -(-N // npk), dtype=torch.int32, device=device))


@pytest.mark.parametrize("what,M,N,K,gs,bits,dtype,match", [
    ("bits4", 1, 64, 64, 32, 4, torch.bfloat16, "bits=4"),
    ("bits8", 1, 64, 64, 32, 8, torch.bfloat16, "bits=8"),
    ("m0", 0, 64, 64, 32, 3, torch.bfloat16, "M=0"),
    ("m17", 17, 64, 64, 32, 3, torch.bfloat16, "M=17"),
    ("k48", 1, 64, 48, 16, 3, torch.bfloat16, "K=48"),
    ("n66", 1, 66, 64, 32, 3, torch.bfloat16, "N=66"),
    ("group48", 1, 64, 96, 48, 3, torch.bfloat16, "group_size=48"),
    ("fp32", 1, 64, 64, 32, 3, torch.float32, "bf16 or fp16"),
    ("cpu", 1, 64, 64, 32, 3, torch.bfloat16, "is on cpu"),
])
def test_ops_wrapper_raises_before_any_launch(monkeypatch, what, M, N, K, gs, bits, dtype, match):
    from neural_compressor_amd import _lib, ops

    def no_launch(*a):
        raise AssertionError("inc_woq_gemv_anyw was called")

    monkeypatch.setattr(_lib.lib, "inc_woq_gemv_anyw", no_launch, raising=False)
    qw, sc, qz = _module_tensors(N, K, gs, bits)
    x = torch.zeros(M, K, dtype=dtype)
    with pytest.raises(ValueError, match=match):
        ops.woq_gemv_anyw(x, qw, sc, qz, None, N, K, gs, bits)


def test_eligibility_rule_matches_the_entry_point():
    """ops.gemv_anyw_takes (what the module records with its plan) says yes exactly where inc_woq_gemv_anyw_slices plans a launch."""
    from neural_compressor_amd import _lib, ops

    for bits in range(1, 9):
        for N in (60, 64, 66, 68, 21):
            for K, gs in ((64, 32), (150, 32), (96, 48), (160, 64), (64, -1), (64, 16), (64, 128)):
                gs_eff = K if gs == -1 or gs >= K else gs
                groups_ok = gs_eff == K or (gs_eff >= 32 and gs_eff & (gs_eff - 1) == 0)
                assert ops.gemv_anyw_takes(N, K, gs, bits) == (_lib.lib.inc_woq_gemv_anyw_slices(1, N, K, bits) > 0 and groups_ok), (bits, N, K, gs)
