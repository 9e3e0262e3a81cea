"""CPU: argument validation of inc_woq_gemm_lut / inc_woq_gemm_lut_workspace_bytes (K4d) -- every rejection happens before any HIP
call, so it is testable without a GPU.  No call here is eligible: nothing is ever launched."""

import ctypes

import pytest

BF16, F16, F32 = 2, 1, 0
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4


@pytest.fixture(scope="module")
def L():
    from neural_compressor_amd import _lib

    return _lib.lib


TABLE = (ctypes.c_float * 16)(*range(16))
FAKE = 1 << 20  # a 16-byte aligned address that is never dereferenced: every call below returns before touching memory


def _call(L, x=FAKE, xdtype=BF16, qweight=FAKE, row_bytes=2048, table=TABLE, scales=FAKE, sdt=F32, rnd=0, qzeros=None, zrow_bytes=0,
          y=FAKE, M=1, N=4096, K=4096, G=128, gs=32, ws=None, ws_bytes=0):
    return L.inc_woq_gemm_lut(x, xdtype, qweight, row_bytes, table, scales, sdt, rnd, qzeros, zrow_bytes, None, y, M, N, K, G, gs, ws,
                              ws_bytes, None)


def test_null_pointers_and_sizes(L):
    assert _call(L, x=None) == BAD_ARG
    assert _call(L, qweight=None) == BAD_ARG
    assert _call(L, table=None) == BAD_ARG
    assert _call(L, scales=None) == BAD_ARG
    assert _call(L, y=None) == BAD_ARG
    assert _call(L, M=0) == BAD_ARG and _call(L, N=-1) == BAD_ARG and _call(L, K=0) == BAD_ARG
    assert _call(L, gs=0) == BAD_ARG
    assert _call(L, G=127) == BAD_ARG  # G must be ceil(K / group_size)
    assert _call(L, qzeros=FAKE, zrow_bytes=0) == BAD_ARG
    assert _call(L, qzeros=FAKE, zrow_bytes=32) == BAD_ARG  # 64 nibbles for 128 groups


def test_ineligible_requests_are_unsupported(L):
    assert _call(L, xdtype=F32) == UNSUPPORTED
    assert _call(L, sdt=7) == UNSUPPORTED
    assert _call(L, K=4080, G=255, gs=16, row_bytes=2048) == UNSUPPORTED  # K % 32 != 0
    assert _call(L, G=86, gs=48) == UNSUPPORTED                            # a 32-k step would straddle two groups
    assert _call(L, row_bytes=2032) == UNSUPPORTED                         # shorter than K / 2
    assert _call(L, row_bytes=2056) == UNSUPPORTED                         # rows not 16-byte aligned
    assert _call(L, x=FAKE + 2) == UNSUPPORTED and _call(L, qweight=FAKE + 8) == UNSUPPORTED


def test_workspace_contract(L):
    W = L.inc_woq_gemm_lut_workspace_bytes
    assert W(1, 4096, 4096) > 16 << 10          # decode: split-K partials behind the 16 KiB of counters
    assert W(4096, 4096, 4096) == 0             # enough (M tile, column strip) pairs: no split
    assert W(1, 256, 512) == 0                  # one super-step of K: nothing to split
    assert W(0, 4096, 4096) == 0 and W(1, 0, 1) == 0
    assert _call(L, ws=None, ws_bytes=0) == WORKSPACE
    assert _call(L, ws=FAKE, ws_bytes=W(1, 4096, 4096) - 4) == WORKSPACE
