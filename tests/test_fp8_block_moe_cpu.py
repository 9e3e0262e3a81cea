"""CPU: inc_fp8_block_moe_gemm is bound and rejects what it does not take before any HIP call; FP8BlockExperts needs a HIP device."""

import pytest

ONE = 4096  # any non-NULL, 16-byte aligned address: rejected calls never touch it
OK = dict(mode=2, aq=ONE, as_=ONE, route=ONE, wq=ONE, ws=ONE, rw=None, wdt=0, out=ONE, odt=0, T=4, k=2, E=4, N=16, Kp=128)
BAD = [dict(aq=None), dict(as_=None), dict(route=None), dict(wq=None), dict(ws=None), dict(out=None), dict(T=0), dict(k=0), dict(E=0),
       dict(N=0), dict(Kp=0), dict(mode=3), dict(mode=-1), dict(mode=1), dict(aq=ONE + 8), dict(wq=ONE + 4), dict(as_=ONE + 2),
       dict(ws=ONE + 1)]
UNSUPPORTED = [dict(Kp=192), dict(E=513), dict(T=2 ** 21 + 1), dict(mode=0, N=15, odt=2), dict(mode=0), dict(odt=2), dict(odt=77),
               dict(mode=1, rw=ONE, odt=1), dict(mode=1, rw=ONE, wdt=7)]


@pytest.mark.parametrize("kw,rc", [(kw, -1) for kw in BAD] + [(kw, -2) for kw in UNSUPPORTED], ids=str)
def test_entry_point_validates_before_any_hip_call(kw, rc):
    from neural_compressor_amd import _lib
    assert _lib.SIGNATURES["inc_fp8_block_moe_gemm"] == _lib.SIGNATURES["inc_fp8_moe_gemm"] and _lib.lib.inc_abi_version() == 12
    a = dict(OK, **kw)
    assert _lib.lib.inc_fp8_block_moe_gemm(a["mode"], a["aq"], a["as_"], a["route"], a["wq"], a["ws"], a["rw"], a["wdt"], a["out"], a["odt"],
                                           a["T"], a["k"], a["E"], a["N"], a["Kp"], None) == rc


def test_module_needs_a_hip_device():
    from neural_compressor_amd.torch.algorithms.fp8_quant import FP8BlockExperts
    with pytest.raises(RuntimeError, match="HIP device"):
        FP8BlockExperts(2, 8, 8, device="cpu")
