"""SHA-256 of the outputs of every kernel on the 256 x 256 wave frame (csrc/tile256_frame.hpp), one line per case: run it in two trees
and diff the listings to see whether a change of the kernels moved a bit.  The cases and their seeded inputs are the tests' own tables,
in bf16 and fp16:

  woq            the BIG / 3A2B_W4 / 3A2B_W8 / D2R rows of tests/gemm_route_cases.py (ops.woq_gemm)
  w8a8 static    every case of tests/w8a8_route_cases.py through inc_w8a8_gemm with corr and bias, with the workspace the plan asks for
                 (the K-split tail and its finish kernel) and without one (one pass); y aligned as the case says
  w8a8 rowscale  the same through inc_w8a8_gemm_rowscale with row scales and bias
  mx             every GCASES x PAIRS of tests/mx_cases.py on random_operands with a bias (inc_mx_gemm)

Every case is called twice; the two outputs must agree before the digest is printed.
usage: python scripts/tile256_outputs_digest.py > listing.txt"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd import _lib, ops  # noqa: E402
from tests import gemm_route_cases as R  # noqa: E402
from tests import mx_cases as X  # noqa: E402
from tests import w8a8_route_cases as W  # noqa: E402
from tests import w8a8_token_cases as T  # noqa: E402

dev = torch.device("cuda:0")
DTYPES = ((torch.bfloat16, "bf16", _lib.INC_BF16), (torch.float16, "fp16", _lib.INC_F16))
SENTINEL = 0x7B5A


def emit(name, fn):
    outs = [fn(), fn()]
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), f"{name}: a second call is not bit-identical"
    print(f"{name} {hashlib.sha256(outs[0].contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()}", flush=True)


def window(M, N, lead):
    """y [M * N] int16 inside a sentinel-filled buffer, `lead` elements past a 16-byte boundary, and the check of its surroundings."""
    buf = torch.full((16 + lead + M * N + 16,), SENTINEL, dtype=torch.int16, device=dev)
    y = buf[16 + lead:16 + lead + M * N]

    def intact():
        return bool((buf[:16 + lead] == SENTINEL).all()) and bool((buf[16 + lead + M * N:] == SENTINEL).all())
    return y, intact


def w8a8(c, d, code, dtype, rows, use_ws):
    need = _lib.lib.inc_w8a8_gemm_workspace_bytes(c.M, c.N, c.K)
    ws = torch.full((max(need, 16),), 0x7F, dtype=torch.uint8, device=dev)
    y, intact = window(c.M, c.N, W.misalign(c.y_align) // 2)
    bias = None if d["bias"] is None else d["bias"].to(dtype)
    bp = None if bias is None else bias.data_ptr()
    wp, wb = (ws.data_ptr(), need) if use_ws else (None, 0)
    s = torch.cuda.current_stream().cuda_stream
    if rows:
        rc = _lib.lib.inc_w8a8_gemm_rowscale(d["xq"].data_ptr(), d["wq"].data_ptr(), d["rs"].data_ptr(), d["alpha"].data_ptr(), bp, y.data_ptr(),
                                             code, c.M, c.N, c.K, wp, wb, s)
    else:
        rc = _lib.lib.inc_w8a8_gemm(d["xq"].data_ptr(), d["wq"].data_ptr(), d["alpha"].data_ptr(),
                                    None if d["corr"] is None else d["corr"].data_ptr(), bp, y.data_ptr(), code, c.M, c.N, c.K, wp, wb, s)
    torch.cuda.synchronize()
    assert rc == 0 and intact(), (c.name, rc)
    return y.clone()


def mx(c, d, pair, bias, code):
    afmt, wfmt = pair
    y, intact = window(c.M, c.N, 1 if c.y_misaligned else 0)
    rc = _lib.lib.inc_mx_gemm(d["xq"].data_ptr(), d["xs"].data_ptr(), afmt, d["wq"].data_ptr(), d["ws"].data_ptr(), wfmt, bias.data_ptr(),
                              y.data_ptr(), code, c.M, c.N, c.Kp, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and intact(), (c.name, rc)
    return y.clone()


def main():
    for c in R.CASES:
        if c.route in ("BIG", "3A2B_W4", "3A2B_W8", "D2R"):
            L = R.make_layer(c.N, c.K, c.group_size, c.bits)
            qw, sc, qz = (torch.from_numpy(L[k]).to(dev) for k in ("qweight", "scales", "qzeros"))
            for dtype, dn, _ in DTYPES:
                x, bias = R.make_x(c.M, c.K, dtype).to(dev), R.make_bias(c.N, dtype).to(dev)
                emit(f"woq {c.name} {dn}", lambda: ops.woq_gemm(x, qw, sc, qz, bias, c.N, c.K, c.group_size, c.bits))
    for c in W.CASES:
        d = {k: (None if v is None else v.to(dev)) for k, v in W.make_inputs(c).items()}
        d["rs"] = T.gemm_row_scale(c.M).to(dev)
        for dtype, dn, code in DTYPES:
            for rows in (False, True):
                for use_ws in (True, False):
                    emit(f"w8a8 {'rowscale' if rows else 'static'} {'ws' if use_ws else 'no_ws'} {c.name} {dn}",
                         lambda: w8a8(c, d, code, dtype, rows, use_ws))
    for c in X.GCASES:
        for pair, pid in zip(X.PAIRS, X.PAIR_IDS):
            r = X.random_operands(c.M, c.N, c.Kp, pair[0], pair[1], seed=5)
            d = dict(xq=X.stored(r["xq"], pair[0]).to(dev), xs=r["xs"].to(dev), wq=X.stored(r["wq"], pair[1]).to(dev), ws=r["ws"].to(dev))
            for dtype, dn, code in DTYPES:
                bias = (torch.randn(c.N, generator=torch.Generator().manual_seed(9)) * 0.5).to(dtype).to(dev)
                emit(f"mx {pid} {c.name} {dn}", lambda: mx(c, d, pair, bias, code))


if __name__ == "__main__":
    with torch.no_grad():
        main()
