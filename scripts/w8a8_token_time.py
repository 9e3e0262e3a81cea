"""Times of the dynamic per-token int8 activation cell of SmoothQuant W8A8 next to the static cell, on an MI355X.

  quantiser   inc_sq_quant_act_token against inc_sq_quant_act on the same input, M = 1 / 16 / 4096 at K = 5120 / 13824 (bf16), with the
              share of the HBM peak on the algorithmic bytes M*K*elt + M*Kp + 4*M;
  GEMM        inc_w8a8_gemm_rowscale against inc_w8a8_gemm on the bench's Llama-2-13B shapes and at M = 1; with --parent-lib also the
              static launch of another build of the library (loaded twice: the two copies against each other give the spread);
  module      W8A8Linear forward, per-token against static, M = 1 / 16 / 4096.

Every call is timed by its own pair of device events; the variants alternate inside one loop; the inputs of consecutive calls come from
a ring of buffers larger than the caches ("cold"): every call, whichever variant makes it, takes the next buffer of the ring, so no call
finds its operands in L2 / MALL and no variant inherits them from the one before.  The order of the variants rotates from pass to pass.
The figure is the median over the loop.
usage: python scripts/w8a8_token_time.py [--parent-lib other/libinc_mi355x.so] [--out profiles/w8a8_token/w8a8_token_time.log]
"""
import argparse
import ctypes
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_compressor_amd import _lib  # noqa: E402
from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s
COLD_BYTES = 768 << 20   # a ring at least this large: well past L2 (8 x 4 MiB) and the 256 MiB MALL
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def ring_len(nbytes):
    return max(2, -(-COLD_BYTES // max(nbytes, 1)))


def time_alternating(variants, n_ring, iters):
    """variants: {name: fn(i)} where i walks the ring -> {name: median microseconds}.  One warm-up pass over every variant first."""
    names = list(variants)
    call = 0
    for k in names:
        variants[k](call % n_ring)
        call += 1
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in variants}
    for it in range(iters):
        for j in range(len(names)):
            k = names[(it + j) % len(names)]
            a, b = ev[k][it]
            a.record()
            variants[k](call % n_ring)
            call += 1
            b.record()
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in ev[k]) * 1e3 for k in variants}


def load_other(path, tag):
    """A second, separate instance of a build of the library (dlopen of one path twice would return one handle)."""
    tmp = os.path.join(tempfile.mkdtemp(prefix="w8a8_token_time_"), f"libinc_{tag}.so")
    shutil.copy(path, tmp)
    lib = ctypes.CDLL(tmp)
    for name in ("inc_w8a8_gemm", "inc_w8a8_gemm_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def quantiser_section():
    say("== quantiser: inc_sq_quant_act_token against inc_sq_quant_act (bf16 input, cold, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    for K in (5120, 13824):
        for M in (1, 16, 4096):
            nbytes = M * K * 2 + M * K + 4 * M
            n = ring_len(M * K * 2) if M > 16 else 64
            xs = [torch.randn(M, K, device=dev, dtype=torch.bfloat16) for _ in range(n)]
            xq = torch.empty(M, K, dtype=torch.int8, device=dev)
            rs = torch.empty(M, dtype=torch.float32, device=dev)

            def token(i):
                _lib.check(_lib.lib.inc_sq_quant_act_token(xs[i].data_ptr(), _lib.INC_BF16, M, K, K, None, xq.data_ptr(), rs.data_ptr(), stream), "token")

            def static(i):
                _lib.check(_lib.lib.inc_sq_quant_act(xs[i].data_ptr(), _lib.INC_BF16, M, K, K, None, 0.05, 128.0, xq.data_ptr(), stream), "static")

            t = time_alternating({"token": token, "static": static}, n, 200 if M <= 16 else 60)
            bound = "HBM-bound" if M == 4096 else "latency-bound"
            say(f"M={M:5d} K={K:5d}: per-token {t['token']:8.1f} us ({nbytes / (t['token'] * 1e-6) / HBM_PEAK:6.3f} of HBM peak on {nbytes} B, {bound})   "
                f"static {t['static']:8.1f} us ({nbytes / (t['static'] * 1e-6) / HBM_PEAK:6.3f})   ratio {t['token'] / t['static']:.2f}")
            del xs


def gemm_section(parent):
    say()
    say("== GEMM: inc_w8a8_gemm_rowscale against inc_w8a8_gemm (bf16 output, no bias, cold weights, median us) ==")
    stream = torch.cuda.current_stream().cuda_stream
    others = {}
    if parent:
        others = {"other_a": load_other(parent, "a"), "other_b": load_other(parent, "b")}
        say(f"other build: {parent} (two separate copies: other_a / other_b)")
    for M in (4096, 1):
        for N, K in ((5120, 5120), (13824, 5120), (5120, 13824)):
            n = ring_len(N * K)
            ws_ = [torch.randint(-127, 128, (N, K), device=dev, dtype=torch.int8) for _ in range(n)]
            xq = torch.randint(-127, 128, (M, K), device=dev, dtype=torch.int8)
            alpha = torch.rand(N, device=dev) * 1e-4 + 1e-5
            corr = torch.randint(-1000, 1000, (N,), device=dev, dtype=torch.int32)
            rs = torch.rand(M, device=dev) * 1e-2 + 1e-3
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            need = _lib.lib.inc_w8a8_gemm_workspace_bytes(M, N, K)
            wsp = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

            def static_of(lib):
                def run(i):
                    rc = lib.inc_w8a8_gemm(xq.data_ptr(), ws_[i].data_ptr(), alpha.data_ptr(), corr.data_ptr(), None, y.data_ptr(), _lib.INC_BF16,
                                           M, N, K, wsp.data_ptr(), need, stream)
                    assert rc == 0, rc
                return run

            def rowscale(i):
                rc = _lib.lib.inc_w8a8_gemm_rowscale(xq.data_ptr(), ws_[i].data_ptr(), rs.data_ptr(), alpha.data_ptr(), None, y.data_ptr(),
                                                     _lib.INC_BF16, M, N, K, wsp.data_ptr(), need, stream)
                assert rc == 0, rc

            variants = {"static": static_of(_lib.lib), "rowscale": rowscale}
            variants.update({k: static_of(v) for k, v in others.items()})
            t = time_alternating(variants, n, 60 if M > 16 else 200)
            rate = f"{2.0 * M * N * K / (t['static'] * 1e-6) / 1e12:7.1f} Top/s" if M > 16 else f"{N * K / (t['static'] * 1e-6) / HBM_PEAK:6.3f} of HBM peak"
            msg = f"M={M:5d} N={N:5d} K={K:5d}: static {t['static']:8.1f} us ({rate})   row-scale {t['rowscale']:8.1f} us ({(t['rowscale'] / t['static'] - 1) * 100:+.1f} %)"
            if others:
                spread = (t["other_b"] / t["other_a"] - 1) * 100
                msg += f"   other_a {t['other_a']:8.1f} us, other_b {t['other_b']:8.1f} us (spread {spread:+.1f} %), static against other_a {(t['static'] / t['other_a'] - 1) * 100:+.1f} %"
            say(msg)
            del ws_


def module_section():
    say()
    say("== module: W8A8Linear forward (quantiser + GEMM, bf16, with input_scale, N=13824 K=5120, cold activations, median us) ==")
    N, K = 13824, 5120
    lin = torch.nn.Linear(K, N, bias=False).to(dev).to(torch.bfloat16)
    mods = {"static": W8A8Linear.from_float(lin, torch.full((K,), -4.0), torch.full((K,), 4.0), device=dev),
            "per_token": W8A8Linear.from_float(lin, device=dev, act_quant="per_token")}
    for m in mods.values():
        m.input_scale = torch.rand(K, device=dev) + 0.5
    for M in (1, 16, 4096):
        n = ring_len(M * K * 2) if M > 16 else 64
        xs = [torch.randn(M, K, device=dev, dtype=torch.bfloat16) for _ in range(n)]
        t = time_alternating({k: (lambda i, m=m: m(xs[i])) for k, m in mods.items()}, n, 60 if M > 16 else 200)
        say(f"M={M:5d}: static {t['static']:8.1f} us   per-token {t['per_token']:8.1f} us ({(t['per_token'] / t['static'] - 1) * 100:+.1f} %)")
        del xs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="another build of libinc_mi355x.so whose static inc_w8a8_gemm is timed alongside")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w8a8_token", "w8a8_token_time.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    say(f"device: {torch.cuda.get_device_name(0)}; HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s")
    quantiser_section()
    gemm_section(a.parent_lib)
    module_section()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
