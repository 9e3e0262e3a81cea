"""Plain helpers of the GPTQ-on-MX tests: a torch restatement of the column loop of inc_gptq_quantize_layer_mx (runnable in fp32, where
every operation is the kernel's own elementwise fp32 op in the kernel's order, or in fp64), the round-to-nearest restatement that is
inc_mx_quant's specification, the packed layouts, and the inputs."""

import functools
import math

import torch

FMT = {"fp4": dict(code=4, EMAX=2, MB=1, EMINF=127, SAT=6.0, sign=3), "fp8_e4m3": dict(code=0, EMAX=8, MB=3, EMINF=121, SAT=448.0, sign=7)}


def _expfield(a):
    """The fp32 exponent field of a >= 0 (0 for zero and for what fp32 holds as a subnormal), in a's own precision."""
    _, ex = torch.frexp(a)
    return torch.where(a > 0, (ex + 126).clamp(min=0), torch.zeros_like(ex)).to(torch.int64)


def mx_bytes(blocks, fmt):
    """E8M0 byte of every block: blocks [..., 32] -> [...]."""
    return (_expfield(blocks.abs().amax(-1)) - FMT[fmt]["EMAX"]).clamp(0, 254)


def mx_encode(v, sign, fmt):
    """mx_encode of csrc/mx_format.hpp: RNE of the scaled value onto the element grid, saturating, `sign` in the sign bit."""
    f = FMT[fmt]
    a = v.abs().clamp(max=f["SAT"])
    e = _expfield(a).clamp(min=f["EMINF"])
    t = torch.round(torch.ldexp(a, 127 + f["MB"] - e)).to(torch.int64)
    return ((e - f["EMINF"]) << f["MB"]) + t + (sign.to(torch.int64) << f["sign"])


def mx_value(code, fmt, dtype):
    """The signed value of a code (the sign bit gives -0.0 for a zero magnitude, as the modules' table does)."""
    f = FMT[fmt]
    mag = code & ((1 << f["sign"]) - 1)
    field, frac = mag >> f["MB"], mag & ((1 << f["MB"]) - 1)
    mant = torch.where(field > 0, frac + (1 << f["MB"]), frac).to(dtype)
    val = torch.ldexp(mant, torch.where(field > 0, field - 1, field) + f["EMINF"] - f["MB"] - 127)
    return torch.where((code >> f["sign"]) > 0, -val, val)


def gptq_mx_loop(W, Hinv, fmt, dtype):
    """-> codes [N,K] int64, bytes [N,K/32] int64, Q [N,K] and Err1 of the first 128 columns [N,128], computed in `dtype`."""
    W, Hinv = W.to(dtype).clone(), Hinv.to(dtype)
    N, K = W.shape
    one = torch.ones((), dtype=dtype)
    codes, bytes_ = torch.zeros(N, K, dtype=torch.int64), torch.zeros(N, K // 32, dtype=torch.int64)
    Q, first_err = torch.zeros_like(W), None
    for i1 in range(0, K, 128):
        i2 = min(i1 + 128, K)
        cnt = i2 - i1
        W1, H1, Err = W[:, i1:i2].clone(), Hinv[i1:i2, i1:i2], torch.zeros(N, 128, dtype=dtype)
        b = mx_bytes(W1.view(N, cnt // 32, 32), fmt)  # on the columns as they are when the 128 columns start
        bytes_[:, i1 // 32:i2 // 32] = b
        mult, sc = torch.ldexp(one, 127 - b), torch.ldexp(one, b - 127)
        for i in range(cnt):
            x = W1[:, i]
            code = mx_encode(x * mult[:, i // 32], torch.signbit(x), fmt)
            q = mx_value(code, fmt, dtype) * sc[:, i // 32]
            e = (x - q) / H1[i, i]
            W1[:, i:] = W1[:, i:] - e[:, None] * H1[i, i:][None]
            codes[:, i1 + i], Q[:, i1 + i], Err[:, i] = code, q + 0.0, e  # (a zero q is stored as +0)
        W[:, i2:] = W[:, i2:] - Err[:, :cnt] @ Hinv[i1:i2, i2:]
        first_err = Err if first_err is None else first_err
    return codes, bytes_, Q, first_err


def rtn_mx(W, fmt):
    """inc_mx_quant's specification on a weight: -> Q [N,K] fp32."""
    N, K = W.shape
    blocks = W.float().view(N, K // 32, 32)
    b = mx_bytes(blocks, fmt)[..., None]
    one = torch.ones((), dtype=torch.float32)
    code = mx_encode(blocks * torch.ldexp(one, 127 - b), torch.signbit(blocks), fmt)
    return (mx_value(code, fmt, torch.float32) * torch.ldexp(one, b - 127)).view(N, K)


def pack(codes, bytes_, fmt):
    """The storage of inc_mx_quant for Kp = K rounded up to 128: (qweight, w_scale) uint8, the padding zero."""
    N, K = codes.shape
    Kp = -(-K // 128) * 128
    c = torch.zeros(N, Kp, dtype=torch.int64)
    c[:, :K] = codes
    s = torch.zeros(N, Kp // 32, dtype=torch.int64)
    s[:, : K // 32] = bytes_
    if fmt == "fp4":
        c = c[:, 0::2] | (c[:, 1::2] << 4)  # element 2i in the low nibble
    return c.to(torch.uint8), s.to(torch.uint8)


def unpack(qweight, fmt, K):
    """One code per element of the first K columns, int64."""
    q = qweight.cpu().to(torch.int64)
    return (torch.stack([q & 0xF, q >> 4], dim=2).reshape(q.shape[0], -1) if fmt == "fp4" else q)[:, :K]


def objective(W, Q, H):
    """The layer objective tr((W - Q) H (W - Q)^T) in fp64."""
    D = W.double() - Q.double()
    return float(((D @ H) * D).sum())


@functools.lru_cache(maxsize=None)
def case(N, K, seed=0):
    """W [N,K] fp32 = 0.02 * randn, H fp64 from 512 correlated tokens with every seventh channel x 4 and 1 % damping, and Hinv =
    chol(H^-1)^T computed in fp64 and cast to fp32 (injected: the factor kernel is not part of what these tests compare)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(512, K, dtype=torch.float64, generator=g)
    X = X @ (torch.eye(K, dtype=torch.float64) + 0.3 * torch.randn(K, K, dtype=torch.float64, generator=g) / math.sqrt(K))
    X[:, ::7] *= 4
    H = 2 * X.T @ X / 512
    H += 0.01 * H.diag().mean() * torch.eye(K, dtype=torch.float64)
    Hinv = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True).float().contiguous()
    W = 0.02 * torch.randn(N, K, generator=g)
    return W, H, Hinv


@functools.lru_cache(maxsize=None)
def reference(N, K, fmt, dtype):
    """gptq_mx_loop of case(N, K), computed once per session and left unchanged."""
    W, _, Hinv = case(N, K)
    return gptq_mx_loop(W, Hinv, fmt, dtype)
