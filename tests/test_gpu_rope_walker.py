"""The rotary walker of csrc/fwd_elementwise.hip (one wave per token, cos / sin pieces held in registers across the heads) against the
original apply_rotary_pos_emb on the same device, bit for bit and stride for stride, at the smallest shapes that reach every branch:
fewer heads than one walker iteration takes, more (with a ragged last iteration), q and k head counts that differ, both head sizes
(8 and 32 heads per iteration), the item-per-lane kernel that other head sizes keep; then NaN, infinities and denormals planted in
the operands of all three forward kernels (the pair-wise hardware rounding has to write torch's NaN)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
B, T = 2, 5


def _assert_same(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    assert got.stride() == ref.stride(), f"{what}: strides {got.stride()} vs eager {ref.stride()}"
    diff = got.view(torch.int16) != ref.view(torch.int16)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} elements differ"


def _operands(hip, dtype, Hq, Hk, D, cs_batch, model_layout, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)

    def make(H):
        x = (torch.randn(B, T, H * D, generator=g) * 3).to(dtype).to(hip)
        x = x.view(B, T, H, D).transpose(1, 2)  # the view LlamaAttention hands to apply_rotary_pos_emb
        return x if model_layout else x.contiguous()

    ang = torch.rand(cs_batch, T, D, generator=g) * 6.28
    return make(Hq), make(Hk), ang.cos().to(dtype).to(hip), ang.sin().to(dtype).to(hip)


SPECIAL_BITS = {  # quiet, signalling and negative NaN; both infinities; two denormals; +-max; both zeros
    torch.bfloat16: [0x7FC0, 0x7F81, 0xFFFF, 0x7F80, 0xFF80, 0x0001, 0x8040, 0x7F7F, 0xFF7F, 0x0000, 0x8000],
    torch.float16: [0x7E00, 0x7C01, 0xFFFF, 0x7C00, 0xFC00, 0x0001, 0x8200, 0x7BFF, 0xFBFF, 0x0000, 0x8000],
}


def _plant(x, dtype, seed):
    """The special bit patterns of the dtype, three times each, at scattered places of x (in place, through whatever strides x has)."""
    bits = SPECIAL_BITS[dtype]
    xi = x.view(torch.int16)
    g = torch.Generator(device="cpu").manual_seed(seed)
    where = torch.randperm(x.numel(), generator=g)[: 3 * len(bits)].tolist()
    for n, i in enumerate(where):
        idx = []
        for s in reversed(x.shape):
            idx.append(i % s)
            i //= s
        b = bits[n % len(bits)]
        xi[tuple(reversed(idx))] = b if b < 0x8000 else b - 0x10000
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model_layout", [True, False])
@pytest.mark.parametrize("D", [32, 128, 48])  # 48: three pieces per head half, no power of two -- the item-per-lane kernel
def test_walker_bit_equal_to_eager(hip, dtype, model_layout, D):
    from transformers.models.llama import modeling_llama

    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    n = 0
    for Hq, Hk in ((4, 4), (4, 2), (9, 3)):
        for cs_batch in (1, B):
            q, k, cos, sin = _operands(hip, dtype, Hq, Hk, D, cs_batch, model_layout, seed=100 * D + n)
            ref = modeling_llama.apply_rotary_pos_emb(q, k, cos, sin)
            got = ff.rope(q, k, cos, sin)
            what = f"H=({Hq},{Hk}) D={D} cos batch {cs_batch}"
            assert got is not None, what
            _assert_same(got[0], ref[0], "q " + what)
            _assert_same(got[1], ref[1], "k " + what)
            n += 1
    assert n == 6


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 128, 48])
def test_rope_with_planted_specials(hip, dtype, D):
    """A NaN in the rotated half reaches memory with its sign flipped (eager negates that half in a kernel of its own): in fp16 the sign
    is visible, and the kernel has to negate where eager does, not wherever the compiler would like to."""
    from transformers.models.llama import modeling_llama

    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    def two_nans(x, cos):
        """Outputs that two different NaNs reach (x[d] * cos[d] + rot[d] * sin[d]: x[d], cos[d], x[d +- D/2]).  Which of the two payloads
        an fp16 result then carries depends on the operand order of one hardware instruction, which no source fixes: not planted."""
        xn, cn = torch.isnan(x), torch.isnan(cos).unsqueeze(1).expand_as(x)
        rn = torch.cat([xn[..., D // 2:], xn[..., : D // 2]], dim=-1)
        return int((xn.int() + cn.int() + rn.int() >= 2).sum())

    for model_layout in (True, False):
        for seed in range(64):  # the first planting without such a place (the operands come from CPU generators: always the same one)
            q, k, cos, sin = _operands(hip, dtype, 9, 3, D, B, model_layout, seed=7 + D)
            _plant(q, dtype, 3 * seed + 1)
            _plant(k, dtype, 3 * seed + 2)
            _plant(cos, dtype, 3 * seed + 3)
            if two_nans(q, cos) == 0 and two_nans(k, cos) == 0:
                break
        else:
            raise AssertionError("no planting without colliding NaNs")
        ref = modeling_llama.apply_rotary_pos_emb(q, k, cos, sin)
        assert bool(torch.isnan(ref[0]).any()) and bool(torch.isnan(ref[1]).any())
        got = ff.rope(q, k, cos, sin)
        assert got is not None
        _assert_same(got[0], ref[0], f"q D={D}")
        _assert_same(got[1], ref[1], f"k D={D}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_mul_with_planted_specials(hip, dtype):
    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    n = 8 * 37 + 3  # 37 pieces of 16 bytes and a tail of three
    g = torch.Generator(device="cpu").manual_seed(21)
    gate = _plant((torch.randn(n, generator=g) * 4).to(dtype).to(hip), dtype, 4)
    up = _plant((torch.randn(n, generator=g) * 4).to(dtype).to(hip), dtype, 5)
    gate[-1], up[-2] = float("nan"), float("inf")  # the tail's own path
    ref = torch.nn.functional.silu(gate) * up
    assert bool(torch.isnan(ref).any())
    got = ff.silu_mul(gate, up)
    assert got is not None
    _assert_same(got, ref, "silu_mul")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [256, 8192 + 8])  # one wave per row, and eight waves per row with a ragged last piece
def test_rmsnorm_with_planted_specials(hip, dtype, cols):
    from transformers.models.llama import modeling_llama

    from neural_compressor_amd.torch.algorithms.weight_only import fused_forward as ff

    rows = 9
    g = torch.Generator(device="cpu").manual_seed(31 + cols)
    x = (torch.randn(rows, cols, generator=g) * 2).to(dtype).to(hip)
    fi = torch.finfo(dtype)
    x[1, 5] = float("nan")                 # a NaN row: every output of it is torch's NaN
    x[2, cols - 1] = float("inf")          # an infinite mean: rsqrt gives 0, inf * 0 a NaN in that one place
    x[3, 7] = float("-inf")
    x[4] = fi.smallest_normal / 4          # a row of denormals
    x[5, 3], x[5, 11] = fi.smallest_normal / 2, -fi.smallest_normal / 4
    x[6] = 0
    weight = (1 + 0.25 * torch.randn(cols, generator=g)).to(dtype).to(hip)
    weight[0], weight[9] = float("nan"), fi.smallest_normal / 4
    m = modeling_llama.LlamaRMSNorm(cols, eps=1e-5).to(hip).to(dtype)
    with torch.no_grad():
        m.weight.copy_(weight)
        ref = m(x)
        got = ff.rmsnorm(x, m.weight, m.variance_epsilon)  # (under no_grad: the fused route declines a weight that wants a gradient)
    assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref[7]).all())
    assert got is not None
    _assert_same(got, ref, f"rmsnorm cols={cols}")
