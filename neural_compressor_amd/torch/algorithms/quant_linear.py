"""The frame of the quantised linear modules (W8A8Linear, FP8Linear, FP8BlockLinear, MXLinear, MXWeightOnlyLinear), of the groups that
share an activation (fp8_linear_group, mx_linear_group) and of the data-free quantizers (FP8Quantizer, MXQuantizer).

`QuantLinear` holds the one copy of the forward contract -- the reshape to rows, the empty batch, the type the product runs in, the
cast back for an fp32 input -- of the decode rule `_decodes`, of the device refusal and of the `from_float` skeleton.  A cell is a
subclass with its buffers, its `recover` / `extra_repr` and two hooks:

  _product(x2d, out_dtype)     y [rows, out_features] in out_dtype: the cell's quantise -> gemv-or-gemm lines, no host wait
  _quantize_weight(w)          the float weight [N, K] (on the module's device) -> the weight buffers: from_float's middle

and, where its members can share an activation (`linear_group`), the pieces of `_product` on their own and what a group agrees in:

  _quantize_rows(x2d)                           -> the codes of x and their scales
  _gemm(xq, xs, out_dtype)                      this member's product above the decode limit
  _gemv_multi(xq, xs, mods, out_dtype)          static: the products of all members in one decode launch, a list
  _group_key()                                  what members of one group agree in: a tuple that starts with in_features and the device

Functions of `ops` are looked up when they are called (`ops.fp8_gemm`), never bound in a class body: the tests patch `ops`.  The frame
never asks which subclass it serves.
"""

import torch

from ... import ops
from ...common.utils import logger
from ..utils.utility import get_module, half_or_fp16, set_module
from .base_algorithm import Quantizer


def e4m3_table(device=None):
    """The value of every OCP e4m3fn code, fp32 [256] (0x7f / 0xff are NaN and never stored)."""
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(device=device)


class QuantLinear(torch.nn.Module):
    # A cell with a decode GEMV sets all three beside its measurement: DECODE_GEMV switches the GEMV on, it serves up to DECODE_MAX_M
    # rows and never more than the kernel's own limit, the constant of `ops` that GEMV_LIMIT names (read from ops at every call, as
    # the functions are).  They are read through self, so a class is patched on its own
    DECODE_GEMV = False
    DECODE_MAX_M, GEMV_LIMIT = 0, None
    K_ALIGN = 128  # the K tile of every GEMM here, int8, FP8 and MX alike (ops.MX_KTILE)

    def __init__(self, in_features, out_features, float_type=torch.float16):
        """No device here (a stub can be built on the CPU): a concrete class calls _hip_device first, registers its buffers in its
        own order and ends with _register_bias."""
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.kp = -(-in_features // self.K_ALIGN) * self.K_ALIGN
        self.float_type = float_type

    @classmethod
    def _hip_device(cls, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{cls.__name__} needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation.")
        return dev

    def _register_bias(self, bias, dev):
        self.register_buffer("bias", torch.zeros(self.out_features, dtype=self.float_type, device=dev) if bias else None)

    @classmethod
    @torch.no_grad()
    def from_float(cls, linear, device="cuda", **kwargs):
        ft = half_or_fp16(linear.weight.dtype)
        new = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, device=device, float_type=ft, **kwargs)
        new._quantize_weight(linear.weight.detach().to(new.qweight.device))
        if linear.bias is not None:
            new.bias.copy_(linear.bias.detach().to(ft))
        return new

    def forward(self, input):
        x, dtype = input, input.dtype
        lead = x.shape[:-1]
        x2d = x.reshape(-1, self.in_features)
        out_dtype = dtype if dtype in (torch.float16, torch.bfloat16) else self.float_type
        if x2d.shape[0] == 0:
            return torch.empty((*lead, self.out_features), dtype=torch.float32 if dtype == torch.float32 else out_dtype, device=x.device)
        y = self._product(x2d, out_dtype)
        if dtype == torch.float32:  # an fp32 model keeps seeing fp32 activations (the kernel's epilogue emits 16-bit)
            y = y.float()
        return y.reshape(*lead, self.out_features)

    def _decodes(self, rows):
        return self.DECODE_GEMV and rows <= min(self.DECODE_MAX_M, getattr(ops, self.GEMV_LIMIT))

    def _product(self, x2d, out_dtype):
        raise NotImplementedError

    def _quantize_weight(self, w):
        raise NotImplementedError


def linear_group_plan(x, mods, cls, max_members, max_rows):
    """What `cls` members (FP8Linear / MXLinear) that multiply the same x share, or None where the group is the plain list of forwards:
    (x2d, out_dtype, every member decodes).  2 .. max_members members of one `_group_key()`, x on their device and not empty; an fp32 x
    needs one float_type; the row count decodes on every member or is above max_rows."""
    m0 = mods[0] if mods else None
    ok = (2 <= len(mods) <= max_members and all(isinstance(m, cls) for m in mods) and x.is_cuda and x.numel() > 0
          and x.shape[-1] == m0.in_features and x.device == m0.qweight.device and all(m._group_key() == m0._group_key() for m in mods))
    if not ok:
        return None
    half = x.dtype in (torch.float16, torch.bfloat16)
    out_dtype = x.dtype if half else m0.float_type
    x2d = x.reshape(-1, m0.in_features)
    rows = x2d.shape[0]
    decode = [m._decodes(rows) for m in mods]
    if not (half or all(m.float_type == out_dtype for m in mods)) or not (all(decode) or rows > max_rows):
        return None
    return x2d, out_dtype, all(decode)


def linear_group(x, mods, cls, max_members, max_rows):
    """The body of fp8_linear_group / mx_linear_group.  Under a plan (linear_group_plan) x is quantised ONCE, by the first member, and
    the products are one launch (`cls._gemv_multi`) where every member decodes, else `_gemm` per member; the cast back and the reshape
    are QuantLinear.forward's.  Without a plan, the plain list of forwards."""
    plan = linear_group_plan(x, mods, cls, max_members, max_rows)
    if plan is None:
        return [m(x) for m in mods]
    x2d, out_dtype, decode = plan
    xq, xs = mods[0]._quantize_rows(x2d)
    ys = cls._gemv_multi(xq, xs, mods, out_dtype) if decode else [m._gemm(xq, xs, out_dtype) for m in mods]
    if x.dtype == torch.float32:
        ys = [y.float() for y in ys]
    return [y.reshape(*x.shape[:-1], m.out_features) for y, m in zip(ys, mods)]


class DataFreeQuantizer(Quantizer):
    """The quantizer of an algorithm that calibrates nothing (FP8Quantizer, MXQuantizer): `prepare` returns the model unchanged and
    `convert` swaps every selected module.  quant_config: {layer name: dict}; a subclass names LOG (the prefix of its warnings) and
    STAYS_FLOAT (the key of that dict, and the value, also the default, that leaves the layer in float) and says which modules besides
    nn.Linear it takes (_is_experts, _unsupported_reason), what a selected module becomes (_quantized) and what it leaves on the
    model (_leave_info)."""

    LOG = STAYS_FLOAT = None

    def _selected(self, model):
        key, value = self.STAYS_FLOAT
        out = []
        for name, cfg in self.quant_config.items():
            if cfg.get(key, value) == value:
                continue
            mod = get_module(model, name)
            if isinstance(mod, torch.nn.Linear):
                out.append(name)
            elif self._is_experts(mod, cfg):
                why = self._unsupported_reason(mod, cfg)
                if why is None:
                    out.append(name)
                else:
                    logger.warning("%s: experts module %s stays in floating point: %s", self.LOG, name, why)
        return out

    def prepare(self, model, *args, **kwargs):
        return model  # data-free: nothing to calibrate

    @torch.no_grad()
    def convert(self, model, *args, **kwargs):
        dev = torch.device("cuda", torch.cuda.current_device())
        model.to(dev)
        model.eval()
        names = self._selected(model)
        if not names:
            logger.warning("%s: no nn.Linear selected, the model is returned unchanged", self.LOG)
        for name in names:
            set_module(model, name, self._quantized(get_module(model, name), self.quant_config[name], dev))
        self._leave_info(model, names)
        return model
