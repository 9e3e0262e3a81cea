"""The weight-only Linear operator for MI355X.

Drop-in for the reference's operator classes (neural_compressor/torch/algorithms/weight_only/modules.py):
  WeightOnlyLinear (abstract)        :91-154
  INCWeightOnlyLinear                :157-627   -> MI355XWeightOnlyLinear (alias INCWeightOnlyLinear)
  UnpackedWeightOnlyLinearParams     :74-88
  MulLinear                          :907-949

Same constructor, same buffers (`qweight`, `scales`, `qzeros`, `bias`, `g_idx`, `scale_bf16_to_fp8`) with the
same shapes / dtypes, so state_dicts round-trip with the reference and with HF / AutoGPTQ checkpoints.  What
changes is where the arithmetic runs: pack / unpack / recover are HIP kernels over HBM-resident tensors
(no per-nibble device syncs, no Python loop over K), and forward is a fused INT4->bf16 dequant-GEMM on the
matrix cores instead of "recover once, cache the dense weight, F.linear".  There is no CPU path: tensors
must live on a HIP device.
"""

import math
from abc import abstractmethod

import torch

from .... import ops
from ....common.utils import logger
from ..fused_experts import is_silu


class UnpackedWeightOnlyLinearParams(dict):
    """Unpacked tensors of a packed module: int_weight, scales, scale_bf16_to_fp8, zp, g_idx, bias."""

    def __init__(self, unpack_weight, scales, scale_bf16_to_fp8, unpack_zp, **kwargs):
        super().__init__(int_weight=unpack_weight, scales=scales, scale_bf16_to_fp8=scale_bf16_to_fp8, zp=unpack_zp, **kwargs)

    def to(self, device):
        for key, value in self.items():
            if isinstance(value, torch.Tensor):
                self[key] = value.to(device)
        return self


class WeightOnlyLinear(torch.nn.Module):
    """Abstract operator: a device class implements pack / unpack / forward (reference modules.py:91)."""

    def __init__(self, in_features, out_features, dtype, bits, group_size, device, scale_dtype, **kwargs):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.dtype = dtype
        self.bits = bits
        self.group_size = group_size if group_size != -1 else in_features
        self.device = device
        self.scale_dtype = scale_dtype
        self.kwargs = kwargs

    @abstractmethod
    def pack(self, *args, **kwargs):
        raise NotImplementedError(f"{self.__class__.__name__} doesn't implement `pack` function. ")

    @abstractmethod
    def unpack(self, *args, **kwargs):
        raise NotImplementedError(f"{self.__class__.__name__} doesn't implement `unpack` function. ")

    @abstractmethod
    def forward(self, input):
        raise NotImplementedError(f"{self.__class__.__name__} doesn't implement `forward` function. ")

    def extra_repr(self):
        return "in_features={}, out_features={}, bits={}, group_size={}, bias={}".format(
            self.in_features, self.out_features, self.bits, self.group_size, self.bias is not None
        )


_CBITS = {torch.int8: 8, torch.int16: 16, torch.int32: 32, torch.int64: 64}


def _hip_device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(
            f"MI355XWeightOnlyLinear needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation; "
            "construct the module with device='cuda'."
        )
    return dev


class MI355XWeightOnlyLinear(WeightOnlyLinear):
    """Packed-weight Linear whose pack / unpack / recover / forward are HIP kernels (gfx950)."""

    def __init__(
        self,
        in_features,
        out_features,
        dtype="int",
        bits=4,
        group_size=32,
        zp=False,
        bias=False,
        scale_dtype=torch.float32,
        compression_dtype=torch.int32,
        compression_dim=1,
        g_idx=False,
        device="cuda",
        use_optimum_format=True,
        **kwargs,
    ):
        super().__init__(in_features, out_features, dtype, bits, group_size, device, scale_dtype=scale_dtype, **kwargs)
        if not (isinstance(bits, int) and 1 <= bits <= 8):  # the widths the reference's configs tune (config.py:211)
            raise ValueError(f"bits={bits}: weight-only widths are 1..8 (n_pack = compress_bits // bits, reference modules.py:231)")
        dev = _hip_device(device)
        self.use_optimum_format = use_optimum_format
        self._lut = None
        if "int" not in self.dtype:  # nf4 / fp4 code books (reference modules.py:213-221)
            from .utility import FLOAT_MAPPING, INT_MAPPING

            if self.dtype not in FLOAT_MAPPING:
                raise NotImplementedError(f"dtype={dtype}: integer, NF4 and FP4 weight-only formats are implemented")
            assert bits == 4, "NF4 / FP4 are 4-bit formats"
            self.use_optimum_format = False  # optimum_format doesn't suit symmetric nf4 / fp4 (reference :216)
            # stored integer (-8..7) -> code-book value; unpack() applies it like the reference's int2float_mapping
            lut = torch.zeros(16, dtype=torch.float32)
            lut[torch.tensor(INT_MAPPING[self.dtype]) + 8] = torch.tensor(FLOAT_MAPPING[self.dtype], dtype=torch.float32)
            self._lut = lut.to(dev)
        self.compression_dim = compression_dim
        assert compression_dtype in _CBITS, f"Only support torch.int8|16|32|64 as compressed dtype. but got {compression_dtype}"
        assert compression_dim in (0, 1), "Only support 0 or 1 as compression dimension, 0 is output channel, 1 is input channel."
        K, N, gs = in_features, out_features, self.group_size
        G = math.ceil(K / gs)
        self.register_buffer("scale_bf16_to_fp8", torch.zeros(1, dtype=torch.bfloat16, device=dev))
        if self.use_optimum_format:
            self.float_type = torch.float16
            self.compression_dtype = torch.int32
            self.compress_bits = 32
            self.n_pack = 32 // bits
            self.register_buffer("scales", torch.zeros((G, N), dtype=self.float_type, device=dev))
            self.register_buffer("qweight", torch.zeros((math.ceil(K / self.n_pack), N), dtype=torch.int32, device=dev))
            self.register_buffer("qzeros", torch.zeros((G, math.ceil(N / self.n_pack)), dtype=torch.int32, device=dev))
            self.register_buffer("bias", torch.zeros(N, dtype=self.float_type, device=dev))
        else:
            self.compression_dtype = compression_dtype
            self.compress_bits = _CBITS[compression_dtype]
            self.n_pack = self.compress_bits // bits
            self.float_type = scale_dtype
            self.register_buffer("scales", torch.zeros((N, G), dtype=self.float_type, device=dev))
            if compression_dim == 1:
                self.register_buffer("qweight", torch.zeros((N, math.ceil(K / self.n_pack)), dtype=compression_dtype, device=dev))
                if zp:
                    self.register_buffer("qzeros", torch.zeros((N, math.ceil(G / self.n_pack)), dtype=compression_dtype, device=dev))
            else:
                self.register_buffer("qweight", torch.zeros((math.ceil(N / self.n_pack), K), dtype=compression_dtype, device=dev))
                if zp:
                    self.register_buffer("qzeros", torch.zeros((math.ceil(N / self.n_pack), G), dtype=compression_dtype, device=dev))
            if bias:
                self.register_buffer("bias", torch.zeros(N, dtype=self.float_type, device=dev))
            else:
                self.bias = None
        if g_idx:
            self.register_buffer("g_idx", torch.zeros(K, dtype=torch.int32, device=dev))
        else:
            self.g_idx = None

    # ------------------------------------------------------------------------------------------------
    def pack(self, int_weight, scales, zp, bias, scale_bf16_to_fp8=None, g_idx=None, **kwargs):
        """Pack integer weights (reference modules.py:321-375); arguments are NOT mutated (the reference
        adds the sym shift / subtracts 1 from zp in place)."""
        dev = self.qweight.device
        N, K = self.out_features, self.in_features
        assert bias is None or hasattr(self, "bias"), "bias is not set when initializing."
        self._begin_pack(bias, g_idx, self.use_optimum_format)
        if scale_bf16_to_fp8 is not None:
            self.scale_bf16_to_fp8 = scale_bf16_to_fp8.to(dev).type(self.float_type)
        int_weight = int_weight.to(dev)
        scales = scales.to(dev)
        zp = None if zp is None else zp.to(dev)
        if self.use_optimum_format:
            assert tuple(scales.shape) == (N, self.scales.shape[0]), f"{scales.shape} Scale shape is mismatched."
            shift = 2 ** (self.bits - 1) if zp is None else 0
            ops.woq_pack(
                int_weight, scales, zp, self.bits, shift, qweight=self.qweight, qzeros=self.qzeros, scales_out=self.scales
            )
            return
        # non-optimum layouts (modules.py:270-314): generic row packer + layout transposes
        assert scales.shape == self.scales.shape, f"{scales.shape} != {self.scales.shape} Scale shape is mismatched."
        self.scales = scales.type(self.float_type).contiguous()
        iw = int_weight.to(torch.int32)
        if self.compression_dim == 0:
            iw = iw.T.contiguous()
        packed = ops.pack_rows(iw, self.bits, self.compress_bits)
        if self.compression_dim == 0:
            packed = packed.T.contiguous()
        assert packed.shape == self.qweight.shape, "output channels mismatch, please check."
        self.qweight.copy_(packed)
        if zp is not None:
            assert hasattr(self, "qzeros"), "zp is not set when initializing."
            z = zp.to(torch.int32)
            if self.compression_dim == 0:
                z = z.T.contiguous()
            pz = ops.pack_rows(z, self.bits, self.compress_bits)
            if self.compression_dim == 0:
                pz = pz.T.contiguous()
            self.qzeros.copy_(pz)

    def _begin_pack(self, bias, g_idx, sort_g_idx):
        """What pack() and pack_codes() do before they write the packed buffers: drop what was derived from the old contents, store
        the bias and the g_idx (`sort_g_idx`: in the optimum format's argsort // group_size form, reference modules.py:341-344)."""
        dev = self.qweight.device
        self._plan_key = None  # the kernels write the buffers through raw pointers: drop the cached forward plan
        self.__dict__["_call"] = None  # ... and the prepared call (its converted bias / plan belong to the old contents)
        if bias is not None:
            self.bias = bias.detach().to(dev).type(self.float_type)
        if g_idx is not None:
            assert hasattr(self, "g_idx"), "g_idx is not set when initializing."
            g = g_idx.to(dev).type(torch.int32)
            if sort_g_idx:
                g = (torch.argsort(g) // self.group_size).type(torch.int32)  # (index plumbing)
            self.g_idx = g.contiguous()

    def pack_codes(self, codes, scales, zp, bias, g_idx=None):
        """MI355X-native fast path (optimum format only): pack already-offset codes 0..2^bits-1 (uint8 [N,K], what
        the GPTQ column-loop kernel emits) instead of int32 signed ints.  Produces bit-identical buffers to
        `pack(codes - 2^(bits-1), scales, None, ...)` for sym and `pack(codes, scales, zp, ...)` for asym."""
        assert self.use_optimum_format, "pack_codes writes the optimum layout"
        self._begin_pack(bias, g_idx, True)
        ops.woq_pack(codes, scales, zp, self.bits, 0, qweight=self.qweight, qzeros=self.qzeros, scales_out=self.scales)

    def unpack(self):
        """Reference modules.py:377-411 -> UnpackedWeightOnlyLinearParams (int16 ints, as the reference)."""
        N, K = self.out_features, self.in_features
        if self.use_optimum_format:
            G = self.scales.shape[0]
            if self.scales.dtype == torch.float16 and self.scales.is_contiguous():
                iw, zp, scales = ops.woq_unpack(self.qweight, self.qzeros, N, K, G, self.bits, scales=self.scales)  # one launch
            else:
                iw, zp = ops.woq_unpack(self.qweight, self.qzeros, N, K, G, self.bits)
                scales = self.scales.T.contiguous()
        else:
            has_zp = hasattr(self, "qzeros")
            qw = self.qweight if self.compression_dim == 1 else self.qweight.T.contiguous()
            iw = ops.unpack_rows(qw.contiguous(), self.bits, self.compress_bits, has_zp)
            if self.compression_dim == 0:
                iw = iw.T.contiguous()
            iw = iw[:N, :K].contiguous()
            if self._lut is not None:  # nf4 / fp4: the unpacked "weight" is the code-book value (reference :391-395)
                iw = self._lut.to(iw.device)[(iw.to(torch.int64) + 8)]
            zp = None
            if has_zp:
                qz = self.qzeros if self.compression_dim == 1 else self.qzeros.T.contiguous()
                zp = ops.unpack_rows(qz.contiguous(), self.bits, self.compress_bits, True)
                if self.compression_dim == 0:
                    zp = zp.T.contiguous()
                zp = zp[: self.scales.shape[0], : self.scales.shape[1]].contiguous()
            scales = self.scales
        return UnpackedWeightOnlyLinearParams(iw, scales, self.scale_bf16_to_fp8, zp, g_idx=self.g_idx, bias=self.bias)

    def recover(self, dtype=None):
        """Dense weight [N,K] (reference modules.py:413-443).  Default dtype = float_type (fp16 in optimum format)."""
        out_dtype = dtype or self.float_type
        if self.use_optimum_format:
            return ops.woq_dequant(
                self.qweight, self.scales, self.qzeros, self.g_idx, self.out_features, self.in_features,
                self.group_size, self.bits, out_dtype=out_dtype,
            )
        p = self.unpack()
        if self._lut is not None:  # code-book value x group scale (reference :438-441), zp is None for these formats
            N, K, gs = self.out_features, self.in_features, self.group_size
            gs = K if gs == -1 or gs > K else gs
            gi = (torch.arange(K, device=p["scales"].device) // gs) if self.g_idx is None else self.g_idx.long()
            return (p["int_weight"].float() * p["scales"].float()[:, gi]).to(out_dtype)
        return ops.dequant_ints(p["int_weight"], p["scales"], p["zp"], self.g_idx, self.group_size, out_dtype)

    def forward(self, input):
        """y = x W^T + b with W dequantised on the fly (reference modules.py:594-610).

        bf16 / fp16 inputs are computed in their own dtype (fp32 accumulate); any other dtype is cast to fp16 for the
        multiplication (what the reference does on an accelerator: `input.type(self.weight.dtype)` with an fp16 weight)
        and an fp32 input gets an fp32 output back, as on the reference's CPU path (:598-600), so an fp32 model keeps
        running after some of its layers are packed (true_sequential re-runs the block mid-way).
        """
        x = input
        # decode path: a prepared call for the plan (ops.WoqGemmCall and its kin); the 6-us kernels make the host side count
        d = self.__dict__
        call = d.get("_call")
        if call is not None and x.dtype is call.dtype and x.device == call.dev and x.is_contiguous() and x.numel() > 0 and x.shape[-1] == call.K:
            bufs = self._buffers
            # (_prepared_serves for the call held, written out: the method call is host time on the plain 4-bit route, profiles/decode_host/)
            if (call.current(bufs["qweight"], bufs["scales"], bufs.get("qzeros"), bufs.get("bias", d.get("bias")), bufs.get("g_idx", d.get("g_idx")))
                    and (not call.lut or (self.LUT_FUSED and x.numel() <= self.LUT_MAX_M * call.K))
                    and (call.ko is None or self.ACT_ORDER_FUSED_GATHER)
                    and (not call.anyw or (self.ODD_WIDTH_DECODE and not self.ODD_WIDTH_FUSED
                                           and x.numel() <= min(self.ODD_WIDTH_DECODE_MAX_M, call.MAX_M) * call.K
                                           and (call.ko is None or call.gather_max_mn == self.ODD_WIDTH_GATHER_MAX_MN)))):
                y = call(x if x.dim() == 2 else x.view(-1, call.K))
                return y if x.dim() == 2 else y.view(*x.shape[:-1], call.N)
        if x.dtype not in (torch.bfloat16, torch.float16):
            x = x.to(torch.float16)
        lead = x.shape[:-1]
        x2d = x.reshape(-1, self.in_features)
        if x2d.shape[0] == 0:  # empty batch: nothing to launch (F.linear returns an empty tensor too)
            return x2d.new_empty((*lead, self.out_features), dtype=torch.float32 if input.dtype == torch.float32 else x2d.dtype)
        if not x2d.is_contiguous():
            x2d = x2d.contiguous()
        plan = self._forward_plan()
        d["_call"] = None
        if plan == "fused" and self._fused_max_m is not None and x2d.shape[0] > self._fused_max_m:
            plan = "dense"  # (a group size the fast kernels do not take: see _forward_plan)
        # the prepared call serves the module from now on -- or, where this batch takes another route, none does
        call = d["_call"] = self._prepare_call(plan, x2d.dtype, x2d.shape[0])
        if call is not None:
            y = call(x2d)
        elif plan == "fused":  # (_fused_max_m: decode-sized batches of such a module)
            y = ops.woq_gemm(x2d, self.qweight, self.scales, self.qzeros, self.bias, self.out_features, self.in_features, self.group_size, self.bits)
        elif plan == "fused_act_order":
            # ACT_ORDER_FUSED_GATHER = False: the activations are gathered by a torch kernel in front of the ordinary launch
            y = ops.woq_gemm(
                x2d.index_select(1, self._k_order), self._qweight_sorted, self.scales, self.qzeros, self.bias,
                self.out_features, self.in_features, self.group_size, self.bits,
            )
        elif plan == "fused_g_idx":
            # an irregular g_idx (not a permutation of whole groups): inc_woq_gemm's general tile kernel reads scale / zero of
            # group g_idx[k] per element (reference modules.py:427-431 semantics), still without a dense weight
            y = ops.woq_gemm(x2d, self.qweight, self.scales, self.qzeros, self.bias, self.out_features, self.in_features,
                             self.group_size, self.bits, g_idx=self.g_idx)
        else:
            # non-optimum layouts (compression_dim / int8-16-64 containers, NF4 / FP4 code books beyond LUT_MAX_M rows), odd widths beyond
            # their decode limit: HIP dequant + dense library GEMM
            w = self.recover(dtype=x2d.dtype)
            b = None if self.bias is None else self.bias.to(x2d.dtype)
            y = torch.nn.functional.linear(x2d, w, b)
        if input.dtype == torch.float32:
            y = y.float()
        return y.reshape(*lead, self.out_features)

    # act_order modules (plan "fused_act_order"): True = a prepared call that gathers the activations inside the decode kernels
    # (inc_woq_gemm_perm, up to 64 rows on the streaming routes); False = x.index_select + ops.woq_gemm per call, two launches
    ACT_ORDER_FUSED_GATHER = True
    # widths other than 4 / 8 bits: True = multiply through inc_woq_gemm's per-element tile form (no dense weight ever exists; 8-10 x
    # slower), False = HIP recover() into a transient dense weight + the library GEMM (what the reference's forward does on its CPU)
    ODD_WIDTH_FUSED = False
    # ... and at decode, whatever the above says for larger batches: True = up to ODD_WIDTH_DECODE_MAX_M rows of an eligible module (optimum
    # layout, contiguous groups of a power of two >= 32 or one per row, K % 32 == 0, N % 4 == 0, N >= 64) go through inc_woq_gemv_anyw,
    # one launch that reads the packed words once and never builds the dense weight; False = the dense route for every batch.
    # ODD_WIDTH_FUSED = True takes precedence (its plan is "fused").
    # An act_order module of these widths (eligible in everything but its g_idx, which permutes whole groups) takes the same route
    # through inc_woq_gemv_anyw_perm while ACT_ORDER_FUSED_GATHER is on too: the packed fields are sorted along K by group once per packed
    # state (ops.sort_packed_k) and the kernel gathers the activations.  The K-sorted copy doubles such a module's packed-weight memory,
    # as it does at 4 bits; with either switch off the module runs the dense route exactly as before (the copy stays until re-packing).
    ODD_WIDTH_DECODE = True
    # the kernel's own limit.  Measured so far (profiles/anyw_decode/anyw_decode_time.log): 3 bits, 4096^2, M = 1 / 4: 8.3 / 8.5 us against
    # 41.1 us for the dense route.  M = 16, 2 bits and the two other shapes of scripts/anyw_decode_time.py are NOT measured: 16 rests on
    # the kernel's work not depending on M (the MFMA takes 16 rows, live or not) while the dense route writes and re-reads a dense weight.
    # Lower it to 4 or 1 if a row of that script loses.
    ODD_WIDTH_DECODE_MAX_M = 16
    # act_order modules of these widths: outputs (rows of x times out_features) up to which the activations are gathered INSIDE the kernel
    # (inc_woq_gemv_anyw_perm, one launch).  Above it, up to ODD_WIDTH_DECODE_MAX_M rows, the prepared call runs x.index_select(1, k_order)
    # + inc_woq_gemv_anyw on the K-sorted words: two launches, the same bits.  Every 64-column strip repeats the in-kernel gather and its
    # 2-byte loads touch one cache line per (row, k), so its cost grows with rows x columns while the torch gather is paid once.  Measured
    # (profiles/anyw_decode/anyw_group_time.log, 3 bits g128, us gathered | index_select form): 4096^2 M = 1 / 4 / 8 / 16: 9.3 | 12.7, 11.5 | 12.8,
    # 14.5 | 13.0, 18.5 | 13.7; 11008 x 4096 (per module of the pair) M = 1 / 4: 16.7 | 17.6, 22.6 | 17.8.  The kernel wins up to 4 x 4096
    # outputs and loses from 8 x 4096 and 4 x 11008 on; nothing in between is measured, so the limit is the largest product that won.
    # woq_linear_group applies it to a group with act_order members through the widest member (beyond it: the single calls).
    ODD_WIDTH_GATHER_MAX_MN = 4 * 4096
    # 4-bit row-packed modules (compression_dim = 1, dtype int / nf4 / fp4 / fp4_e2m1 / fp4_e2m1_bnb, no g_idx, K % 32 == 0, groups of
    # 32 k multiples): True = inc_woq_gemm_lut, False = HIP recover() into a transient dense weight + the library GEMM
    LUT_FUSED = True
    # ... up to this many rows of x: NF4 g32 through inc_woq_gemm_lut is 2.2-3.1 x faster than the dense route at M = 256 and as fast or
    # slower from M = 1024 on (272.1 vs 260.2 us at 4096^2, 759.3 vs 736.6 us at 11008 x 4096; 2.8-3.5 x slower at M = 4096:
    # profiles/r7/lut_gemm_time.log), so larger batches keep HIP recover() + the library GEMM
    LUT_MAX_M = 256

    def _forward_plan(self):
        """Pick the forward route once per packed state.  A per-element `g_idx` (GPTQ act_order, HF desc_act
        checkpoints; modules.py:341-344) that is a permutation of whole groups is handled by sorting the K axis by group:
        x W^T = x[:, p] W[:, p]^T, and in the sorted order the groups are contiguous again, so the fused kernel runs on a
        K-sorted copy of the packed words with only an activation gather per call."""
        # in-place re-packing / load_state_dict bump the tensors' version counters -> the plan is rebuilt
        key = (self.qweight.data_ptr(), self.qweight._version,
               None if self.g_idx is None else (self.g_idx.data_ptr(), self.g_idx._version), self.ODD_WIDTH_FUSED, self.LUT_FUSED)
        if getattr(self, "_plan_key", None) == key:
            return self._plan
        plan = "dense"
        # 4 / 8 bits: whole words per group (the fast kernels); every other width 1..7 runs inc_woq_gemm's per-element tile form,
        # which takes any group size (n_pack = 10 / 6 / 5 for 3 / 5 / 6 bits never divides one)
        # (the per-element form is the memory-saving route, not the fast one: measured 376-480 us against 40-100 us for HIP recover() +
        # the library GEMM at 4096^2 for every M from 1 to 4096, profiles/r6/anyw_route_time.log -- so it is opt-in: ODD_WIDTH_FUSED)
        fusable = self.use_optimum_format and (self.group_size % self.n_pack == 0 if self.bits in (4, 8) else self.ODD_WIDTH_FUSED)
        # group sizes that are neither a power of two >= 32 nor the whole row (e.g. 96) run inc_woq_gemm's general 128 x 128 tile kernel
        # above 16 rows: 190-245 us at 4096 x 4032 against 34-74 us for HIP recover() + the library GEMM (scripts/route_sweep.py) -- such
        # modules keep the fused form for decode-sized batches only
        K = self.in_features
        gs_eff = K if (self.group_size == -1 or self.group_size >= K) else self.group_size
        fast_groups = gs_eff == K or (gs_eff >= 32 and (gs_eff & (gs_eff - 1)) == 0)
        self._fused_max_m = None if (fast_groups or self.bits not in (4, 8)) else 16
        anyw = self._decode_anyw_eligible()
        kind, order = "contiguous", None
        if self.g_idx is not None and (fusable or anyw):  # (a device sync: once per packed state)
            kind, order = _classify_g_idx(self.g_idx, K, self.group_size)
        self._decode_anyw = anyw and kind == "contiguous"
        self._decode_anyw_perm = False
        if fusable:
            if kind == "contiguous":
                plan = "fused"
            elif kind == "permuted" and K % self.n_pack == 0:
                plan = "fused_act_order"
            else:
                plan = "fused_g_idx"  # groups of uneven size, or ragged words: the library's general kernel looks the group up per k
        elif anyw and kind == "permuted":
            # an odd width whose g_idx permutes whole groups: the plan stays "dense" (larger batches), decode gathers through the order
            self._decode_anyw_perm = True
        self._k_order = self._k_order32 = self._qweight_sorted = None
        if plan == "fused_act_order" or self._decode_anyw_perm:
            self._qweight_sorted = ops.sort_packed_k(self.qweight, order, K, self.bits)
            self._k_order = order
            self._k_order32 = order.to(torch.int32)  # what inc_woq_gemm_perm / inc_woq_gemv_anyw_perm read
        self._lut_table = self._lut_eligible() if (not self.use_optimum_format and self.LUT_FUSED) else None
        if self._lut_table is not None:
            plan = "fused_lut"
        self._plan_key, self._plan = key, plan
        return plan

    def _prepared_serves(self, M, lut, anyw, perm, gather_max_mn):
        """A prepared call of this kind -- `lut`: inc_woq_gemm_lut, `anyw`: the odd-width GEMV, `perm`: with the act_order gather, built
        for `gather_max_mn` -- may serve M rows now (M = None: by the switches alone, the caller has its own row limit)?  The one place
        where the switches and limits above decide that, at call time (they may change between two forwards): _prepare_call and
        _group_member ask here, and forward's guard repeats it inline for the call it holds (the flipping tests hold the two together)."""
        if lut:
            return self.LUT_FUSED and M <= self.LUT_MAX_M
        if perm and not self.ACT_ORDER_FUSED_GATHER:
            return False
        if anyw:
            return (self.ODD_WIDTH_DECODE and not self.ODD_WIDTH_FUSED
                    and (M is None or M <= min(self.ODD_WIDTH_DECODE_MAX_M, ops.GEMV_ANYW_MAX_M))
                    and (not perm or gather_max_mn == self.ODD_WIDTH_GATHER_MAX_MN))
        return True

    def _prepare_call(self, plan, dtype, M):
        """The prepared call that serves M rows of `dtype` under `plan` (and every later batch its guard admits), or None where the
        batch takes an un-prepared route: _fused_max_m modules, act_order with ACT_ORDER_FUSED_GATHER off, "fused_g_idx", dense."""
        lut = plan == "fused_lut"
        # 1 / 2 / 3 / 5 / 6 / 7 bits at decode: inc_woq_gemv_anyw streams the packed words once; recover() never runs.  act_order modules:
        # the K-sorted words and the gather inside the kernel (inc_woq_gemv_anyw_perm / inc_woq_gemm_perm), still one launch
        anyw = plan == "dense" and (self._decode_anyw or self._decode_anyw_perm)
        perm = plan == "fused_act_order" or (anyw and not self._decode_anyw)
        if not (lut or anyw or perm or (plan == "fused" and self._fused_max_m is None)):
            return None
        if not self._prepared_serves(M, lut, anyw, perm, self.ODD_WIDTH_GATHER_MAX_MN):
            return None
        if lut:
            # 4-bit row-packed modules (NF4 / FP4 code books, non-optimum integers): inc_woq_gemm_lut decodes the fields through a
            # 16-entry table per (row, group) in registers; recover() never runs
            return ops.WoqGemmLutCall(self.qweight, self._lut_table, self.scales, getattr(self, "qzeros", None), self.bias,
                                      self.out_features, self.in_features, self.group_size, self._lut is None, dtype)
        kw = dict(owner_g_idx=self.g_idx)
        if perm:
            kw.update(k_order=self._k_order32, owner_qweight=self.qweight)
            if anyw:
                kw["gather_max_mn"] = self.ODD_WIDTH_GATHER_MAX_MN
        return (ops.WoqGemvAnywCall if anyw else ops.WoqGemmCall)(
            self._qweight_sorted if perm else self.qweight, self.scales, self.qzeros, self.bias, self.out_features, self.in_features,
            self.group_size, self.bits, dtype, **kw)

    def _group_member(self):
        """(part, order) of the module in a one-launch decode group (woq_linear_group, woq_gated_pair), or None.  4 / 8 bits: the plain
        fused plan, or -- while ACT_ORDER_FUSED_GATHER is on -- the act_order plan with the K-sorted words and the order the kernels
        gather x through.  1 / 2 / 3 / 5 / 6 / 7 bits: a module that decodes through inc_woq_gemv_anyw or, likewise, its gathered form."""
        plan = self._forward_plan()
        anyw = self.bits not in (4, 8)
        if anyw:
            perm = self._decode_anyw_perm
            ok = plan == "dense" and (self._decode_anyw or perm)
        else:
            perm = plan == "fused_act_order"
            ok = plan == "fused" or perm
        if not ok or not self._prepared_serves(None, False, anyw, perm, self.ODD_WIDTH_GATHER_MAX_MN):
            return None
        return ((self._qweight_sorted if perm else self.qweight, self.scales, self.qzeros, self.bias, self.out_features),
                self._k_order32 if perm else None)

    def _decode_anyw_eligible(self):
        """inc_woq_gemv_anyw takes the module's layout at decode (ODD_WIDTH_DECODE)?  Everything but the g_idx, which _forward_plan
        classifies: contiguous -> the plain kernel, a permutation of whole groups -> the gathered form."""
        return bool(self.use_optimum_format and ops.gemv_anyw_takes(self.out_features, self.in_features, self.group_size, self.bits)
                    and self.scales.dtype is torch.float16 and self.scales.is_contiguous() and self.qweight.is_contiguous()
                    and self.qzeros.is_contiguous() and not self.qweight.data_ptr() % 16 and not self.scales.data_ptr() % 8)

    def _lut_eligible(self):
        """The field -> value table of the module where inc_woq_gemm_lut takes it, else None."""
        K, gs = self.in_features, self.group_size
        gs_eff = K if (gs == -1 or gs >= K) else gs
        has_zp = hasattr(self, "qzeros")
        if (self.compression_dim != 1 or self.bits != 4 or self.g_idx is not None or K % 32 != 0 or (gs_eff != K and gs_eff % 32 != 0)
                or self.scales.dtype not in (torch.float32, torch.float16, torch.bfloat16) or not self.scales.is_contiguous()
                or not self.qweight.is_contiguous() or self.qweight.data_ptr() % 16 or (has_zp and not self.qzeros.is_contiguous())):
            return None
        f = list(range(16))
        if self._lut is not None:  # code book: the stored code is sign-extended, then +8 (unpack)
            if has_zp:
                return None  # (recover() of a code book has no zero point)
            lut = self._lut.cpu().tolist()
            return [lut[(v + 8) & 15] for v in f]
        if "int" in self.dtype:
            return [float(v) for v in f] if has_zp else [float(v - 16 if v >= 8 else v) for v in f]
        return None

    def extra_repr(self):
        s = super().extra_repr()
        if self.use_optimum_format:
            s += ", use_optimum_format=True"
        return s


# the reference's class name for the non-Gaudi device class; code that imports it keeps working
INCWeightOnlyLinear = MI355XWeightOnlyLinear


def _classify_g_idx(g_idx, K, group_size):
    """(kind, order) of a per-element group index [K]: "contiguous" (arange(K) // gs_eff, gs_eff = K for group_size -1 or >= K: what a
    module without g_idx has), "permuted" (a permutation of whole groups: the stable argsort `order`, int64, restores the contiguous
    one) or "irregular" (anything else); order is None unless "permuted".  Pure torch on g_idx's device; each comparison is a sync."""
    gs_eff = K if (group_size == -1 or group_size >= K) else group_size
    g = g_idx.to(torch.int64)
    contiguous = torch.arange(K, device=g.device) // gs_eff
    if torch.equal(g, contiguous):
        return "contiguous", None
    order = torch.argsort(g, stable=True)
    if torch.equal(g[order], contiguous):
        return "permuted", order
    return "irregular", None


def _owner_call(owner, name, key, tensors, build):
    """The prepared call `key` of the per-owner cache `name` (a cache, not state: it dies with the owner module, copies and pickles of
    the module start without it), rebuilt through build() when any buffer it describes -- a g_idx among them: the plan then has new
    sorted words and a new order -- was replaced or written to."""
    cache = owner.__dict__.setdefault(name, {})
    call = cache.get(key)
    if call is None or not call.current(*tensors):
        if len(cache) >= 8:
            cache.clear()
        call = cache[key] = build()
    return call


def woq_linear_group(x, modules):
    """[m(x) for m in modules] for packed modules that multiply the SAME activation -- q / k / v of an attention block, gate / up of
    an MLP -- as ONE launch (inc_woq_gemm_multi) when x is a decode-sized batch (<= 64 rows).  Each module keeps its own buffers and
    state-dict keys (`MI355XWeightOnlyLinear` stays the single-module path).  act_order (HF desc_act) members join the launch while
    ACT_ORDER_FUSED_GATHER is on (inc_woq_gemm_multi_perm: every member gathers x through its own order inside the kernel; a member
    without a permutation takes the identity); with the switch off such groups are the single calls.

    A grouped result equals the single call's within output rounding, NOT bit for bit: the grouped launch always takes the streaming
    kernel with the steps per wave chosen from the strips of all members together, while a single call at M <= 4 on a small layer
    (N, K <= 4096) takes the no-split kernel and otherwise chooses from its own strips -- the fp32 summation order differs, so an
    output may move by one unit of the 16-bit type depending on eligibility (M <= 64 or not, the siblings, a declined batch).
    Members of one odd width (1, 2, 3, 5, 6, 7 bits) that all decode through inc_woq_gemv_anyw or its gathered form go out as ONE
    inc_woq_gemv_anyw_multi launch up to min(ODD_WIDTH_DECODE_MAX_M, 16) rows -- with act_order members up to ODD_WIDTH_GATHER_MAX_MN
    outputs of the widest member; there every output IS the single call's bit for bit (the K-slices depend on K and the width alone).
    Anything the batched launch does not cover (prefill-sized x, irregular g_idx plans, other widths, non-optimum layouts, a dtype
    other than bf16 / fp16, x on another device or of another width) is the plain list of single calls: the reference's forward
    per module (modules.py:594-610)."""
    mods = list(modules)
    m0 = mods[0]
    ok = (len(mods) >= 2 and x.dtype in (torch.bfloat16, torch.float16) and x.is_cuda and x.numel() > 0
          and all(isinstance(m, MI355XWeightOnlyLinear) and m.bits == m0.bits and m.in_features == m0.in_features and m.group_size == m0.group_size
                  for m in mods)
          and x.device == m0.qweight.device and x.shape[-1] == m0.in_features)
    anyw = ok and m0.bits in ops.GEMV_ANYW_BITS
    ok = ok and (anyw or m0.bits in (4, 8))
    members = [m._group_member() for m in mods] if ok else None
    if ok and all(mem is not None for mem in members):
        K = m0.in_features
        x2d = x.reshape(-1, K)
        max_m = min([ops.GEMV_ANYW_MAX_M] + [m.ODD_WIDTH_DECODE_MAX_M for m in mods]) if anyw else 64
        if anyw and any(mem[1] is not None for mem in members):  # (the gather inside the kernel: see the attribute)
            max_m = min(max_m, min(m.ODD_WIDTH_GATHER_MAX_MN for m in mods) // max(m.out_features for m in mods))
        if x2d.shape[0] <= max_m:
            if not x2d.is_contiguous():
                x2d = x2d.contiguous()
            parts = [mem[0] for mem in members]
            orders = [mem[1] for mem in members]
            if all(o is None for o in orders):
                orders = None
            # the prepared call lives on the group's first module
            cls = ops.WoqGemvAnywGroupCall if anyw else ops.WoqGemmGroupCall
            call = _owner_call(m0, "_group_calls", tuple(id(m) for m in mods[1:]) + (x.dtype,), (parts, orders),
                               lambda: cls(parts, K, m0.group_size, m0.bits, x.dtype, k_orders=orders))
            ys = call(x2d)
            if ys is not None:
                return [y.view(*x.shape[:-1], m.out_features) for y, m in zip(ys, mods)]
    return [m(x) for m in mods]


# gate / up of a dense gated MLP: True = woq_gated_pair forms silu(gate(x)) * up(x) inside the decode launch (inc_woq_gemm_gated),
# False = woq_linear_group + the activation + the product as torch kernels
GATED_FUSED = True


def woq_gated_pair(x, gate, up, act_fn=None):
    """act_fn(gate(x)) * up(x) -- the first half of a gated MLP (transformers' LlamaMLP.forward) -- in ONE launch for a decode-sized
    batch (inc_woq_gemm_gated, up to ops.WoqGatedCall.MAX_M rows): both products and the SiLU product, which is formed in fp32 from the
    two fp32 sums and rounded once.  The unfused form rounds three times (g, u, the product), so the two agree within output rounding,
    not bit for bit.  act_fn: None (SiLU) or a SiLU module.

    Fused when both members are MI355XWeightOnlyLinear, 4-bit, on the plain fused or (with ACT_ORDER_FUSED_GATHER) the act_order plan
    -- each member then gathers x through its own order --, without a bias, of equal shape and group size, x is bf16 / fp16 on the
    modules' device with x.shape[-1] == K, the rows are within the entry's limit, act_fn is None or SiLU and GATED_FUSED is on.
    Otherwise exactly act(g) * u with g, u = woq_linear_group(x, [gate, up]) and act = F.silu by default.  The prepared call is a
    cache on `gate` (not state: it dies with the module, copies start without it, a replaced buffer rebuilds it)."""
    cls = MI355XWeightOnlyLinear
    if (GATED_FUSED and (act_fn is None or is_silu(act_fn)) and isinstance(gate, cls) and isinstance(up, cls) and gate.bits == 4 and up.bits == 4
            and gate.bias is None and up.bias is None and gate.in_features == up.in_features and gate.out_features == up.out_features
            and gate.group_size == up.group_size and x.dtype in (torch.bfloat16, torch.float16) and x.is_cuda and x.numel() > 0
            and x.device == gate.qweight.device and x.shape[-1] == gate.in_features and x.numel() <= ops.WoqGatedCall.MAX_M * gate.in_features):
        mg, mu = gate._group_member(), up._group_member()
        if mg is not None and mu is not None:
            K = gate.in_features
            x2d = x.reshape(-1, K)
            if not x2d.is_contiguous():
                x2d = x2d.contiguous()
            orders = None if mg[1] is None and mu[1] is None else [mg[1], mu[1]]
            call = _owner_call(gate, "_gated_calls", (id(up), x.dtype), (mg[0], mu[0], orders),
                               lambda: ops.WoqGatedCall(mg[0], mu[0], K, gate.group_size, 4, x.dtype, k_orders=orders))
            h = call(x2d)
            if h is not None:
                return h.view(*x.shape[:-1], gate.out_features)
    g, u = woq_linear_group(x, [gate, up])
    return (torch.nn.functional.silu(g) if act_fn is None else act_fn(g)) * u


class MulLinear(torch.nn.Module):
    """Linear with a per-input-channel multiplier in front (AWQ scale that cannot be folded upstream,
    reference modules.py:907-949)."""

    def __init__(self, module, input_scale=None):
        super().__init__()
        if input_scale is None:
            input_scale = torch.empty(module.in_features)
        self.register_buffer("input_scale", input_scale)
        self.add_module("linear", module)

    @property
    def weight(self):
        return self.linear.weight

    @weight.setter
    def weight(self, weight):
        self.linear.weight = weight

    def forward(self, X):
        return self.linear(torch.mul(X, self.input_scale))

    def _update_linear(self):
        """Fold the multiplier into the weight: y = (x * input_scale) W'^T with W' = W / input_scale (reference :939-943)."""
        with torch.no_grad():
            self.linear.weight.div_(self.input_scale.view(1, -1).to(self.linear.weight.dtype))
        return self.linear

    def _recover_linear(self):
        """Undo `_update_linear` (reference :945-949)."""
        with torch.no_grad():
            self.linear.weight.mul_(self.input_scale.view(1, -1).to(self.linear.weight.dtype))
        return self.linear
