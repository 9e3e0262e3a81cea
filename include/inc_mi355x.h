/*
 * inc_mi355x.h -- C-ABI of libinc_mi355x.so: the MI355X (gfx950 / CDNA4) implementation of
 * intel/neural-compressor's weight-only-quant hot path.
 *
 * The reference (INC 3.9) is 100 % Python and has NO FFI for this path; each entry point below
 * replaces the torch/numpy/numba arithmetic of the cited reference function (file:line relative to
 * /root/reference).  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types.  All pointers are DEVICE pointers (HBM) unless noted.
 *   - the caller owns every buffer (torch-allocated, passed as tensor.data_ptr()); the library
 *     allocates nothing persistent and keeps no state -> thread-safe.
 *   - every call is asynchronous w.r.t. the host and ordered on `stream` (a hipStream_t passed as
 *     void*; NULL = the default stream).
 *   - return value: INC_OK (0) or a negative INC_ERR_* code; the C side never throws.
 *   - tensors are dense row-major; "[N,K]" means N rows of K contiguous elements.
 *   - dtype codes: INC_F32 / INC_F16 / INC_BF16 for floating tensors.
 */
#ifndef INC_MI355X_H_
#define INC_MI355X_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INC_OK 0
#define INC_ERR_BAD_ARG (-1)     /* null pointer / non-positive size / inconsistent shape          */
#define INC_ERR_UNSUPPORTED (-2) /* valid request this build does not implement (e.g. bits = 9)    */
#define INC_ERR_LAUNCH (-3)      /* hipGetLastError() != hipSuccess after the launch               */
#define INC_ERR_WORKSPACE (-4)   /* workspace too small (see *_workspace_bytes)                    */

#define INC_F32 0
#define INC_F16 1
#define INC_BF16 2

#define INC_SCHEME_ASYM 0
#define INC_SCHEME_SYM 1

typedef void* inc_stream_t; /* hipStream_t */

/* ---- library info ------------------------------------------------------------------------- */
int inc_abi_version(void);                 /* bumps on any signature change                      */
const char* inc_error_string(int code);    /* static string for an INC_ERR_* code                */
const char* inc_target_arch(void);         /* "gfx950"                                           */

/* The library keeps no mutable process-global state: every call is a function of its arguments and the stream.
 * (The A/B switch of tools/kbench, inc_debug_set_small_tiles, exists only in the harness build
 * tools/libinc_mi355x_kbench.so, compiled from the same sources with -DINC_KBENCH.)                              */

/* ---- K1/K2: bit packing ------------------------------------------------------------------- *
 * inc_pack_rows  == INCWeightOnlyLinear.pack_tensor   (weight_only/modules.py:580, :445, :546,
 *                   numba packers torch/utils/bit_packer.py:35-278):
 *     packed[r, j] = OR_e ((raw[r, j*n_pack + e] & (2^bits-1)) << (bits*e)),  n_pack = cbits/bits
 *   raw: int32 [rows, cols]; packed: [rows, ceil(cols/n_pack)] words of `cbits` bits.
 *   bits in 1..8 (every width the reference's configs tune, torch/quantization/config.py:211; 3 / 5 / 6 / 7 leave the
 *   word's high bits unused, modules.py:231); cbits in {8,16,32,64}, cbits >= bits.
 * inc_unpack_rows == INCWeightOnlyLinear.unpack_tensor (modules.py:587, :468, :558):
 *     out[r, j*n_pack+e] = (packed[r,j] << (cbits-bits*(e+1))) >>arith (cbits-bits), then & mask
 *     iff mask_sign != 0 (the reference masks iff the module has `qzeros`); out: int16.
 */
int inc_pack_rows(const int32_t* raw, void* packed, int64_t rows, int64_t cols, int bits, int cbits,
                  inc_stream_t stream);
int inc_unpack_rows(const void* packed, int16_t* out, int64_t rows, int64_t packed_cols, int bits,
                    int cbits, int mask_sign, inc_stream_t stream);

/* ---- K1 fused: pack into the "optimum" (HF/AutoGPTQ) layout ------------------------------- *
 * == INCWeightOnlyLinear.pack with use_optimum_format=True (modules.py:321-375).
 *   int_weight [N,K] (int32 when in_bytes == 4, int8 when in_bytes == 1); `shift` is added to every
 *     value before masking (reference: +2^(bits-1) when zp is None, modules.py:329-334).
 *   scales   [N,G] fp32  -> scales_out [G,N] fp16          (modules.py:346,372)
 *   zp       [N,G] int32 or NULL.  NULL => every zero point is 2^(bits-1) (sym, modules.py:334).
 *            qzeros stores zp-1 (modules.py:364) packed along N: qzeros [G, ceil(N/n_pack)] int32.
 *            (`shift` only moves the weights: pass signed ints with shift=2^(bits-1), or already
 *            offset codes 0..2^bits-1 with shift=0 -- the GPTQ kernel emits the latter.)
 *   qweight  [ceil(K/n_pack), N] int32: nibble e of qweight[r, n] = int_weight[n, r*n_pack+e]+shift.
 */
int inc_woq_pack(const void* int_weight, int in_bytes, const float* scales, const int32_t* zp,
                 int32_t* qweight, int32_t* qzeros, uint16_t* scales_out, int64_t N, int64_t K,
                 int64_t G, int bits, int shift, inc_stream_t stream);

/* ---- K2 fused: unpack the optimum layout -------------------------------------------------- *
 * == INCWeightOnlyLinear.unpack (modules.py:377-411): int_weight [N,K] int16 (0..2^bits-1),
 *   zp [N,G] int16 = stored+1, values > 2^bits-1 wrap to 0 (modules.py:407-410).
 *   Either output pointer may be NULL to skip it.  scales_ng (with int_weight; NULL = off): the module's scales [G,N] fp16
 *   (scales_gn) written as [N,G] in the same launch -- unpack returns `scales.T.contiguous()` (modules.py:382).
 */
int inc_woq_unpack(const int32_t* qweight, const int32_t* qzeros, int16_t* int_weight, int16_t* zp,
                   int64_t N, int64_t K, int64_t G, int bits, const uint16_t* scales_gn, uint16_t* scales_ng,
                   inc_stream_t stream);

/* ---- K3: recover / dequantize ------------------------------------------------------------- *
 * == INCWeightOnlyLinear.recover (modules.py:413-443):
 *     W[n,k] = int8(q[n,k] - zp[n,g(k)]) * scales[n,g(k)],  g(k) = g_idx ? g_idx[k] : k / group_size
 *   computed exactly in fp32 then rounded ONCE to out_dtype (fp16 reproduces the reference bit for
 *   bit).  Optimum layout in: qweight [ceil(K/n_pack),N], scales [G,N] fp16, qzeros [G,ceil(N/np)].
 *   out [N,K] of out_dtype.
 */
int inc_woq_dequant(const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros,
                    const int32_t* g_idx, void* out, int out_dtype, int64_t N, int64_t K, int64_t G,
                    int group_size, int bits, inc_stream_t stream);

/* same arithmetic from already-unpacked integers (non-optimum formats, modules.py:270-314):
 *   int_weight [N,K] int16, scales [N,G] of scale_dtype, zp [N,G] int16 or NULL.               */
int inc_dequant_ints(const int16_t* int_weight, const void* scales, int scale_dtype,
                     const int16_t* zp, const int32_t* g_idx, void* out, int out_dtype, int64_t N,
                     int64_t K, int64_t G, int group_size, inc_stream_t stream);

/* ---- K4: fused INT4/INT8 unpack + group dequant + GEMM ------------------------------------- *
 * == INCWeightOnlyLinear.forward (modules.py:594-610) == F.linear(x, recover(), bias), without
 *   ever materialising the dense weight.  x [M,K] and y [M,N] of dtype `xdtype` (INC_BF16 or
 *   INC_F16), fp32 accumulate; weights dequantised to `xdtype` in registers.
 *   bias [N] of `xdtype` or NULL.  bits in 1..8: 4 and 8 take the fast kernels below; 1 / 2 / 3 / 5 / 6 / 7 (n_pack = 32 / bits
 *   fields per word, modules.py:231) take the 128x128 tile kernel's per-element form (any group_size, any g_idx).
 *   g_idx [K] int32 or NULL: the group of every k
 *   (act_order / HF desc_act checkpoints, modules.py:341-344, 427-431); with a g_idx the general 128x128 tile
 *   kernel (or the M <= 16 split-K kernel) looks scale / zero up per element.  A g_idx that permutes whole groups
 *   is faster through a K-sorted copy of the words and a gather of x, which MI355XWeightOnlyLinear does once per module.
 *   The library picks the kernel itself from (M, N, K, group_size, bits, g_idx) and the alignment of x / y / bias; inc_woq_gemm_route
 *   below reports the choice (INC_WOQ_ROUTE_*).  In short, for 4 / 8 bits without g_idx and a power-of-two group_size >= 32 (or one
 *   group): M <= 64 streams the packed weights once (GEMV16 / STREAM_*), 64 < M <= 1024 with few 256x256 tiles takes the strip
 *   kernels (STRIP8 / STRIP), everything larger a 256-row tile kernel (D2R, 3A2B_*, BIG); whatever those do not take (g_idx, other
 *   group sizes, K % 32 != 0, N < 64 or N % 4 != 0, unaligned x) runs on the general 128x128 tile kernel (TILE, M > 16) or the
 *   generic split-K kernel (SMALL, M <= 16).
 *   `workspace` (inc_woq_gemm_workspace_bytes bytes; may be 0).  STRIP / D2R / 3A2B_* with too few tiles to fill the chip: fp32
 *   split-K slabs, summed in a fixed order (by the last-arriving workgroup, or by a second small kernel); without a workspace the
 *   call still works, single pass.  STREAM_* and SMALL need it (INC_ERR_WORKSPACE without, nothing launched).
 *   Its first 16 KiB hold the per-strip arrival counters of the in-kernel split-K reductions and MUST BE
 *   ZERO when the workspace is first used (the last-arriving workgroup re-arms them, so a workspace that
 *   is only ever handed to this function stays valid); the fp32 partials follow.  One workspace must not
 *   be shared by calls that may run concurrently (different streams).
 */
int64_t inc_woq_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int inc_woq_gemm(const void* x, int xdtype, const int32_t* qweight, const uint16_t* scales,
                 const int32_t* qzeros, const int32_t* g_idx, const void* bias, void* y, int64_t M,
                 int64_t N, int64_t K, int64_t G, int group_size, int bits, void* workspace,
                 int64_t workspace_bytes, inc_stream_t stream);

/* Which kernel inc_woq_gemm launches for a call: the dispatcher's own decision (inc_woq_gemm branches on the result of the same
 * function), computed on the host without touching the GPU or dereferencing a pointer -- of x, y, bias and workspace only the
 * alignment / being NULL is used.  Returns an INC_WOQ_ROUTE_* value, or a negative INC_ERR_* code where inc_woq_gemm would reject
 * the shape.  Out-parameters (each may be NULL):
 *   splitk       K-slices actually used with the given workspace (1 = single pass).  The tile-shaped routes (STRIP, D2R, 3A2B_*)
 *                fall back to 1 when the workspace is NULL or smaller than *workspace_need; STREAM_* and SMALL cannot, and
 *                inc_woq_gemm returns INC_ERR_WORKSPACE there (compare *workspace_need with workspace_bytes).
 *   row_blocks   STREAM_*: 16-row blocks per workgroup (1 / 2 / 4); 0 elsewhere.
 *   steps        STREAM_*: K-steps of 32 per wave (4 / 8); D2R / 3A2B_*: K-steps of 64 per slab; 0 elsewhere.
 *   y_vec_ok     D2R: bit 0 = 8-byte stores, bit 1 = 16-byte stores; 3A2B_* / BIG: 0 / 1; -1 elsewhere.
 *   x_vec_ok     TILE / TILE_ANYW: 16-byte loads of x possible (0 / 1); -1 elsewhere.
 *   workspace_need  bytes of workspace the route uses when it is given enough (0 = none).                                    */
#define INC_WOQ_ROUTE_TILE_ANYW 1 /* 128x128 tile kernel, per-element form: 1 / 2 / 3 / 5 / 6 / 7 bits                   */
#define INC_WOQ_ROUTE_STRIP8 2    /* 128-row four-wave strip kernel (gemm_strip8.hip), no K-slices                       */
#define INC_WOQ_ROUTE_STRIP 3     /* 64-row strip kernel, <= 4 K-slices handed over in the kernel                        */
#define INC_WOQ_ROUTE_3A2B_W8 4   /* 256x256 3A2B tile kernel, 8-bit words (+ slab reduce)                               */
#define INC_WOQ_ROUTE_D2R 5       /* 256x256 direct-to-register kernel (gemm_d2r.hip) (+ slab reduce)                    */
#define INC_WOQ_ROUTE_3A2B_W4 6   /* 256x256 3A2B tile kernel, 4-bit words (+ slab reduce)                               */
#define INC_WOQ_ROUTE_BIG 7       /* the older 256x256 kernel (K % 128 == 64)                                            */
#define INC_WOQ_ROUTE_TILE 8      /* general 128x128 tile kernel, 4 / 8 bits, M > 16                                     */
#define INC_WOQ_ROUTE_GEMV16 9    /* decode kernel without split-K (M <= 4)                                              */
#define INC_WOQ_ROUTE_STREAM_W4 10 /* streaming decode kernel, 4-bit                                                     */
#define INC_WOQ_ROUTE_STREAM_W8 11 /* streaming decode kernel, 8-bit                                                     */
#define INC_WOQ_ROUTE_SMALL 12    /* generic split-K kernel + reduce, M <= 16                                            */
int inc_woq_gemm_route(int64_t M, int64_t N, int64_t K, int group_size, int bits, int xdtype, int has_g_idx, const void* x,
                       const void* y, const void* bias, const void* workspace, int64_t workspace_bytes, int* splitk,
                       int* row_blocks, int* steps, int* y_vec_ok, int* x_vec_ok, int64_t* workspace_need);

/* act_order (HF desc_act) decode in ONE launch: y = x[:, k_order] . W_sorted^T + bias -- INCWeightOnlyLinear.forward (modules.py:594-610)
 * on a module whose g_idx permutes whole groups (modules.py:427-431 looks the group up per element).  `qweight` is the packed weight
 * with its K axis sorted by group (row k of the sorted fields is row k_order[k] of the module's), so scales / qzeros are the module's own
 * and the groups are contiguous; k_order [K] int32, 16-byte aligned, is that order.  The activations are gathered inside the decode
 * kernels (x needs only 2-byte alignment); every entry of k_order is clamped to [0, K-1] before it is used, so no array can send a
 * read outside x.  The result is bit-identical to inc_woq_gemm(x.index_select(1, k_order), qweight, ..., g_idx = NULL) with the
 * same workspace size: the same kernel body, the same plan.
 *   Planned as inc_woq_gemm_route plans (M, N, K, group_size, bits, no g_idx) for a 16-byte aligned x; launched only on the routes
 *   GEMV16, STREAM_W4 and STREAM_W8.  INC_ERR_UNSUPPORTED (nothing launched) on every other route -- every M > 64 among them --
 *   and for a k_order that is not 16-byte aligned: gather x and call inc_woq_gemm then.
 *   `workspace`: inc_woq_gemm_workspace_bytes(M, N, K) bytes, with inc_woq_gemm's rules (zeroed arrival counters in the first
 *   16 KiB; INC_ERR_WORKSPACE where a STREAM_* route gets too little).                                                        */
int inc_woq_gemm_perm(const void* x, int xdtype, const int32_t* k_order, const int32_t* qweight, const uint16_t* scales,
                      const int32_t* qzeros, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int64_t G,
                      int group_size, int bits, void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* Several packed modules that multiply the SAME x, in ONE launch -- the decode path of q / k / v (and of gate / up): n calls of
 * INCWeightOnlyLinear.forward (modules.py:594-610) on one activation, which the reference issues one F.linear after the other.
 *   x [M,K] of `xdtype`, M <= 64; module i: qweight[i] [K/8,N[i]], scales[i] [G,N[i]] fp16, qzeros[i] [G,ceil(N[i]/8)], bias[i] [N[i]] of
 *   `xdtype` or NULL (bias itself may be NULL), y[i] [M,N[i]] of `xdtype`; K, group_size and bits (4, or 8 with M <= 16) are common, no g_idx.
 *   The arrays of pointers / sizes live in HOST memory (like inc_gptq_hessian_accum_multi); the state dict is untouched.
 *   Every 64-column strip is computed exactly as inc_woq_gemm's streaming kernel computes it, so the launch is bit-identical to
 *   inc_woq_gemm on the N-concatenated module (deterministic: fixed-order split-K sum).  INC_ERR_UNSUPPORTED (nothing launched)
 *   when the batch is not eligible (n < 2 or > 8, M > 64, bits other than 4 / 8, a group size that is not a power of two >= 32 or one
 *   group, N[i] < 64 or N[i] % 4 != 0, K % 32 != 0, unaligned x, or M > 32 on more than 24 Mi weights, where inc_woq_gemm's
 *   strip kernel is the faster form): call inc_woq_gemm per module then.
 *   `workspace`: inc_woq_gemm_multi_workspace_bytes bytes; its first 16 KiB are arrival counters with the rules of inc_woq_gemm's. */
int64_t inc_woq_gemm_multi_workspace_bytes(int n, int64_t M, const int64_t* N, int64_t K);
int inc_woq_gemm_multi(int n, const void* x, int xdtype, const int32_t* const* qweight, const uint16_t* const* scales,
                       const int32_t* const* qzeros, const void* const* bias, void* const* y, int64_t M, const int64_t* N,
                       int64_t K, int group_size, int bits, void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* inc_woq_gemm_multi for act_order (HF desc_act) members: y[i] = x[:, k_order[i]] . W_sorted_i^T + bias_i, all members in ONE launch --
 * n calls of INCWeightOnlyLinear.forward (modules.py:594-610) whose groups are looked up per element (modules.py:427-431).  The arguments
 * are inc_woq_gemm_multi's plus `k_order`, a HOST array of n device pointers: k_order[i] [K] int32, 16-byte aligned, never NULL, and
 * qweight[i] member i's K-sorted words, as for inc_woq_gemm_perm.  A member without a permutation takes the identity (0 .. K-1).  Every
 * entry of an order is clamped to [0, K-1] before it is used; x needs only 2-byte alignment.
 *   Contract: y[i] is bit-identical to output i of inc_woq_gemm_multi called with the same n, N[], K, workspace size and
 *   x.index_select(1, k_order[i]) in place of x -- the same plan, the same rung of the same body, the same MFMAs in the same order.
 *   INC_ERR_UNSUPPORTED (nothing launched) wherever inc_woq_gemm_multi returns it (an unaligned x excepted: x is read 2 bytes at a
 *   time here), for M * K >= 2^31 and for an order that is not 16-byte aligned; INC_ERR_BAD_ARG for a NULL k_order or k_order[i].
 *   `workspace`: inc_woq_gemm_multi_workspace_bytes bytes, with inc_woq_gemm_multi's rules.                                      */
int inc_woq_gemm_multi_perm(int n, const void* x, int xdtype, const int32_t* const* k_order, const int32_t* const* qweight,
                            const uint16_t* const* scales, const int32_t* const* qzeros, const void* const* bias, void* const* y, int64_t M,
                            const int64_t* N, int64_t K, int group_size, int bits, void* workspace, int64_t workspace_bytes,
                            inc_stream_t stream);

/* gate_proj / up_proj of a dense gated MLP with the SiLU product in the SAME launch: h = act_fn(gate_proj(x)) * up_proj(x), the first half
 * of transformers' LlamaMLP.forward (models/llama/modeling_llama.py: `down_proj(act_fn(gate_proj(x)) * up_proj(x))`; also Mistral /
 * Qwen2 / Qwen3), whose two products are INCWeightOnlyLinear.forward (modules.py:594-610) and whose activation and product are two more
 * torch kernels on 16-bit copies of g and u.  Here
 *     h[m, j] = rx( g / (1 + expf(-g)) * u ),   g = x[m] . Wg[j],  u = x[m] . Wu[j]
 *   in fp32 with ONE rounding rx to xdtype (the expression of inc_woq_moe_gemm's mode 0).  g and u are the fixed-order fp32 sums
 *   inc_woq_gemm_multi forms for the pair (N, N) before it rounds them: deterministic, repeated calls are bit-identical.
 *   x [M,K] of `xdtype` (INC_BF16 / INC_F16), M <= 16; gate and up: qweight [K/8,N], scales [G,N] fp16, qzeros [G,ceil(N/8)], the same
 *   N, K and group_size, no bias; h [M,N] of `xdtype`; act: 0 = SiLU.  k_order_gate / k_order_up: both NULL, or both given ([K] int32,
 *   16-byte aligned; INC_ERR_BAD_ARG for one without the other) -- then the words are the K-sorted ones and each member gathers x through
 *   its OWN order as inc_woq_gemm_perm does (entries clamped to [0, K-1], x 2-byte aligned, M * K < 2^31).
 *   INC_ERR_UNSUPPORTED (nothing launched): bits other than 4, act other than 0, M > 16, whatever inc_woq_gemm_multi declines for
 *   n = 2 and N[] = {N, N}, an unaligned x without orders, a misaligned order.
 *   `workspace`: inc_woq_gemm_gated_workspace_bytes bytes (0 for a non-positive size; INC_ERR_WORKSPACE for less than the launch needs);
 *   its first 16 KiB are arrival counters with the rules of inc_woq_gemm's (zero on first use, re-armed by the kernel), so one
 *   (device, stream) workspace serves this entry and the other inc_woq_gemm* entries in turn.                                       */
int64_t inc_woq_gemm_gated_workspace_bytes(int64_t M, int64_t N, int64_t K);
int inc_woq_gemm_gated(const void* x, int xdtype, const int32_t* k_order_gate, const int32_t* k_order_up, const int32_t* gate_qweight,
                       const uint16_t* gate_scales, const int32_t* gate_qzeros, const int32_t* up_qweight, const uint16_t* up_scales,
                       const int32_t* up_qzeros, void* h, int64_t M, int64_t N, int64_t K, int group_size, int bits, int act,
                       void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* ---- K4f: decode GEMV of the 1 / 2 / 3 / 5 / 6 / 7-bit optimum-layout modules -------------- *
 * == INCWeightOnlyLinear.forward (modules.py:594-610) for up to 16 rows of x: y = x . W^T + bias with W[n,k] = rn16(int8(q - zp) * scale)
 *   rounded once to xdtype (bit-identical to inc_woq_dequant), fp32 accumulation, the dense weight never materialised
 *   (csrc/gemm_anyw.hip).  inc_woq_gemm keeps INC_WOQ_ROUTE_TILE_ANYW for these widths; this entry is the decode route.
 *     qweight [ceil(K / n_pack), N] int32, n_pack = 32 / bits: word w of column n holds k = n_pack * w .. in fields of `bits` bits from bit 0
 *       (fields at k >= K in the last word are padding: they contribute nothing and x is never read at or beyond column K);
 *     scales [G, N] fp16; qzeros [G, ceil(N / n_pack)] int32 packed along N, stored field = zp - 1 (z = field + 1, above 2^bits - 1 -> 0);
 *     groups are contiguous, looked up per field (g = k / group_size: a word may straddle two groups); bias [N] of xdtype or NULL.
 *   INC_ERR_UNSUPPORTED (nothing launched) unless bits is 1, 2, 3, 5, 6 or 7; xdtype INC_BF16 / INC_F16; 1 <= M <= 16; K % 32 == 0;
 *     N % 4 == 0, N >= 64; group_size a power of two >= 32 or one group per row (-1 or >= K; a ragged last group is allowed:
 *     G = ceil(K / group_size)); x, y, qweight 16-byte and scales 8-byte aligned.  INC_ERR_BAD_ARG for a G that does not match.
 *   Split-K over inc_woq_gemv_anyw_slices(M, N, K, bits) K-slices (0 for a shape the entry declines) with a fixed-order sum:
 *     repeated calls are bit-identical.  `workspace`: inc_woq_gemv_anyw_workspace_bytes bytes (0 where one slice suffices: workspace may
 *     be NULL then; INC_ERR_WORKSPACE for less than a split needs); its first 16 KiB are arrival counters with the rules of inc_woq_gemm's
 *     (zero on first use, re-armed by the kernel), so one (device, stream) workspace serves this and the inc_woq_gemm* entries in turn. */
int inc_woq_gemv_anyw_slices(int64_t M, int64_t N, int64_t K, int bits);
int64_t inc_woq_gemv_anyw_workspace_bytes(int64_t M, int64_t N, int64_t K, int bits);
int inc_woq_gemv_anyw(const void* x, int xdtype, const int32_t* qweight, const uint16_t* scales, const int32_t* qzeros, const void* bias,
                      void* y, int64_t M, int64_t N, int64_t K, int64_t G, int group_size, int bits, void* workspace,
                      int64_t workspace_bytes, inc_stream_t stream);

/* K4f, gathered: == INCWeightOnlyLinear.forward (modules.py:594-610) of an act_order module of these widths, whose g_idx (modules.py:427-431)
 *   is a permutation of whole groups: y = x[:, k_order] . W_sorted^T + bias in ONE launch.  `qweight` holds the packed fields with the K
 *   axis sorted by group (k_order = stable argsort of g_idx; field j of the sorted words is field k_order[j] of the module's), `k_order`
 *   [K] int32, 16-byte aligned; the kernel gathers the activations itself, entries outside [0, K-1] are clamped.  Bit-identical to
 *   inc_woq_gemv_anyw on x.index_select(1, k_order): the same MFMAs in the same order.  x needs 2-byte alignment only.
 *   INC_ERR_UNSUPPORTED (nothing launched): whatever inc_woq_gemv_anyw declines except an unaligned x; M * K >= 2^31 (x is addressed by
 *   32-bit byte offsets); a misaligned k_order.  Slices, workspace and counters are inc_woq_gemv_anyw's.                              */
int inc_woq_gemv_anyw_perm(const void* x, int xdtype, const int32_t* k_order, const int32_t* qweight, const uint16_t* scales,
                           const int32_t* qzeros, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int64_t G,
                           int group_size, int bits, void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* K4f, batched: == INCWeightOnlyLinear.forward (modules.py:594-610) of n modules of ONE of these widths that multiply the same x (q / k / v,
 *   gate / up; act_order members: modules.py:427-431) in ONE launch: y[i] = x . W_i^T + bias[i], or x[:, k_order[i]] . W_sorted_i^T + bias[i].
 *   2 <= n <= 8; qweight, scales, qzeros, bias, y, k_order and N are arrays of n entries in HOST memory (bias may be NULL, or hold NULL
 *   entries); K, group_size and bits are common, every member a shape inc_woq_gemv_anyw takes (64 <= N[i] <= 2^18, N[i] % 4 == 0,
 *   qweight[i] / y[i] 16-byte and scales[i] 8-byte aligned), all members' 64-column strips together within the 16 KiB counter block.
 *   `k_order`: NULL (no member gathers; x 16-byte aligned) or n non-NULL 16-byte aligned orders (x 2-byte aligned, M * K < 2^31; a
 *   member without a permutation gets the identity from the caller; a NULL entry is INC_ERR_BAD_ARG).  Everything else the single
 *   entries decline is INC_ERR_UNSUPPORTED here, nothing launched.
 *   Output i is bit-identical to inc_woq_gemv_anyw / inc_woq_gemv_anyw_perm on member i: the K-slices depend on K and bits alone.
 *   `workspace`: inc_woq_gemv_anyw_multi_workspace_bytes = 0 for one slice (or a batch the entry declines), else
 *   16384 + slices * M * sum(N) * 4 bytes: one arrival counter per strip of the batch, then the members' fp32 slabs [slice][M][N[i]] one
 *   after the other.  Counter rules as above (zero on first use, re-armed by the kernel, one workspace per (device, stream)).      */
int64_t inc_woq_gemv_anyw_multi_workspace_bytes(int n, int64_t M, const int64_t* N, int64_t K, int bits);
int inc_woq_gemv_anyw_multi(int n, const void* x, int xdtype, const int32_t* const* k_order, const int32_t* const* qweight,
                            const uint16_t* const* scales, const int32_t* const* qzeros, const void* const* bias, void* const* y,
                            int64_t M, const int64_t* N, int64_t K, int group_size, int bits,
                            void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* ---- K4d: fused 4-bit code-book / row-packed integer dequant + GEMM ------------------------ *
 * == INCWeightOnlyLinear.forward (modules.py:594-610) for the layouts that are not the optimum one: F.linear(x, recover(x.dtype), bias)
 *   with recover (modules.py:413-443) done in registers, the dense weight never materialised.  NF4 / FP4 code books and integer
 *   modules packed with use_optimum_format=False, compression_dim = 1, bits = 4:
 *     qweight [N, row_bytes] bytes (any of the int8 / 16 / 32 / 64 containers of pack_rows: field k of row n is the low nibble of byte
 *       n * row_bytes + k/2 for even k, the high one for odd k);  row_bytes >= K/2, a multiple of 16
 *     table16 [16] fp32 in HOST memory, indexed by the field f: LUT[(f + 8) & 15] for a code book, f sign-extended for sym
 *       integers, f for asym integers
 *     scales [N,G] of scale_dtype (fp32 / fp16 / bf16);  qzeros NULL or [N, zrow_bytes] bytes with the 4-bit zero point of group g
 *       at byte g/2 (same nibble order)
 *     W[n,k] = rx( rs( (table16[f] - zp[n,g]) * scales[n,g] ) ), g = k / group_size, in fp32; rs rounds to scale_dtype when
 *       `scale_round` is set (integers: inc_dequant_ints's rule; with fp32 scales and an fp16 xdtype that rule rounds the exact
 *       product once to fp16) and is the identity otherwise (code books: the product stays fp32); rx rounds to xdtype.  So
 *       W == recover(dtype=xdtype) bit for bit.  The fused route serves up to 256 rows of x (MI355XWeightOnlyLinear.LUT_MAX_M).
 *   x [M,K], y [M,N] and bias [N] (or NULL) of `xdtype` (INC_BF16 / INC_F16), fp32 accumulate in a fixed order: repeated calls are
 *   bit-identical.  INC_ERR_UNSUPPORTED (nothing launched) unless K % 32 == 0, group_size a multiple of 32 or one group
 *   (-1 / >= K), x and qweight 16-byte aligned.
 *   `workspace` (inc_woq_gemm_lut_workspace_bytes bytes; 0 = none needed): its first 16 KiB are split-K arrival counters that
 *   MUST BE ZERO when the workspace is first used (the kernel re-arms them, as inc_woq_gemm's), the fp32 partials follow.  One
 *   workspace must not be shared by calls that may run concurrently (different streams).                                   */
int64_t inc_woq_gemm_lut_workspace_bytes(int64_t M, int64_t N, int64_t K);
int inc_woq_gemm_lut(const void* x, int xdtype, const uint8_t* qweight, int64_t row_bytes, const float* table16, const void* scales,
                     int scale_dtype, int scale_round, const uint8_t* qzeros, int64_t zrow_bytes, const void* bias, void* y, int64_t M,
                     int64_t N, int64_t K, int64_t G, int group_size, void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* ---- K4e: weight-only INT4 fused MoE experts ------------------------------------------------- *
 * == transformers' MixtralExperts.forward (also Qwen2-MoE / Qwen3-MoE / OLMoE experts): for every expert that was hit, gather its
 *   tokens, act_fn(x Wg^T) * (x Wu^T), times Wd^T, times the routing weight, index_add_ into the output.  Four launches, no host wait:
 *   inc_moe_route -> inc_woq_moe_gemm(mode 0) -> inc_woq_moe_gemm(mode 1) -> inc_moe_combine, all on `stream`.
 *   S = T * top_k slots, slot t*k+s = token t, choice s.  E <= 512, S <= 2^22.
 *
 *   inc_moe_route: top_k_index [T, top_k] int32 / int64 (index_bytes 4 / 8) -> `route` (inc_moe_route_bytes bytes, int32):
 *     [0] number of 64-row tiles, then offsets [E+1] (the slots of expert e are positions offsets[e] .. offsets[e+1]-1 of the sorted
 *     order; offsets[E] = slots with an id in 0..E-1, other ids contribute nothing), order [S] (sorted position -> slot; ascending slot
 *     inside an expert), pos [S] (slot -> sorted position), tiles [2 * (ceil(S/64) + min(E, S))] (expert, first position).
 *   inc_woq_moe_gemm: per-expert optimum layout stacked on the expert axis -- qweight [E, K/8, N] int32, scales [E, G, N] fp16,
 *     qzeros [E, G, N/8] int32 (slice e == MI355XWeightOnlyLinear's buffers for expert e) -- dequantised as inc_woq_dequant (the weight
 *     equals recover(xdtype) bit for bit), fp32 accumulate in a fixed order (repeated calls are bit-identical):
 *       mode 0 (gate_up, N = 2I): a = x [T, K]; out [S, I] xdtype, out[p, j] = silu(g) * u, g / u = row order[p]/top_k of x times
 *              weight rows j / I+j of the expert of position p
 *       mode 1 (down): a = [S, K] in sorted order (mode 0's output); out [S, N] fp32 = routing_weights[order[p]] * (a[p] . W[n])
 *              (routing_weights [T, top_k] of wdtype INC_F32 / INC_F16 / INC_BF16)
 *       mode 2 (plain): a = x [T, K]; out [S, N] fp32 = x[order[p]/top_k] . W[n]
 *     INC_ERR_UNSUPPORTED (nothing launched) unless xdtype is INC_BF16 / INC_F16, K % 32 == 0, N % 8 == 0, group_size a power of two
 *     >= 32 dividing K or one group (-1 / >= K), a / qweight / out 16-byte and scales 8-byte aligned.
 *     `workspace` (inc_woq_moe_gemm_workspace_bytes; 0 = none needed, also for N % 8 != 0 or K % 32 != 0, which the GEMM rejects): its
 *     first 4 KiB are split-K arrival counters, which MUST BE ZERO when the workspace is first used (the kernel re-arms them), then
 *     fp32 partials.  One workspace of the largest size serves every call shape and both modes in stream order; calls that may run
 *     concurrently need their own.
 *   inc_moe_combine: out [T, H] xdtype, out[t] = sum over s = 0 .. top_k-1 of y[pos[t*k+s]] (y = mode 1's output) in fp32, one rounding. */
int64_t inc_moe_route_bytes(int64_t T, int top_k, int64_t E);
int inc_moe_route(const void* top_k_index, int index_bytes, int64_t T, int top_k, int64_t E, int32_t* route, int64_t route_bytes,
                  inc_stream_t stream);
int64_t inc_woq_moe_gemm_workspace_bytes(int mode, int64_t T, int top_k, int64_t E, int64_t N, int64_t K);
int inc_woq_moe_gemm(int mode, const void* a, int xdtype, const int32_t* route, const int32_t* qweight, const uint16_t* scales,
                     const int32_t* qzeros, const void* routing_weights, int wdtype, void* out, int64_t T, int top_k, int64_t E, int64_t N,
                     int64_t K, int64_t G, int group_size, void* workspace, int64_t workspace_bytes, inc_stream_t stream);
int inc_moe_combine(const float* y, const int32_t* route, void* out, int xdtype, int64_t T, int top_k, int64_t E, int64_t H,
                    inc_stream_t stream);

/* ---- K7: group-wise round-to-nearest quantisation ------------------------------------------ *
 * == quant_tensor / qdq_weight_sym / qdq_weight_asym (weight_only/utility.py:272-436, :199, :162).
 *   w [N,K] of `wdtype`, quantised per row in groups of `group_size` along K (tail group = the
 *   remainder, utility.py:334-376).  scheme INC_SCHEME_SYM / _ASYM, quantile, full_range as the
 *   reference.  Arithmetic is done in `wdtype` precision exactly like the reference's torch ops
 *   (every intermediate rounded to wdtype; fp32 for INC_F32).
 *   Outputs (any may be NULL):
 *     qdq_out   [N,K] wdtype : fake-quantised weight (may alias w -> the reference's in-place mode)
 *     int_out   [N,K] int32  : integer codes (sym: -2^(b-1)..2^(b-1)-1, asym: 0..2^b-1)
 *     scale_out [N,G] fp32, zp_out [N,G] fp32 (asym only; ignored for sym)
 */
int inc_groupwise_quant(const void* w, int wdtype, void* qdq_out, int32_t* int_out, float* scale_out,
                        float* zp_out, int64_t N, int64_t K, int group_size, int bits, int scheme,
                        float quantile, int full_range, inc_stream_t stream);

/* Group-wise code-book quantisation == quantize_4bit (utility.py:112-149; the NF4 / FP4 branch of quant_tensor :246-265):
 *   scale[n,g] = max|w| * quantile / max(values);  w / scale -> nearest entry by the midpoint intervals of the reference.
 *   values [n_entries] ascending fp32 code book and codes [n_entries] (the integers written to int_out, INT_MAPPING) are HOST
 *   arrays read before the call returns.  Outputs (any may be NULL): qdq_out [N,K] wdtype (may alias w), int_out [N,K] int32,
 *   scale_out [N,G] fp32.                                                                                          */
int inc_codebook_quant(const void* w, int wdtype, void* qdq_out, int32_t* int_out, float* scale_out, int64_t N,
                       int64_t K, int group_size, const float* values, const int32_t* codes, int n_entries,
                       float quantile, inc_stream_t stream);

/* The same with the caller's scales: quantize_4bit(tensor, scale=...) (utility.py:127-128: `scale = kwargs["scale"]`, the
 * tensor is divided by it instead of by its own max).  scale_in [N,G] fp32 (device; must not alias scale_out); NULL = compute
 * the scales (== inc_codebook_quant).  `quantile` is ignored when scale_in is given, like in the reference.               */
int inc_codebook_quant_with_scale(const void* w, int wdtype, void* qdq_out, int32_t* int_out, float* scale_out, int64_t N,
                                  int64_t K, int group_size, const float* values, const int32_t* codes, int n_entries,
                                  float quantile, const float* scale_in, inc_stream_t stream);

/* *out += sum((a-b)^2) over n elements, in fp64 with a FIXED summation order (same input -> same bits on every
 * launch; zero *out first).  == the loss of search_clip (utility.py:468) and AWQ's output-MSE (awq.py:336-344,
 * 450-458), which the reference accumulates in Python doubles and takes an argmin over.  `workspace`: at least
 * inc_mse_accumulate_workspace_bytes() bytes of caller-owned device memory (per-workgroup partials).              */
int64_t inc_mse_accumulate_workspace_bytes(void);
int inc_mse_accumulate(const void* a, const void* b, int dtype, int64_t n, double* out, void* workspace,
                       inc_stream_t stream);

/* ---- K5: GPTQ Hessian accumulation ---------------------------------------------------------- *
 * == GPTQ.add_batch (weight_only/gptq.py:1111-1141):
 *     H <- beta*H + alpha * X^T X        (beta = n/(n+b), alpha = 2/(n+b) computed by the caller)
 *   x [T,K] of `xdtype` (row stride ldx elements), H [K,K] fp32.  Only the tiles on/above the
 *   diagonal are touched (syrk); call inc_gptq_hessian_finalize once before factorising.
 *   bf16/fp16 inputs use the bf16/f16 MFMA with fp32 accumulation (products exact);
 *   fp32 inputs use the exact-fp32 MFMA.
 */
int inc_gptq_hessian_accum(const void* x, int xdtype, int64_t T, int64_t K, int64_t ldx, float* H,
                           float beta, float alpha, inc_stream_t stream);

/* The same update for up to 8 Hessians in ONE launch: the distinct layer inputs of one calibration forward of a block
 * (add_batch runs once per hooked layer per forward, gptq.py:670-688) -- xs[i] [T,Ks[i]] 16-bit with row stride
 * ldxs[i], Hs[i] [Ks[i],Ks[i]] fp32, all with the same token count T.  The small Hessians no longer leave half of the
 * CUs idle, and -- given `workspace` (>= inc_gptq_hessian_accum_multi_workspace_bytes(), 16-byte aligned; NULL = off) --
 * the tiles of the launch's last, partly filled round are cut into token ranges computed by otherwise idle CUs and added
 * into H in range order by a second small launch (deterministic).  Every other tile is computed exactly as by
 * inc_gptq_hessian_accum (bit-identical); a tile of the split tail differs from it by the fp32 rounding of adding two to four
 * partial sums instead of one.
 * INC_ERR_UNSUPPORTED (nothing launched) for fp32 inputs, K < 256, unaligned rows or more than 8 problems: call the
 * single-problem entry instead.  The pointer / size arrays are HOST arrays, read before the call returns.             */
int64_t inc_gptq_hessian_accum_multi_workspace_bytes(void);
int inc_gptq_hessian_accum_multi(int n, const void* const* xs, int xdtype, int64_t T, const int64_t* Ks,
                                 const int64_t* ldxs, float* const* Hs, const float* betas, const float* alphas,
                                 void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* ---- K5e: the same update for ALL experts of a fused MoE module, from routed rows ------------ *
 * == GPTQ.add_batch (weight_only/gptq.py:1111-1141) of every expert as if it were an nn.Linear fed the rows routed to it.
 *   `route` is the buffer inc_moe_route wrote for top_k_index [T, top_k] and E experts (offsets [E+1], order [S]; K4e above).
 *   mode 0 (gather): a = x [T, K]; the rows of expert e are x[order[p] / top_k], p = offsets[e] .. offsets[e+1]-1 (gate_up Hessian)
 *   mode 1 (sorted): a [S, K] already in the route's sorted order (down Hessian, fed with silu(g) * u)
 *   H [E, K, K] fp32, rows [E] int64 (device): rows folded so far.  Per expert with c_new = offsets[e+1] - offsets[e] > 0, c = rows[e]:
 *     H[e] <- H[e] * c/(c+c_new) + 2/(c+c_new) * X_e^T X_e  (c = 0: H[e] is overwritten, not read),  rows[e] <- c + c_new
 *   on the tiles on / above the diagonal only (inc_gptq_hessian_finalize works on each H[e] unchanged).  An expert with c_new = 0 is
 *   not touched.  In stream order, no host wait (the grid depends on E and K only); fixed summation order, no atomics: repeated calls
 *   on the same inputs are bit-identical.  16-bit inputs: bf16 / f16 MFMA, fp32 accumulation; fp32 inputs: exact-fp32 MFMA (untuned).
 *   INC_ERR_UNSUPPORTED (nothing launched): E > 512, T * top_k > 2^22, K % 32 != 0, a / H not 16-byte aligned.              */
int inc_gptq_hessian_accum_routed(const void* a, int xdtype, int mode, const int32_t* route, int64_t T, int top_k, int64_t E,
                                  int64_t K, float* H, int64_t* rows, inc_stream_t stream);

/* == GPTQ.fasterquant prologue (gptq.py:1186-1189, 1221-1227): mirror the upper triangle to the
 *   lower, dead[i] = (H[i,i]==0) -> H[i,i]=1, damp = percdamp*mean(diag(H)), H[i,i] += damp.
 *   dead: uint8 [K] out.  workspace: >= 16 bytes.                                               */
int inc_gptq_hessian_finalize(float* H, int64_t K, float percdamp, uint8_t* dead, void* workspace,
                              inc_stream_t stream);

/* == `W = W.float(); W[:, dead] = 0` (gptq.py:1176, 1189): weight of `wdtype` -> fp32 working copy
 *   with the columns flagged in dead (uint8 [K], may be NULL) zeroed.                           */
int inc_gptq_prepare_weight(const void* w, int wdtype, float* out, const uint8_t* dead, int64_t N,
                            int64_t K, inc_stream_t stream);

/* == Quantizer.find_params(weight=True) (gptq.py:1501-1624, int dtype, perchannel, no mse):
 *   per row n and per group g over columns [col0 + g*group_size, ...) of w [N,K] fp32:
 *     scale[n, g0+g], zero[n, g0+g]  (fp32 [N,G]) for ngroups groups.
 *   sym: scale = 2*absmax/maxq, zero = (maxq+1)/2; asym: scale=(max-min)/maxq, zero=round(-min/scale)
 */
int inc_gptq_find_params(const float* w, int64_t N, int64_t K, int64_t col0, int group_size,
                         int ngroups, int bits, int sym, float* scale, float* zero, int64_t G,
                         int64_t g0, inc_stream_t stream);

/* == the same with Quantizer's `mse` shrink-grid search (gptq.py:1567-1584, GPTQConfig(use_mse_search=True)):
 *   for i < int(maxshrink*grid): p = 1 - i/grid; range scaled by p; keep the (scale, zero) minimising
 *   sum |quantize(x) - x|^norm over the group (strict '<').  The reference's configure() uses grid=100,
 *   maxshrink=0.8, norm=2.4 (gptq.py:1375-1387).                                                     */
int inc_gptq_find_params_mse(const float* w, int64_t N, int64_t K, int64_t col0, int group_size,
                             int ngroups, int bits, int sym, int grid, float maxshrink, float norm,
                             float* scale, float* zero, int64_t G, int64_t g0, inc_stream_t stream);

/* == the serial column loop of GPTQ.fasterquant for ONE block of columns [i1, i1+count)
 *   (gptq.py:1250-1299), count <= 128, rows independent:
 *     for i: q = scale*(clamp(rint(w/scale)+zero,0,maxq)-zero); err=(w-q)/Hinv[i,i];
 *            W1[:, i:] -= err (x) Hinv[i, i:];
 *   Un-fused fp32 arithmetic (true divisions, mul-then-sub) == the reference's torch ops.
 *   w [N,K] fp32 working copy (read only here), Hinv [K,K] fp32 upper Cholesky factor of H^-1,
 *   scale/zero [N,G] fp32 (group of column c = c / group_size; group_size<=0 -> one group),
 *   outputs: codes uint8 [N,K] (0..maxq; may be NULL), q_out [N,K] of q_dtype (dequantised,
 *            gptq.py:1337; may be NULL), err [N,128] fp32 (Err1, consumed by inc_gptq_lazy_update).
 */
int inc_gptq_quant_block(const float* w, const float* Hinv, const float* scale, const float* zero,
                         uint8_t* codes, void* q_out, int q_dtype, float* err, int64_t N, int64_t K,
                         int64_t G, int64_t i1, int count, int group_size, int bits,
                         inc_stream_t stream);

/* == inc_gptq_quant_block that ALSO computes the (scale, zero) of the block's groups first: Quantizer.find_params
 *   (gptq.py:1501-1571; perchannel, weight=True, no mse search) on the 128 columns as they are when the block starts
 *   (gptq.py:1266-1272), written to scale / zero [N,G].  Only for a full block on a 128-column boundary whose groups lie
 *   inside it (group_size 32 / 64 / 128) and a reference block size of 128: INC_ERR_UNSUPPORTED otherwise (callers then
 *   use inc_gptq_find_params + inc_gptq_quant_block).  Saves one launch per 128 columns of the serial chain.          */
int inc_gptq_quant_block_params(const float* w, const float* Hinv, float* scale, float* zero,
                                uint8_t* codes, void* q_out, int q_dtype, float* err, int64_t N, int64_t K,
                                int64_t G, int64_t i1, int count, int group_size, int bits, int sym,
                                inc_stream_t stream);

/* == W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:]  (gptq.py:1304), fp32 MFMA.  err [N,128].           */
int inc_gptq_lazy_update(float* w, const float* Hinv, const float* err, int64_t N, int64_t K,
                         int64_t i1, int count, inc_stream_t stream);

/* == the same update (gptq.py:1304) for the columns [col_begin, col_end) only; col_begin - (i1 + count) a multiple
 *   of 128, col_end == K or a multiple of 128 columns past col_begin.  Lets the caller apply the next block's 128
 *   columns first and the remainder on a second stream while the next block's column loop runs; W is bit-identical
 *   to the one-call form.  INC_ERR_UNSUPPORTED when count != 128 (callers then use inc_gptq_lazy_update).       */
int inc_gptq_lazy_update_cols(float* w, const float* Hinv, const float* err, int64_t N, int64_t K,
                              int64_t i1, int count, int64_t col_begin, int64_t col_end,
                              inc_stream_t stream);

/* == K6 as ONE call: the blocked column loop of GPTQ.fasterquant (gptq.py:1250-1304) for one (N-stacked) layer, given the
 *   inverse-Cholesky factor: per 128 columns [find_params ->] quantisation chain -> lazy update, issued by the library on
 *   `stream` in the reference's order.  With `aux_stream` != NULL (and K a multiple of 128, K >= 384, block_size a multiple
 *   of 128) the bulk of every lazy update runs on it underneath the next block's chain; results are bit-identical either way.
 *     w [N,K] fp32 working copy (inc_gptq_prepare_weight; column-permuted by the caller for act_order) -- consumed;
 *     Hinv [K,K] fp32; scale / zero [N,G] fp32: written for dynamic groups (find_params on W "as it is now", gptq.py:1266-1272),
 *     read otherwise; loop_scale / loop_zero [N,loop_G] (may be NULL = scale / zero): the table the chain reads, with
 *     kernel_group_size columns per entry (<= 0: one group) -- differs from scale / zero only for act_order + static_groups
 *     (one entry per column); codes uint8 [N,K] and q_out [N,K] of q_dtype (either may be NULL); err_ws fp32 [2, N, 128];
 *     group_size = columns per quantisation group (K for per-channel); block_size = GPTQConfig.block_size (<= 0: K);
 *     flags: INC_GPTQ_DYNAMIC_GROUPS (group_size != -1 and not static_groups), INC_GPTQ_MSE (use_mse_search),
 *            INC_GPTQ_NO_LOOKAHEAD, INC_GPTQ_NO_FUSED_PARAMS (A/B switches; default = fastest bit-identical form).      */
#define INC_GPTQ_DYNAMIC_GROUPS 1
#define INC_GPTQ_MSE 2
#define INC_GPTQ_NO_LOOKAHEAD 4
#define INC_GPTQ_NO_FUSED_PARAMS 8
int inc_gptq_quantize_layer(float* w, const float* Hinv, float* scale, float* zero, int64_t G,
                            const float* loop_scale, const float* loop_zero, int64_t loop_G, uint8_t* codes,
                            void* q_out, int q_dtype, float* err_ws, int64_t N, int64_t K, int group_size,
                            int kernel_group_size, int block_size, int bits, int sym, int flags,
                            inc_stream_t stream, inc_stream_t aux_stream);

/* ---- K6': diagonal block of the blocked inverse-Cholesky factor -------------------------------- *
 * The reference builds Hinv = cholesky(cholesky_inverse(cholesky(H)), upper) (gptq.py:1228-1230) with
 * three LAPACK factorisations.  Here U = J Lr^-1 J with J H J = Lr Lr^T (see gptq.py: inverse_cholesky_upper):
 * a blocked Cholesky + a blocked triangular inverse whose O(K^3) parts are fp32 GEMMs; this entry point is
 * the unblocked kernel for one diagonal block (== LAPACK potf2 + trti2 on it):
 *   A [n,n] fp32 (row stride lda, n <= 128): lower triangle read; on return the lower triangle holds L
 *   (A = L L^T) and the strict upper triangle is zero.  Linv [n,n] (row stride ldi) receives L^-1.
 *   info: device int32, atomically max-ed with `tag` when a pivot is not positive (H not SPD).
 */
int inc_chol_diag_block(float* A, int64_t lda, int n, float* Linv, int64_t ldi, int32_t* info, int tag,
                        inc_stream_t stream);

/* ---- K6': the whole inverse-Cholesky factor (gptq.py:1228-1231) as ONE call ---------------------- *
 * inc_gptq_inverse_factor: U [K,K] fp32 = upper Cholesky factor of H^-1 (H^-1 = U^T U) for the symmetric positive
 *   definite H [K,K] fp32 (dense, row stride K; already damped: inc_gptq_hessian_finalize; H is only read).
 *   == `H = cholesky(H); H = cholesky_inverse(H); Hinv = cholesky(H, upper=True)`, computed as U = J L^-1 J with
 *   J H J = L L^T: one blocked Cholesky + one blocked triangular inverse (128 inside 1024 columns), every product an
 *   exact-fp32 MFMA GEMM of this library (v_mfma_f32_32x32x2_f32, triangular operands skipped by K-range, syrk on the
 *   lower tiles only), the diagonal blocks by the inc_chol_diag_block kernel.  The chain (diagonal blocks, block
 *   inverses, panel solves, the update of the next block's columns) is issued on `stream`; with `aux_stream` (may be
 *   NULL) the rest of every trailing update and the top-level doubling products run there underneath the chain (two
 *   transient HIP events; the call returns with `stream` ordered behind everything).  Deterministic.  With flags = 0 the
 *   two-stream form is bit-identical to the one-stream form; with flags bit 1 it is NOT: the side stream's products stay exact
 *   fp32 (one plane buffer, owned by the main stream), so the factor differs from the one-stream form within the distance
 *   bit 1 is gated by (both <= 1e-6 relative from an fp64 factor).
 *   workspace: >= inc_gptq_inverse_factor_workspace_bytes(K, flags) bytes, 16-byte aligned, contents undefined on return
 *   (3 Kp^2 + 2048 Kp floats, Kp = K rounded up to 128; + 6 (Kp + 256)(Kp + 128) bytes of bf16 planes with flags bit 1:
 *   2.2 GB at K = 11008, 14.8 GB at K = 28672).
 *   info: device int32, written by the call: 0, or the (1-based) index of the last 128-column diagonal block with a
 *   non-positive pivot (H not positive definite -- the reference's torch.linalg.cholesky raises there); U is
 *   undefined in that case.  flags: bit 0 = ignore aux_stream (one stream); bit 1 = the large products with
 *   their fp32 operands split into three bf16 pieces (six bf16 MFMAs per fp32 product: dropped terms <= 2^-24 |a b|, same distance to an
 *   fp64 factor as the exact-fp32 products of flags = 0, 1.3 - 2 x faster; the Python driver's default).                */
int64_t inc_gptq_inverse_factor_workspace_bytes(int64_t K, int flags);
int inc_gptq_inverse_factor(const float* H, int64_t K, float* U, void* workspace, int64_t workspace_bytes, int32_t* info,
                            int flags, inc_stream_t stream, inc_stream_t aux_stream);

/* ---- K8: AWQ statistics ---------------------------------------------------------------------- *
 * inc_awq_act_abs_sum: out[k] += sum_t |x[t,k]|  (fp32 [K], accumulate; caller divides by T)
 *   == _get_act_scale (weight_only/awq.py:151-154).
 * inc_awq_weight_scale: out[k] = sum_n( |w[n,k]| / max_{k' in group(k)} |w[n,k']| )
 *   == _get_weight_scale (awq.py:131-147).  w [N,K] of wdtype, out fp32 [K].
 */
int inc_awq_act_abs_sum(const void* x, int xdtype, int64_t T, int64_t K, float* out,
                        inc_stream_t stream);
/* out[k] += sum_n |w[n,k]| / groupmax (zero `out` first; the caller divides by N).
 * workspace: inc_awq_weight_scale_workspace_bytes (fp32 group maxima [N, K/group_size]).          */
int64_t inc_awq_weight_scale_workspace_bytes(int64_t N, int64_t K, int group_size);
int inc_awq_weight_scale(const void* w, int wdtype, int64_t N, int64_t K, int group_size, float* out,
                         void* workspace, int64_t workspace_bytes, inc_stream_t stream);

/* ---- K9: AutoAWQ checkpoint words -> optimum layout -------------------------------------------- *
 * == repack_awq_to_optimum_format (weight_only/utility.py:1426-1459 = unpack_awq :1273 + awq_reverse_reorder_int_tensor
 *    :1246 + pack_from_tensors :1355), called by repack_awq_and_load_state_dict
 *    (transformers/quantization/utils.py:655-697) when an AutoAWQ checkpoint is loaded.  Integer field shuffle:
 *   awq_qweight [K, N/8] int32 (field i of word (k,c) = code(k, 8c + {0,2,4,6,1,3,5,7}[i]))  ->  qweight [K/8, N] int32
 *   awq_qzeros  [G, N/8] int32 (same field order, plain zero points)                       ->  qzeros  [G, N/8] int32
 *                                                                                            (sequential, (z-1)&15)
 * scales [G, N] fp16 are shared unchanged.  bits must be 4 (as in the reference); K % 8 == 0, N % 8 == 0.      */
int inc_awq_repack(const int32_t* awq_qweight, const int32_t* awq_qzeros, int64_t K, int64_t N, int64_t G, int bits,
                   int32_t* qweight, int32_t* qzeros, inc_stream_t stream);

/* ---- K10-K14: SmoothQuant W8A8 (BASELINE config #4) ------------------------------------------------ *
 * Reference: neural_compressor/torch/algorithms/smooth_quant/utility.py.  The reference executes W8A8 through
 * intel_extension_for_pytorch (smooth_quant.py:105-125; not vendored): the in-tree fake-quant functions are the spec.
 *
 * inc_sq_channel_minmax: mn[k] = min(mn[k], min_t x[t,k]), mx[k] = max(mx[k], max_t x[t,k])          (fp32 [K] each,
 *   initialise to +FLT_MAX / -FLT_MAX) == Calibration._save_input_pc_hook (:858-883), x [T,K] with row stride ld.
 * inc_sq_weight_col_absmax: out[k] = max(out[k], max_n |w[n,k]|) (zero `out` first; call once per Linear that shares
 *   the input) == the `torch.max(torch.abs(torch.cat(weights)), dim=0)` of cal_scale (:617-618).
 * inc_sq_cal_scale: s[k] = clip(amax_x[k]^alpha / clip(amax_w[k], lb)^(1-alpha), 1e-5), s = 1 where amax_x^alpha == 0
 *   == cal_scale (:605-626).
 * inc_sq_quant_weight: per-output-channel symmetric int8 of W * smooth (smooth may be NULL):
 *   scale[n] = clip(max_k |w'| / 127.5, eps), q = clamp(rint(w' / scale), -128, 127) == quant_dequant_w_v1 (:669-690);
 *   qw [N, Kp] int8 (Kp >= K, columns K..Kp-1 are zero), rowsum[n] = sum_k q[n,k] (int32).
 * inc_sq_quant_act: out[m,k] = clamp(rint(x[m,k] * in_scale[k] / sx + zp), 0, 255) - 128 as int8 [M, Kp]
 *   == SQLinearWrapper.forward's mul (:2602) + quant_dequant_x_v1 (:726-755) with the static (sx, zp) of
 *   SQLinearWrapper._calculate_qparams (:2607-2631); in_scale may be NULL (folded smoothing).  Kp % 16 == 0.
 * inc_w8a8_gemm: y[m,n] = alpha[n] * (sum_k xq[m,k] * wq[n,k] + corr[n]) + bias[n]   (v_mfma_i32_32x32x32_i8)
 *   alpha[n] = sx * w_scale[n], corr[n] = (128 - zp) * rowsum[n] (may be NULL), bias in ydtype or NULL,
 *   y bf16 / fp16 [M,N]; K % 128 == 0 (pad with zero weight codes), xq / wq 16-byte aligned.
 *   workspace (inc_w8a8_gemm_workspace_bytes, may be NULL): when the last round of 256x256 tiles would leave most
 *   CUs idle its tiles are split along K into int32 slabs there and a second small kernel finishes them (no
 *   initialisation needed).  Integer sums: the result is bit-identical with or without the workspace.
 *
 * The dynamic per-token symmetric int8 activation cell.  The reference has no text for it (its IPEX path picks the activation
 * observer out of tree); it stands in for inc_sq_quant_act + inc_w8a8_gemm where a frozen per-tensor range is too coarse, and its
 * specification is DESIGN.md section 8, in fp32 with true division and round-half-even:
 * inc_sq_quant_act_token: t = x[m,k] * in_scale[k] (in_scale may be NULL), row_scale[m] = max(max_k |t| / 127, FLT_EPSILON),
 *   xq[m,k] = clamp(rint(t / row_scale[m]), -127, 127) as int8 [M, Kp], 0 for k >= K; no zero point.  Kp % 16 == 0, xq 16-byte
 *   aligned, row_scale fp32 [M].  x bf16 / fp16 / fp32 [M,K] contiguous, read from HBM once for Kp <= 16384.
 * inc_w8a8_gemm_rowscale: y[m,n] = (row_scale[m] * alpha[n]) * (sum_k xq[m,k] * wq[n,k]) + bias[n] with alpha = w_scale: the
 *   kernels, plan and workspace (inc_w8a8_gemm_workspace_bytes) of inc_w8a8_gemm with a row factor in the epilogues, no corr. */
int64_t inc_w8a8_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int inc_sq_channel_minmax(const void* x, int xdtype, int64_t T, int64_t K, int64_t ld, float* mn, float* mx,
                          inc_stream_t stream);
int inc_sq_weight_col_absmax(const void* w, int wdtype, int64_t N, int64_t K, float* out, inc_stream_t stream);
int inc_sq_cal_scale(const float* amax_x, const float* amax_w, int64_t K, float alpha, float weight_max_lb, float* scale,
                     inc_stream_t stream);
int inc_sq_quant_weight(const void* w, int wdtype, int64_t N, int64_t K, int64_t Kp, const float* smooth, int8_t* qw,
                        float* w_scale, int32_t* rowsum, inc_stream_t stream);
int inc_sq_quant_act(const void* x, int xdtype, int64_t M, int64_t K, int64_t Kp, const float* in_scale, float sx, float zp,
                     int8_t* out, inc_stream_t stream);
int inc_w8a8_gemm(const int8_t* xq, const int8_t* wq, const float* alpha, const int32_t* corr, const void* bias, void* y,
                  int ydtype, int64_t M, int64_t N, int64_t K, void* workspace, int64_t workspace_bytes,
                  inc_stream_t stream);
int inc_sq_quant_act_token(const void* x, int xdtype, int64_t M, int64_t K, int64_t Kp, const float* in_scale, int8_t* xq,
                           float* row_scale, inc_stream_t stream);
int inc_w8a8_gemm_rowscale(const int8_t* xq, const int8_t* wq, const float* row_scale, const float* alpha, const void* bias,
                           void* y, int ydtype, int64_t M, int64_t N, int64_t K, void* workspace, int64_t workspace_bytes,
                           inc_stream_t stream);

/* ---- OCP microscaling (MX): MXFP8 / MXFP4 linears on v_mfma_scale_f32_32x32x64_f8f6f4 (csrc/mx.hip, csrc/gemm_mx.hip) ---------- *
 * The reference's MXQuantConfig / MXLinear (torch/algorithms/mx_quant/) emulate the formats with fake quantisation in float; these
 * two entry points execute them.  This text is the specification.  Inputs are finite.
 *   A block is 32 consecutive elements along K (= in_features, for activation rows and weight rows alike).
 *   Scale:    amax = max |x| of the block as fp32;  byte = clamp(expfield(amax) - emax, 0, 254), expfield the biased 8-bit exponent
 *             field of amax (0 for zero and subnormals), emax = 8 for e4m3 and 2 for e2m1.  The block scale is 2^(byte - 127)
 *             (E8M0; byte 255 is never written).
 *   Elements: v = x * 2^(127 - byte), exact; v rounded to nearest, ties to even, onto the element format, saturating to +-448 for
 *             e4m3 (OCP e4m3fn, subnormals down to 2^-9 kept, no NaN code emitted) and to +-6 for e2m1 (grid 0, 0.5, 1, 1.5, 2, 3,
 *             4, 6).  The sign bit of a code is the sign bit of x, for zeros too.
 *   Padding:  columns K .. Kp-1 count as zeros: code 0, and a block that is all padding gets byte 0.  Kp is a multiple of
 *             INC_MX_KTILE = 128 elements for both formats (the GEMM's K-tile; fp4 needs no larger one).
 *   Storage:  fp8 codes [rows, Kp] uint8; fp4 codes [rows, Kp/2] uint8, element 2i in the low nibble and 2i+1 in the high nibble
 *             (the instruction's own order: no permutation in the kernel); scales [rows, Kp/32] uint8.
 *   Product:  y[m,n] = sum_blocks 2^(sx + sw - 254) * sum_{k in block} a_k * b_k  +  bias[n], accumulated in fp32 inside the
 *             matrix pipe (its summation order is not documented), fp32 bias add, one rounding to bf16 / fp16.
 * `fmt` values are the instruction's own format codes.
 * inc_mx_quant: the row quantiser above.  x bf16 / fp16 / fp32 [M,K] contiguous, of any alignment (16-byte loads when K is a
 *   multiple of 8 (fp32: 4) and x is 16-byte aligned); codes 16-byte aligned.  One lane per block: each row is read from HBM once.
 *   Writes every code byte and scale byte, the padding included, and nothing else.  Serves activations at run time and weights at
 *   convert time.  INC_ERR_UNSUPPORTED (nothing launched) for an unknown fmt / dtype or Kp % 128 != 0.
 * inc_mx_gemm: the product above for (xfmt, wfmt) = (fp8, fp8), (fp8, fp4), (fp4, fp4); any other pair is INC_ERR_UNSUPPORTED.
 *   xq [M, Kp or Kp/2], xs [M, Kp/32], wq [N, Kp or Kp/2], ws [N, Kp/32] as stored by inc_mx_quant, xq / wq 16-byte and xs / ws
 *   4-byte aligned; bias [N] in ydtype or NULL; y [M,N] bf16 / fp16, any M >= 1 and N >= 1 (8-byte stores when N % 4 == 0 and y is
 *   8-byte aligned, 2-byte stores otherwise).  256 x 256 x 128 tiles, one workgroup per tile, no split-K tail; the decode route for
 *   M <= 16 is inc_mx_gemv.
 * inc_mx_gemv (csrc/gemm_mx_gemv.hip): the product of inc_mx_gemm for 1 <= M <= INC_MX_GEMV_MAX_M on v_mfma_scale_f32_16x16x128_f8f6f4:
 *   the same operands, storage, alignment rules, format pairs and arithmetic (fp32 accumulation, fp32 bias add, one rounding), any
 *   N >= 1, the same store rule for y.  One workgroup per strip of 16 weight rows, K split over its waves, the partials added in a
 *   fixed order through LDS: no workspace, and repeated calls are bit-identical.  Reads nothing past row M - 1 of x or row N - 1 of W.
 *   INC_ERR_UNSUPPORTED (nothing launched) for M > 16, an unbuilt pair, Kp % 128 != 0 or a ydtype other than bf16 / fp16;
 *   INC_ERR_BAD_ARG for a NULL operand or M, N < 1.
 * inc_mx_gemv_multi: 2 <= n <= 8 weight matrices that multiply the SAME x (q / k / v; gate / up) in ONE launch over the strips of all
 *   members.  wq, ws, bias, y and N are HOST arrays of n entries (the convention of inc_woq_gemv_anyw_multi); bias may be NULL or hold
 *   NULL for a member without one; x, the format pair, ydtype and Kp are common.  y[i] is bit-identical to inc_mx_gemv on member i
 *   alone (the same strip body).  Rejections as for inc_mx_gemv, and INC_ERR_UNSUPPORTED for n outside 2 .. 8.
 * inc_mx_moe_gemm (csrc/gemm_strip_moe.hip, K16e): the product of inc_mx_gemm per expert over the rows inc_moe_route sorted -- the two
 *   F.linear of transformers' MixtralExperts.forward (also the Qwen2-MoE / Qwen3-MoE / OLMoE experts) for MX experts.  One forward is
 *   inc_moe_route -> inc_mx_quant(x) -> inc_mx_moe_gemm(0) -> inc_mx_quant(h) -> inc_mx_moe_gemm(1) -> inc_moe_combine on `stream`.
 *   `route` is K4e's buffer, unchanged ([0] tile count, offsets [E+1], order [S], pos [S], tiles of 64 rows; S = T * top_k).
 *   wq [E, N, Kp] (fp8) or [E, N, Kp/2] (fp4), ws [E, N, Kp/32]: slice e is exactly what inc_mx_quant writes for expert e's [N, K]
 *   matrix.  acc[p, n] = the product above without bias, for position p of the sorted order and the expert e whose range holds p,
 *   summed in fp32 in a fixed order (repeated calls are bit-identical):
 *     mode 2 (plain, gathered):   aq [T, Kp or Kp/2], as [T, Kp/32]; row p is token order[p] / top_k; out [S, N] fp32 = acc
 *     mode 0 (gate_up, gathered, N = 2I): gate rows 0 .. I-1 and up rows I .. 2I-1 of the expert; out [S, I] of odtype (INC_BF16 /
 *            INC_F16), out[p, j] = rd(g / (1.f + expf(-g)) * u), g = acc[p, j], u = acc[p, I + j], formed in fp32, rounded once
 *     mode 1 (down, in place):    aq [S, Kp or Kp/2], as [S, Kp/32] in sorted order; out [S, N] fp32 = w[order[p]] * acc[p, n] (one
 *            fp32 multiply), routing_weights w [T, top_k] of wdtype INC_F32 / INC_BF16 / INC_F16
 *   odtype is INC_F32 in modes 1 and 2.  Positions >= offsets[E] are never written and source rows that no valid position names are
 *   never read.  aq / wq 16-byte aligned; out is stored 4 columns at a time when its width is a multiple of 4 and it is aligned to
 *   that store, element by element otherwise.  No workspace and no counters.
 *   INC_ERR_UNSUPPORTED (nothing launched) for a pair other than inc_mx_gemm's three, Kp % 128 != 0, E > 512, S > 2^22, mode 0 with odd
 *   N, a bad odtype or (mode 1) wdtype; INC_ERR_BAD_ARG for a NULL operand (routing_weights: mode 1 only) or a size < 1.
 * inc_mx_moe_gemm_glu (the same kernel with a second epilogue): inc_mx_moe_gemm for the experts of GPT-OSS (transformers'
 *   GptOssExperts) -- a per-expert bias in every mode and a clamped SwiGLU instead of the SiLU product in mode 0.  Everything not
 *   named here is inc_mx_moe_gemm's: the operands, the route, the three format pairs, the tile / strip map, the in-workgroup K split,
 *   the output dtypes per mode and the argument checks in their order.  acc is that kernel's fp32 sum (the same waves in the same
 *   order: bit-identical).  bias fp32 [E, N], 4-byte aligned, or NULL; b(e, n) = bias[e * N + n], and with bias == NULL no add is
 *   made.  Mode 0 keeps the row convention: gate rows 0 .. I-1 and up rows I .. 2I-1 of wq, ws and bias (GPT-OSS interleaves gate and
 *   up; the caller de-interleaves once, at conversion).
 *     mode 0:  g = acc[p, j] + b(e, j);  u = acc[p, I + j] + b(e, I + j)                    (one fp32 add each)
 *              g = fminf(g, limit);      u = fminf(fmaxf(u, -limit), limit)
 *              out[p, j] = rd16( (u + 1.f) * (g / (1.f + expf(-(alpha * g)))) )             (fp32, no contraction, ONE rounding)
 *     mode 1:  out[p, n] = w[order[p]] * (acc[p, n] + b(e, n))                              (fp32; HF: (h @ W + bias) * weight)
 *     mode 2:  out[p, n] = acc[p, n] + b(e, n)                                              (fp32)
 *   alpha and limit are used in mode 0 only (GPT-OSS: 1.702 and 7.0); limit = +inf is no clamp.  On top of inc_mx_moe_gemm's checks:
 *   INC_ERR_BAD_ARG unless limit > 0 and alpha == alpha, and for a bias that is not 4-byte aligned.  With a NaN accumulator (NaN
 *   codes or 0xFF scale bytes, which inc_mx_quant never writes for finite input) the output is unspecified.  bias is read after the
 *   LDS sum, by the lanes that store, for the columns they store.
 * All six validate their arguments before any HIP call.                                                                         */
#define INC_MX_FP8_E4M3 0
#define INC_MX_FP4_E2M1 4
#define INC_MX_KTILE 128
#define INC_MX_GEMV_MAX_M 16
int inc_mx_quant(const void* x, int xdtype, int64_t M, int64_t K, int64_t Kp, int fmt, uint8_t* codes, uint8_t* scales,
                 inc_stream_t stream);
int inc_mx_gemm(const uint8_t* xq, const uint8_t* xs, int xfmt, const uint8_t* wq, const uint8_t* ws, int wfmt, const void* bias,
                void* y, int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream);
int inc_mx_gemv(const uint8_t* xq, const uint8_t* xs, int xfmt, const uint8_t* wq, const uint8_t* ws, int wfmt, const void* bias,
                void* y, int ydtype, int64_t M, int64_t N, int64_t Kp, inc_stream_t stream);
int inc_mx_gemv_multi(int n, const uint8_t* xq, const uint8_t* xs, int xfmt, const uint8_t* const* wq, const uint8_t* const* ws,
                      int wfmt, const void* const* bias, void* const* y, int ydtype, int64_t M, const int64_t* N, int64_t Kp,
                      inc_stream_t stream);
int inc_mx_moe_gemm(int mode, const uint8_t* aq, const uint8_t* as, int afmt, const int32_t* route, const uint8_t* wq,
                    const uint8_t* ws, int wfmt, const void* routing_weights, int wdtype, void* out, int odtype, int64_t T, int top_k,
                    int64_t E, int64_t N, int64_t Kp, inc_stream_t stream);
int inc_mx_moe_gemm_glu(int mode, const uint8_t* aq, const uint8_t* as, int afmt, const int32_t* route, const uint8_t* wq,
                        const uint8_t* ws, int wfmt, const float* bias, float alpha, float limit, const void* routing_weights,
                        int wdtype, void* out, int odtype, int64_t T, int top_k, int64_t E, int64_t N, int64_t Kp,
                        inc_stream_t stream);

/* ---- FP8 per-token / per-channel: OCP e4m3 codes, one fp32 scale per row of x and one per row of W ------- *
 * The "FP8 dynamic" cell: csrc/sq.hip (the quantiser, next to the int8 token kernel it shares its structure with) and
 * csrc/gemm_fp8.hip and csrc/gemm_fp8_group.hip (the products, on v_mfma_f32_32x32x64_f8f6f4 and v_mfma_f32_16x16x128_f8f6f4).  This text is the specification.
 * Inputs are finite; for a row with a NaN or an infinity nothing is promised except that every write stays in bounds.
 * inc_fp8_quant_rows: x bf16 / fp16 / fp32 [M,K] contiguous, of any alignment; in_scale fp32 [K] or NULL.
 *     t            = float(x[m,k]) * in_scale[k]                       (one fp32 multiply; t = float(x[m,k]) without in_scale)
 *     row_scale[m] = max(max_k |t| / 448.0f, 0x1p-60f)                 (fp32, true division; the floor only keeps an all-zero row
 *                                                                       finite -- e4m3 has a dynamic range of its own)
 *     codes[m,k]   = e4m3(t / row_scale[m])                            (fp32 true division, then round to nearest, ties to even,
 *                    onto the OCP e4m3fn grid -- subnormals down to 2^-9 kept -- saturating at +-448: the quotient can exceed 448
 *                    by one rounding; the element rounding of inc_mx_quant for INC_MX_FP8_E4M3, the same device function)
 *   The sign bit of a code is the sign bit of t, for zeros too; the NaN codes 0x7f / 0xff are never written.  Columns K .. Kp-1 are
 *   code 0.  codes uint8 [M,Kp] 16-byte aligned, Kp >= K a multiple of INC_MX_KTILE = 128; row_scale fp32 [M].  One workgroup per
 *   row; a row is read from HBM once for Kp <= 16384 and twice above.  max is order-free, so codes and row_scale have one right
 *   answer, bit for bit.  A weight [N,K] with one scale per output channel is the same call, row-wise.
 *   INC_ERR_UNSUPPORTED (nothing launched) for an unknown dtype or Kp % 128 != 0.
 * inc_fp8_gemm: y[m,n] = rd16((row_scale[m] * alpha[n]) * acc[m,n] + bias[n]), acc[m,n] = sum_k xq[m,k] * wq[n,k] accumulated in
 *   fp32 by the matrix pipe over the K-tiles of 128 in ascending order (the order inside an instruction is not documented; the
 *   accumulator is bit for bit that of inc_mx_gemm (fp8, fp8) with every scale byte 127).  The factor product is one fp32 multiply;
 *   the multiply by acc and the bias add may contract to one fma, as in inc_w8a8_gemm_rowscale.  xq [M,Kp], wq [N,Kp] uint8, 16-byte
 *   aligned; row_scale fp32 [M], alpha fp32 [N] (= the weight's row_scale); bias [N] in ydtype or NULL; y [M,N] bf16 / fp16, any
 *   M >= 1 and N >= 1 (8-byte stores when N % 4 == 0 and y is 8-byte aligned, 2-byte stores otherwise).  256 x 256 x 128 tiles, one
 *   workgroup per tile, no split-K tail, no workspace.
 * inc_fp8_gemv: the same product for 1 <= M <= INC_MX_GEMV_MAX_M: one workgroup per strip of 16 weight rows, K split over its 8 waves
 *   (wave w takes the K-tiles w, w + 8, ... in ascending order), the 8 partials added in wave order through LDS, then the epilogue
 *   above: no workspace, repeated calls are bit-identical, and acc is bit for bit that of inc_mx_gemv with every scale byte 127.
 *   Reads nothing past row M - 1 of xq or row N - 1 of wq.
 * Both products: INC_ERR_UNSUPPORTED (nothing launched) for Kp % 128 != 0, a ydtype other than bf16 / fp16 or (gemv) M > 16;
 *   INC_ERR_BAD_ARG for a NULL operand, a size < 1 or a misaligned pointer.  All three validate their arguments before any HIP call.
 * inc_fp8_gemv_multi (csrc/gemm_fp8_group.hip, K17g): 2 <= n <= 8 weight matrices that multiply the SAME x (q / k / v; gate / up) in
 *   ONE launch over the strips of all members.  wq, alpha, bias, y and N are HOST arrays of n entries (the convention of
 *   inc_mx_gemv_multi); bias may be NULL or hold NULL for a member without one; xq, row_scale, ydtype, M and Kp are common.  y[i] is
 *   bit-identical to inc_fp8_gemv on member i alone (the same strip body) and nothing outside the [M, N[i]] elements at y[i] is
 *   written.  Rejections as for inc_fp8_gemv, per member, and INC_ERR_UNSUPPORTED for n outside 2 .. 8.
 * inc_fp8_gemv_gated (the same file): the gate / up pair of a gated MLP with the SiLU product in the epilogue, 1 <= M <= 16.
 *   wq_gate, wq_up [N, Kp], alpha_gate, alpha_up fp32 [N], bias_gate, bias_up [N] in ydtype or NULL (each on its own); h [M, N]:
 *     g = (row_scale[m] * alpha_gate[n]) * acc_gate[m,n] + bias_gate[n],  u = (row_scale[m] * alpha_up[n]) * acc_up[m,n] + bias_up[n]
 *     h[m,n] = rd16(g / (1.f + expf(-g)) * u)
 *   acc_gate / acc_up are inc_fp8_gemv's sums over the gate / up weight (one workgroup owns strip s of both, the 8 waves split K as
 *   there, the two sets of 8 partials are added in wave order); g and u are inc_fp8_gemv's values BEFORE its rounding (the same
 *   expression, the same possible contraction), the SiLU product is formed in fp32 and h is rounded once.  Without a bias h is bit
 *   for bit inc_fp8_moe_gemm's mode 0 for one expert with weight cat(gate, up), alpha cat(alpha_gate, alpha_up) and every row routed
 *   to it.  Below g ~ -88.7 expf(-g) is +inf and silu(g) is -0, which is the rounded exact value; g = -inf gives NaN.  The store rule
 *   of y, the reads (nothing past row M - 1 of xq or row N - 1 of a weight) and the rejections are inc_fp8_gemv's.
 *   Both validate their arguments before any HIP call; no workspace, no counters, repeated calls are bit-identical.
 * inc_fp8_moe_gemm (csrc/gemm_strip_moe.hip, K17e): the product of inc_fp8_gemm per expert over the rows inc_moe_route sorted -- the two
 *   F.linear of transformers' MixtralExperts.forward (also the Qwen2-MoE / Qwen3-MoE / OLMoE experts) for FP8 experts.  One forward is
 *   inc_moe_route -> inc_fp8_quant_rows(x) -> inc_fp8_moe_gemm(0) -> inc_fp8_quant_rows(h) -> inc_fp8_moe_gemm(1) -> inc_moe_combine
 *   on `stream`.  `route` is K4e's buffer, unchanged ([0] tile count, offsets [E+1], order [S], pos [S], tiles of 64 rows; S = T *
 *   top_k).  wq [E, N, Kp] uint8, alpha fp32 [E, N]: slice e of both is exactly what inc_fp8_quant_rows writes for expert e's [N, K]
 *   matrix.  For position p of the sorted order and the expert e whose range holds p, acc[p, n] = sum_k aq[row, k] * wq[e, n, k] is
 *   the fp32 accumulator of v_mfma_f32_16x16x128_f8f6f4 over the row's K-tiles in inc_mx_moe_gemm's fixed order (wave w of 8 takes
 *   the tiles w, w + 8, ... ascending, the 8 partials are added in wave order; repeated calls are bit-identical; bit for bit the
 *   accumulator of inc_mx_moe_gemm (fp8, fp8) with every scale byte 127, and for one expert's rows that of inc_fp8_gemv), and
 *   f(r, n) = a_scale[r] * alpha[e, n] is one fp32 multiply:
 *     mode 2 (plain, gathered):   aq [T, Kp], a_scale [T]; r = order[p] / top_k; out [S, N] fp32 = f(r, n) * acc[p, n] (one fp32
 *            multiply)
 *     mode 0 (gate_up, gathered, N = 2I): gate rows 0 .. I-1 and up rows I .. 2I-1 of the expert; r as in mode 2; out [S, I] of odtype
 *            (INC_BF16 / INC_F16), out[p, j] = rd(g / (1.f + expf(-g)) * u), g = f(r, j) * acc[p, j], u = f(r, I + j) * acc[p, I + j],
 *            formed in fp32, rounded once
 *     mode 1 (down, in place):    aq [S, Kp], a_scale [S] in sorted order, r = p; out [S, N] fp32 = w[order[p]] * (f(p, n) * acc[p, n])
 *            (three fp32 multiplies in that association; no add, so nothing contracts), routing_weights w [T, top_k] of wdtype
 *            INC_F32 / INC_BF16 / INC_F16
 *   odtype is INC_F32 in modes 1 and 2.  Positions >= offsets[E] are never written, and source rows that no valid position names are
 *   never read, their a_scale entry included.  aq / wq 16-byte aligned, a_scale / alpha 4-byte aligned; out is stored 4 columns at a
 *   time when its width is a multiple of 4 and it is aligned to that store, element by element otherwise.  No workspace, no counters.
 *   INC_ERR_UNSUPPORTED (nothing launched) for Kp % 128 != 0, E > 512, S > 2^22, mode 0 with odd N, a bad odtype or (mode 1) wdtype;
 *   INC_ERR_BAD_ARG for a NULL operand (routing_weights: mode 1 only), a size < 1 or a misaligned pointer.  Validated before any HIP
 *   call.                                                                                                                          */
int inc_fp8_quant_rows(const void* x, int xdtype, int64_t M, int64_t K, int64_t Kp, const float* in_scale, uint8_t* codes,
                       float* row_scale, inc_stream_t stream);
int inc_fp8_gemm(const uint8_t* xq, const float* row_scale, const uint8_t* wq, const float* alpha, const void* bias, void* y, int ydtype,
                 int64_t M, int64_t N, int64_t Kp, inc_stream_t stream);
int inc_fp8_gemv(const uint8_t* xq, const float* row_scale, const uint8_t* wq, const float* alpha, const void* bias, void* y, int ydtype,
                 int64_t M, int64_t N, int64_t Kp, inc_stream_t stream);
int inc_fp8_gemv_multi(int n, const uint8_t* xq, const float* row_scale, const uint8_t* const* wq, const float* const* alpha,
                       const void* const* bias, void* const* y, int ydtype, int64_t M, const int64_t* N, int64_t Kp,
                       inc_stream_t stream);
int inc_fp8_gemv_gated(const uint8_t* xq, const float* row_scale, const uint8_t* wq_gate, const float* alpha_gate,
                       const void* bias_gate, const uint8_t* wq_up, const float* alpha_up, const void* bias_up, void* h, int ydtype,
                       int64_t M, int64_t N, int64_t Kp, inc_stream_t stream);
int inc_fp8_moe_gemm(int mode, const uint8_t* aq, const float* a_scale, const int32_t* route, const uint8_t* wq, const float* alpha,
                     const void* routing_weights, int wdtype, void* out, int odtype, int64_t T, int top_k, int64_t E, int64_t N,
                     int64_t Kp, inc_stream_t stream);

/* ---- measured ceilings (bench.py `ceilings`) -- measurement helpers, not on the hot path ------------- *
 * inc_probe_hbm_triad: a <- b + s*c over n fp32 (n % 4 == 0): 12 n bytes of HBM traffic per call.
 * inc_probe_mfma_bf16: `blocks` workgroups x 4 waves x `iters` x 8 v_mfma_f32_32x32x16_bf16 on operands read from `src`
 *   (>= 64 KiB, any non-zero data); *flops_out (host pointer, may be NULL) receives the flops of the launch.            */
int inc_probe_hbm_triad(float* a, const float* b, const float* c, float s, int64_t n, inc_stream_t stream);
/* dst <- src: `bytes` read + `bytes` written, 16 bytes per lane; `variant` 0..15 picks loads in flight per lane / non-temporal hints /
 * grid shape (probe.hip).  The copy ceiling of the chip (guide: 6.29 TB/s) is what the streaming kernels K1-K3 are priced against. */
int inc_probe_hbm_copy(void* dst, const void* src, int64_t bytes, int variant, inc_stream_t stream);
int inc_probe_mfma_bf16(const void* src, float* sink, int blocks, int iters, double* flops_out, inc_stream_t stream);
/* inc_trace_marker: an EMPTY launch of `id` (1..4096) workgroups of 64 threads on `stream`: a phase boundary that a
 *   `rocprofv3 --kernel-trace` timeline shows as inc_trace_marker_kernel with Grid_Size_X = 64 * id (scripts/step_timeline.py). */
int inc_trace_marker(int id, inc_stream_t stream);

/* ---- forward elementwise chains of a Llama block (csrc/fwd_elementwise.hip) -------------------------------------------------- *
 * One streaming kernel each for the three elementwise chains of a block forward, BIT-IDENTICAL to eager PyTorch-ROCm (every
 * intermediate rounds to the tensor dtype where a torch kernel would).  dtype INC_BF16 / INC_F16.  All three return
 * INC_ERR_BAD_ARG for a NULL pointer or a non-positive size before any HIP call, and INC_ERR_UNSUPPORTED (nothing launched) for
 * anything they do not take -- the caller then runs the eager ops.  Every pointer must be 16-byte aligned.
 * inc_fwd_silu_mul: out[i] = DT(float(DT(g / (1 + expf(-g)))) * float(up[i])), g = float(gate[i]); n contiguous elements, any n.
 * inc_fwd_rope: q [B, Hq, T, D], k [B, Hk, T, D] (Hk may differ: GQA), cos / sin contiguous [cs_batch, T, D] with cs_batch 1 or B;
 *   out[.., d] = DT(DT(x[d] * cos[d]) + DT(r[d] * sin[d])), r[d] = -x[d + D/2] for d < D/2, else x[d - D/2].  `strides`: HOST array
 *   of 12 element strides, (b, h, t) of q, k, q_out, k_out in that order (the d stride is 1); each a non-negative multiple of 8.
 *   INC_ERR_UNSUPPORTED unless D % 16 == 0 and B * T * (Hq + Hk) * D / 16 < 2^31.  D / 16 a power of two up to 64 (D = 16 .. 1024) runs
 *   the walker (a wave per token, cos / sin pieces held in registers across the heads), any other D one lane per 16-byte piece.
 * inc_fwd_rmsnorm: LlamaRMSNorm.forward on row-major contiguous x [rows, cols], weight [cols]:
 *   out = DT(float(w) * float(DT(float(x) * rsqrt(mean(float(x)^2) + eps)))), the mean summed in the order of torch's reduction
 *   kernel for this shape (fwd_elementwise.hip).  INC_ERR_UNSUPPORTED unless rows >= 8, cols % 8 == 0 and 256 <= cols <= 16384:
 *   torch reduces other shapes in another order.                                                                             */
int inc_fwd_silu_mul(const void* gate, const void* up, void* out, int64_t n, int dtype, inc_stream_t stream);
int inc_fwd_rope(const void* q, const void* k, const void* cos, const void* sin, void* q_out, void* k_out, int64_t B, int64_t Hq,
                 int64_t Hk, int64_t T, int64_t D, const int64_t* strides, int64_t cs_batch, int dtype, inc_stream_t stream);
int inc_fwd_rmsnorm(const void* x, const void* w, void* out, int64_t rows, int64_t cols, float eps, int dtype, inc_stream_t stream);
/* inc_probe_round16: out[i] = DT(in[i]) for n fp32 values through the rounding helper of the three kernels above (pair-wise hardware
 *   conversion for bf16 with torch's NaN rule -- every NaN becomes 0x7FC0 --, the hardware conversion for fp16), so that the helper can
 *   be compared with torch's own `.to(dtype)` over every fp32 bit pattern.  `in` and `out` 16-byte aligned, any n > 0.           */
int inc_probe_round16(const float* in, uint16_t* out, int64_t n, int dtype, inc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* INC_MI355X_H_ */
