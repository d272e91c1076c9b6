"""torch-tensor front ends of the glue kernels in include/pafc_encoder_ops.h (GPU only, no fallback)."""
import contextlib
import ctypes
import math
import os
import threading
import weakref
from typing import List, Optional

import torch

from . import _lib
from ._lib import c_int, c_void_p
from .utils import graph_step


# ---- dispatch thresholds: ONE table ---------------------------------------------------------------------------------------
# Which kernel family serves a projection depends on how many rows it has.  Every threshold lives here, with the record that
# justifies it; `PAFC_DISPATCH="name=value,name=value"` overrides any of them for A/B runs (the per-name variables of earlier
# rounds -- PAFC_OWN_GEMM_MIN_ROWS, PAFC_LDS_RESIDENT_MIN_ROWS, PAFC_SPLIT_GEMM_MIN_ROWS, PAFC_SKINNY_MAX_ROWS -- are still
# read).  bench.py sets none of them: what it measures is this table.
#
#   name                   default  meaning, and where the number comes from
#   skinny_max_rows            640  bf16 projections of a streaming chunk step with at most this many rows run on
#                                   csrc/gemm_skinny.hip (one launch on the ~4.7 us floor).  8 streams x 78 rows still win over
#                                   tiled kernels, 16 lose: profiles/r03g_streaming_streams_vs_few_rows_limit.txt
#   own_gemm_min_rows            1  bf16 projections with at least this many rows (that are not few-rows launches) run on the
#                                   hand-written tiled GEMMs (gemm_ph.hip 256-wide tiles when they fill the chip, else
#                                   gemm_bf16.hip 128 x 128 / 128 x 64 / 64 x 64).  Was 8192 while the small kernel only had
#                                   128 x 128 tiles; with the tile variants it ties or beats the library's picks from 1 024
#                                   rows up on every layer shape but w_2 (K = 2048: 14.5 vs 10.5 us at 1 024 rows, 20.7 vs
#                                   17.4 at 3 992) and wins the stacked r/k/v product by 5-7 us:
#                                   profiles/r04d_gemm_mid_rows_own_tiles_vs_library.txt.  No library GEMM is left in a bf16 pass.
#   lds_resident_min_rows     8192  the one-pass LoRA kernels (128 KiB of weights staged into LDS per block) from this many
#                                   rows on, below it shift/lerp + small GEMMs; the chunk step always takes the one-pass
#                                   kernels (fewer launches).  At 3 992 rows the one-pass down-projection takes 27.6 us
#                                   against 6.0 + 6.5 for the two small kernels (profiles/r04e_windows_2000x8_kernels_*.txt);
#                                   a c2 pass measured 2048 / 4096 / 8192 within 1 % (profiles/r03c_bench_c2_knobs.txt)
#   split_gemm_min_rows       1024  fp32 activations of a model with the bf16 slot on the bf16 matrix cores as hi + lo planes
#                                   (3 MFMAs per product, ~2^-16 relative) from this many rows on; below it exact fp32
#                                   products on the fp32 matrix cores (csrc/gemm_f32.hip; pure-fp32 models -- rwkv_do_bfloat16:
#                                   False, the 1e-3 parity bar -- always take those; until round 6 these were library GEMMs).  Was 16384 until round 5: at 1 536 - 24 000 rows the split kernel at its best
#                                   tile height takes 28 / 35 / 48 / 78 / 90 / 138 us for w_1 where the library takes 37 / 76 /
#                                   137 / 256 / 273 / 507 (profiles/r05_split_mid_rows.txt; only w_2 below 4 000 rows is faster
#                                   on the library, 32-74 vs 72-74 us): 2 000-frame windows x 8 20 600 -> 33 200 audio-sec/sec,
#                                   c2 in this precision 44 200; DESIGN section 4 "split operands"
#   ln_fold_min_rows         24576  unmasked bf16 inputs of at least this many rows take the schedule with three LayerNorms
#                                   folded into the 256-wide GEMMs either side of them (needs full grids of 256 x 256 tiles:
#                                   3 x the row count at which they fill the chip): profiles/r03d / r03e
#   dwconv_ln_silu_max_rows  24575  up to this many rows the conv module's LayerNorm + SiLU is the depthwise convolution's epilogue
#                                   (one launch and one round trip less per layer: c2 +0.4-2 %, 2 000-frame windows +1.3 %, same box);
#                                   the 30-minute sequence measured the same or 0.2 ms slower with it (the convolution kernel is
#                                   latency-bound at two waves per SIMD and the epilogue's two block reductions add to that), so
#                                   long inputs keep the two kernels
#   split_small_max_rows      8192  split-operand (and bf16 -> fp32) products of at most this many rows AND at most 2^22 outputs
#                                   (w_1, N = 2048: 2 048 rows) run on the small tiles of csrc/gemm_bf16.hip
#                                   (pafc_gemm_bf16_f32out: 64 x 64 / 128 x 64 tiles, three-stage ring) instead of the 256-wide
#                                   phase-pipelined kernel, whose tiles cost ~25 us (K = 512) / ~72 us (K = 2048) each however few
#                                   there are: at 3 992 rows 17 / 21 / 53 us against 27 / 28 / 72 for pointwise_conv2 / pointwise_conv1
#                                   / w_2, w_1 22.7 against 30.5 at 1 996 rows and 37.5 against 30.4 at 2 500.  Round 6, late: 8 192
#                                   (N = 512 products; long-K ones on 128 x 128 tiles with 2-4 K shares per tile: w_2 76.9 -> 49.3 us at
#                                   5 000 rows, 82.5 -> 66.0 at 7 984: profiles/r06z_split_small_tile_variants.txt)
#                                   (profiles/r06n_split_small_rows.txt)
#   split_layers_min_rows      256  the LAYERS of a model with the bf16 slot take the split-operand schedule
#                                   (fused.layer_forward_split) from this many rows on -- since round 6 also below
#                                   split_gemm_min_rows, where their projections run on the small tiles (a single 2 000-frame
#                                   window is 499 rows: exact fp32 products on the fp32 matrix cores cost 12-55 us each there)
#   ktail_min_k              2048  split-operand fp32-output products whose last round of 256 x 256 tiles covers at most half of the
#                                   CUs run that round's row tiles once per half of K plus a fix-up pass (_ph_ktail_plan,
#                                   pafc_gemm_ph_ktail) from this K on.  44 998 rows x N = 512 (352 tiles on 256 CUs), one launch
#                                   -> three, residual form / plain form: K = 1024 162 -> 167 / 134 -> 146 us, 1536 218 -> 214 /
#                                   189 -> 194, 2048 265 -> 257 / 241 -> 240, 4096 475 -> 447 / 455 -> 430, 9728 1085 -> 963 /
#                                   1082 -> 952 (profiles/gemm_ph_ktail_shapes.jsonl; DESIGN "K-split of the last partial round")
# C side (csrc/gemm_bf16.hip): which GEMM family takes a problem is decided by rounds -- the 128-wide kernel while its 128 x 128
# tiles fit one round of two per CU, the 256-wide phase-pipelined kernel beyond (profiles/r04s_gemm_tile_choice_by_rows.txt);
# PAFC_PH_MIN_FILL=<percent> (round 3's rule: 256-wide tiles must cover that share of the CUs) and PAFC_GEMM_TILE (force a tile
# of the small kernel) are A/B switches of the kernels themselves.
DISPATCH = dict(skinny_max_rows=640, own_gemm_min_rows=1, lds_resident_min_rows=8192, split_gemm_min_rows=1024,
                ln_fold_min_rows=24576, dwconv_ln_silu_max_rows=24575, split_small_max_rows=8192, split_layers_min_rows=256,
                ktail_min_k=2048)


def _load_dispatch():
    legacy = dict(skinny_max_rows="PAFC_SKINNY_MAX_ROWS", own_gemm_min_rows="PAFC_OWN_GEMM_MIN_ROWS",
                  lds_resident_min_rows="PAFC_LDS_RESIDENT_MIN_ROWS", split_gemm_min_rows="PAFC_SPLIT_GEMM_MIN_ROWS")
    for name, env in legacy.items():
        if os.environ.get(env):
            DISPATCH[name] = int(os.environ[env])
    for item in filter(None, os.environ.get("PAFC_DISPATCH", "").split(",")):
        name, _, value = item.partition("=")
        if name.strip() not in DISPATCH:
            raise ValueError(f"PAFC_DISPATCH: unknown threshold {name!r} (known: {sorted(DISPATCH)})")
        DISPATCH[name.strip()] = int(value)


_load_dispatch()


def train_gemms_own() -> bool:
    """PAFC_TRAIN_OWN_GEMMS=0: forward and input-gradient products of the training step's nn.Linear go to the library (A/B)."""
    return os.environ.get("PAFC_TRAIN_OWN_GEMMS", "1") != "0"


def train_kernels_enabled() -> bool:
    """PAFC_TRAIN_KERNELS=0: the training step differentiates through the framework's own operators (A/B measurements)."""
    import os
    return os.environ.get("PAFC_TRAIN_KERNELS", "1") != "0"


def _conv_rows_ld(x: torch.Tensor, who: str) -> int:
    """Row stride (elements) of a convolution input x (B, T, C'): contiguous, or a column slice of a wider (B, T, W) buffer --
    unit channel stride, frames x.stride(1) apart, sequences T frames apart, a channel pair aligned."""
    if not x.is_cuda:
        raise _lib.PafcError("this op runs on the MI355X only (tensor is on %s); there is no CPU fallback" % x.device)
    if x.is_contiguous():
        return x.shape[-1]
    if x.dim() != 3 or x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1) or x.stride(1) < x.shape[2] or x.stride(1) % 2 \
            or x.data_ptr() % (2 * x.element_size()):
        raise _lib.PafcError(f"{who}: x (B, T, C) with unit channel stride, rows of one even stride, an aligned channel pair")
    return x.stride(1)


def depthwise_conv1d_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], left_pad: int,
                        out_len: int, glu: bool = False, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Channels-last depthwise conv1d: x (B, T, C) [or (B, T, 2C) with glu], weight (C, 1, K) -> (B, out_len, C).  x may be a
    column slice of a wider buffer (_conv_rows_ld); any other layout is refused."""
    _lib.require_gpu(weight, bias, lens)
    ldx = _conv_rows_ld(x, "depthwise_conv1d_cl")
    B, T, Cx = x.shape
    C = Cx // 2 if glu else Cx
    K = weight.shape[-1]
    if weight.shape != (C, 1, K) or weight.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise _lib.PafcError("depthwise weight must be (C, 1, K) in the activation dtype")
    if lens is not None and lens.dtype != torch.int32:
        raise _lib.PafcError("lens must be int32")
    y = torch.empty(B, out_len, C, dtype=x.dtype, device=x.device)
    rc = _lib.lib().pafc_dwconv1d_cl_ex(_lib.dtype_code(x.dtype), B, T, C, K, left_pad, out_len, _lib.ptr(x), ldx,
                                        _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), int(glu), _lib.ptr(lens),
                                        _lib.stream_of(x))
    _lib.check(rc, "pafc_dwconv1d_cl")
    return y


def dwconv_ln_silu_ok(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Does the convolution kernel carry the conv module's LayerNorm + SiLU for this input (bf16, 512 channels, k = 15 / 31)?"""
    return (x.numel() // x.shape[-1] <= DISPATCH["dwconv_ln_silu_max_rows"] and x.dtype == torch.bfloat16 and x.is_cuda
            and x.shape[-1] == 512 and weight.shape[-1] in (15, 31))


def depthwise_conv1d_cl_ln_silu(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], left_pad: int, out_len: int,
                                gamma: torch.Tensor, beta: torch.Tensor, eps: float, lens: Optional[torch.Tensor] = None):
    """SiLU(LayerNorm(depthwise_conv1d_cl(x, ...))) in one pass (convolution.py:131-138 with cnn_module_norm: layer_norm): the
    convolution's epilogue normalises its own rows.  x (B, T, 512) bf16, weight (512, 1, K), K in {15, 31}."""
    _lib.require_gpu(weight, bias, gamma, beta, lens)
    ldx = _conv_rows_ld(x, "depthwise_conv1d_cl_ln_silu")
    B, T, C = x.shape
    K = weight.shape[-1]
    if not dwconv_ln_silu_ok(x, weight) or weight.shape != (C, 1, K) or any(
            t is not None and (t.dtype != x.dtype or not t.is_contiguous()) for t in (weight, bias, gamma, beta)):
        raise _lib.PafcError("depthwise_conv1d_cl_ln_silu: bf16, C = 512, K in (15, 31), contiguous parameters in the activation dtype")
    if lens is not None and lens.dtype != torch.int32:
        raise _lib.PafcError("lens must be int32")
    L = _lib.lib()
    y = torch.empty(B, out_len, C, dtype=x.dtype, device=x.device)
    rc = L.pafc_dwconv1d_cl_ln_silu(_lib.dtype_code(x.dtype), B, T, C, K, left_pad, out_len, _lib.ptr(x), ldx, _lib.ptr(weight),
                                    _lib.ptr(bias), _lib.ptr(gamma), _lib.ptr(beta), float(eps), _lib.ptr(y), _lib.ptr(lens),
                                    _lib.stream_of(x))
    _lib.check(rc, "pafc_dwconv1d_cl_ln_silu")
    return y


def depthwise_conv1d_cl_wgrad(x: torch.Tensor, dy: torch.Tensor, K: int, left_pad: int, want_bias: bool = True):
    """(dw (C, 1, K), dbias (C) or None) in float32 for y = depthwise_conv1d_cl(x, w, bias, left_pad, dy.shape[1])."""
    _lib.require_gpu(dy)
    ldx = _conv_rows_ld(x, "depthwise_conv1d_cl_wgrad")
    B, T, C = x.shape
    if dy.shape[0] != B or dy.shape[2] != C or dy.dtype != x.dtype:
        raise _lib.PafcError("dy must be contiguous (B, T_out, C) in x's dtype")
    L = _lib.lib()
    nbytes = L.pafc_dwconv1d_cl_wgrad_workspace_bytes(B, dy.shape[1], C, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    dw = torch.empty(C, 1, K, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device) if want_bias else None
    rc = L.pafc_dwconv1d_cl_wgrad(_lib.dtype_code(x.dtype), B, T, C, K, left_pad, dy.shape[1], _lib.ptr(x), ldx,
                                  _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes, _lib.stream_of(x))
    _lib.check(rc, "pafc_dwconv1d_cl_wgrad")
    return dw, db


class _DepthwiseConvCL(torch.autograd.Function):
    """Autograd over the channels-last depthwise convolution: dx is the forward kernel on dy with the taps reversed and
    left_pad' = K - 1 - left_pad, dw / dbias the reduction kernel (what autograd derives for nn.Conv1d,
    convolution.py:131)."""

    @staticmethod
    def forward(ctx, x, weight, bias, left_pad, out_len):
        # parameters in the activation dtype (what autocast does for nn.Conv1d); the cast sits inside the Function so that the
        # gradients come back in the parameters' own dtype without a cast node each, and bf16 takes the kept copies
        w = _param_as(weight, x.dtype)
        b = None if bias is None else _param_as(bias, x.dtype)
        ctx.save_for_backward(x, w)
        ctx.left_pad, ctx.has_bias = left_pad, bias is not None
        ctx.w_dtype, ctx.b_dtype = weight.dtype, (None if bias is None else bias.dtype)
        return depthwise_conv1d_cl(x, w, b, left_pad, out_len)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        K = weight.shape[-1]
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = depthwise_conv1d_cl(dy, weight.flip(-1).contiguous(), None, K - 1 - ctx.left_pad, x.shape[1])
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = depthwise_conv1d_cl_wgrad(x, dy, K, ctx.left_pad, want_bias=ctx.has_bias)
            dw = dw.to(ctx.w_dtype)
            db = db.to(ctx.b_dtype) if db is not None else None
        return dx, dw, db, None, None


def depthwise_conv1d_cl_autograd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], left_pad: int,
                                 out_len: int) -> torch.Tensor:
    """Training-side entry: parameters are cast to the activation dtype (what autocast does for nn.Conv1d), gradients
    come back in the parameters' dtype."""
    return _DepthwiseConvCL.apply(x.contiguous(), weight, bias, left_pad, out_len)


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, eps: float, dx_add: Optional[torch.Tensor] = None):
    """(dx in x's dtype, dgamma, dbeta in float32) of y = LayerNorm(x) over the last axis; dx_add (like x): added to dx in the same
    pass (the gradient that reaches x past the norm)."""
    _lib.require_gpu(x, dy, gamma, dx_add)
    if dx_add is not None and (dx_add.dtype != x.dtype or dx_add.shape != x.shape or not dx_add.is_contiguous()):
        raise _lib.PafcError("layernorm_bwd: dx_add contiguous, shaped and typed like x")
    C = x.shape[-1]
    rows = x.numel() // C
    if dy.shape != x.shape or gamma.dtype != x.dtype or gamma.shape != (C,):
        raise _lib.PafcError("layernorm_bwd: dy shaped like x, gamma (C) in x's dtype")
    L = _lib.lib()
    nbytes = L.pafc_layernorm_bwd_workspace_bytes(rows, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x)
    dgb = torch.empty(2, C, dtype=torch.float32, device=x.device)
    rc = L.pafc_layernorm_bwd_add(_lib.dtype_code(x.dtype), _lib.dtype_code(dy.dtype), rows, C, _lib.ptr(x), _lib.ptr(dy),
                                  _lib.ptr(gamma), float(eps), _lib.ptr(dx_add), _lib.ptr(dx), _lib.ptr(dgb), _lib.ptr(ws), nbytes,
                                  _lib.stream_of(x))
    _lib.check(rc, "pafc_layernorm_bwd")
    return dx, dgb[0], dgb[1]


class _LayerNormTrain(torch.autograd.Function):
    """nn.LayerNorm for the GPU training step: forward = the inference kernel (one pass, optionally straight to bf16 for
    a consumer that would cast anyway), backward = one pass over (x, dy) + a small reduction, instead of the framework's
    fp32 forward, cast and three backward kernels.  with_skip (round 6): x is handed on as a second output -- the residual
    path of a pre-norm branch, x + f(norm(x)) -- so that its gradient comes back HERE and is added inside the backward
    kernel (pafc_layernorm_bwd_add) instead of by autograd's accumulation pass (one (B, T, C) fp32 add per branch)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype, with_skip=False):
        g, b = _param_as(weight, x.dtype), _param_as(bias, x.dtype)
        _, y, _ = add_layernorm(x, None, 1.0, g, b, out_dtype=out_dtype, want_x=False, eps=eps)
        ctx.save_for_backward(x, g)
        ctx.eps, ctx.w_dtype, ctx.b_dtype = eps, weight.dtype, bias.dtype
        return (y, x.view_as(x)) if with_skip else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, g = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(x)
        if dskip is not None and (dskip.dtype != x.dtype or not dskip.is_contiguous()):
            dskip = dskip.to(x.dtype).contiguous()
        dx, dg, db = layernorm_bwd(x, dy.contiguous(), g, ctx.eps, dx_add=dskip)
        if ctx.w_dtype == ctx.b_dtype and ctx.w_dtype != torch.float32:
            dgb = dg._base.to(ctx.w_dtype)          # (2, C): one cast for both (the bf16 ln_x of the slot)
            return dx, dgb[0], dgb[1], None, None, None
        return dx, dg.to(ctx.w_dtype), db.to(ctx.b_dtype), None, None, None


class _LnSiluTrain(torch.autograd.Function):
    """silu(LayerNorm(x)) of the conv module (convolution.py:136-138) for the GPU training step as one kernel each way
    (pafc_layernorm_silu_fwd / _bwd): x -- the depthwise convolution's bf16 output -- in, bf16 out, fp32 arithmetic against the
    norm's own parameters.  Under bf16 autocast the framework chain is cast, LayerNorm (fp32), SiLU, cast -- four passes over
    (B, T, C) forward and four more backward for the same values."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        L = _lib.lib()
        C = x.shape[-1]
        rows = x.numel() // C
        g, b = weight.detach().contiguous(), bias.detach().contiguous()
        y = torch.empty_like(x)
        _lib.check(L.pafc_layernorm_silu_fwd(_lib.dtype_code(x.dtype), _lib.dtype_code(g.dtype), rows, C, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b),
                                             float(eps), _lib.ptr(y), _lib.stream_of(x)), "pafc_layernorm_silu_fwd")
        ctx.save_for_backward(x, g, b)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, b = ctx.saved_tensors
        L = _lib.lib()
        C = x.shape[-1]
        rows = x.numel() // C
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        nbytes = L.pafc_layernorm_bwd_workspace_bytes(rows, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        dx = torch.empty_like(x)
        dgb = torch.empty(2, C, dtype=torch.float32, device=x.device)
        _lib.check(L.pafc_layernorm_silu_bwd(_lib.dtype_code(x.dtype), _lib.dtype_code(g.dtype), rows, C, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(g),
                                             _lib.ptr(b), float(ctx.eps), _lib.ptr(dx), _lib.ptr(dgb), _lib.ptr(ws), nbytes, _lib.stream_of(x)),
                   "pafc_layernorm_silu_bwd")
        if g.dtype != torch.float32:
            dgb = dgb.to(g.dtype)
        return dx, dgb[0], dgb[1], None


def ln_silu_train_eligible(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor]) -> bool:
    """The conv module's LayerNorm + SiLU as one kernel each way: GPU training step, x contiguous bf16 (fp32 or bf16 parameters) or
    fp32 (fp32 parameters), C % 8 == 0, C <= 1024.  PAFC_TRAIN_LN_SILU=0: the separate LayerNorm and SiLU (A/B runs)."""
    if not (x.is_cuda and torch.is_grad_enabled() and weight is not None and bias is not None and train_kernels_enabled()
            and os.environ.get("PAFC_TRAIN_LN_SILU", "1") != "0"):
        return False
    if weight.dtype != bias.dtype or x.shape[-1] % 8 or x.shape[-1] > 1024 or not (x.requires_grad or weight.requires_grad):
        return False
    return ((x.dtype == torch.bfloat16 and weight.dtype in (torch.float32, torch.bfloat16))
            or (x.dtype == torch.float32 and weight.dtype == torch.float32))


def ln_silu_train(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    return _LnSiluTrain.apply(x.contiguous(), weight, bias, eps)


def layer_norm_train_eligible(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor]) -> bool:
    return (x.is_cuda and torch.is_grad_enabled() and weight is not None and bias is not None and train_kernels_enabled()
            and x.dtype in (torch.float32, torch.bfloat16) and x.shape[-1] % 8 == 0 and x.shape[-1] <= 1024
            and (x.requires_grad or weight.requires_grad))


def layer_norm_with_skip(x: torch.Tensor, weight, bias, eps: float, bf16_out: bool = False):
    """(LayerNorm(x), x) for a pre-norm residual branch x + f(norm(x)) in the GPU training step: use the SECOND value as the
    branch's residual input and its gradient is added inside the norm's backward kernel (see _LayerNormTrain).  None when the
    kernels do not take the call (the caller then norms and adds as usual)."""
    if not (layer_norm_train_eligible(x, weight, bias) and x.requires_grad and os.environ.get("PAFC_TRAIN_LN_SKIP", "1") != "0"):
        return None
    amp = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
    if amp and x.dtype == torch.bfloat16 and weight.dtype == torch.float32:
        return None                       # (autocast would run this norm in fp32 on a cast copy: not the residual stream itself)
    out_dtype = torch.bfloat16 if (bf16_out and amp) else x.dtype
    return _LayerNormTrain.apply(x.contiguous(), weight, bias, eps, out_dtype, True)


def layer_norm(x: torch.Tensor, weight, bias, eps: float, bf16_out: bool = False) -> torch.Tensor:
    """F.layer_norm over the last axis as the modules call it; in the GPU training step the kernels above.  bf16_out:
    the consumer is a projection that autocast would feed bf16 anyway -- under bf16 autocast the fp32 norm then writes
    bf16 directly (same values as the framework's fp32 result cast by the consumer)."""
    if layer_norm_train_eligible(x, weight, bias):
        amp = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
        if amp and x.dtype == torch.bfloat16 and weight.dtype == torch.float32:
            x = x.float()                 # autocast runs layer_norm in fp32
        out_dtype = torch.bfloat16 if (bf16_out and amp) else x.dtype
        return _LayerNormTrain.apply(x.contiguous(), weight, bias, eps, out_dtype, False)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def gemm_tn(dy: torch.Tensor, x: torch.Tensor, out_dtype: torch.dtype = torch.float32, want_bias: bool = False):
    """dw (M, N) = dy^T @ x for dy (R, M), x (R, N) bf16 with unit column stride: nn.Linear's weight gradient;
    with want_bias also db (M) = dy.sum(0) from the same pass -> (dw, db).  dy (Z, R, M), x (Z, R, N): Z products in one launch
    pair -> dw (Z, M, N) (db (Z, M))."""
    if not (dy.is_cuda and x.is_cuda):
        raise _lib.PafcError("gemm_tn runs on the MI355X only; there is no CPU fallback")
    batched = dy.dim() == 3
    Z = dy.shape[0] if batched else 1
    R, M = dy.shape[-2], dy.shape[-1]
    N = x.shape[-1]
    if (dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or x.dim() != dy.dim() or x.shape[-2] != R or dy.stride(-1) != 1
            or x.stride(-1) != 1 or out_dtype not in (torch.float32, torch.bfloat16) or (batched and x.shape[0] != Z)):
        raise _lib.PafcError("gemm_tn: dy (R, M) and x (R, N) bf16 with unit column stride (or both with a leading batch); fp32 or bf16 output")
    L = _lib.lib()
    nbytes = L.pafc_gemm_tn_batched_workspace_bytes(R, M, N, Z)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    dw = torch.empty((Z, M, N) if batched else (M, N), dtype=out_dtype, device=dy.device)
    db = (torch.empty((Z, M) if batched else (M,), dtype=out_dtype, device=dy.device)) if want_bias else None
    rc = L.pafc_gemm_tn_bf16_batched(R, M, N, Z, _lib.ptr(dy), dy.stride(-2), dy.stride(0) if batched else 0, _lib.ptr(x), x.stride(-2),
                                     x.stride(0) if batched else 0, _lib.ptr(dw), _lib.ptr(db), _lib.dtype_code(out_dtype), _lib.ptr(ws),
                                     nbytes, _lib.stream_of(dy))
    _lib.check(rc, "pafc_gemm_tn_bf16")
    return (dw, db) if want_bias else dw


# ---- element-wise groups of the training step (csrc/train_elementwise.hip) ------------------------------------------------
_dropout_calls = 0       # fallback counter when the device generator exposes no offset


def _next_dropout_stream(device=None):
    """(seed, call index) of the next keep mask, drawn from torch's generator of the device: seed = its seed, index = its Philox
    offset, which is advanced by one step of four like any framework dropout.  `torch.manual_seed` therefore restarts the
    sequence, and an activation-checkpoint recompute -- which restores the device RNG state (`preserve_rng_state`) -- draws the
    masks of the original forward pass again (a process-wide counter would not)."""
    global _dropout_calls
    try:
        idx = device.index if device is not None and device.index is not None else torch.cuda.current_device()
        g = torch.cuda.default_generators[idx]
        off = int(g.get_offset())
        g.set_offset(off + 4)
        return int(g.initial_seed()) & 0xFFFFFFFFFFFFFFFF, off // 4 + 1
    except (RuntimeError, IndexError, AttributeError):
        _dropout_calls += 1
        return int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF, _dropout_calls


class _ResidualDropout(torch.autograd.Function):
    """out = x + scale * dropout(y, p): one kernel; backward dx = dout (no kernel), dy = one kernel, mask recomputed."""

    @staticmethod
    def forward(ctx, x, y, scale, p):
        L = _lib.lib()
        x, y = x.contiguous(), y.contiguous()
        seed, off = _next_dropout_stream(x.device) if p > 0 else (0, 0)
        out = torch.empty_like(x)
        _lib.check(L.pafc_residual_dropout(0, _lib.dtype_code(x.dtype), _lib.dtype_code(y.dtype), x.numel(), _lib.ptr(x), _lib.ptr(y),
                                           _lib.ptr(out), float(scale), float(p), seed, off, _lib.stream_of(x)), "pafc_residual_dropout")
        ctx.meta = (float(scale), float(p), seed, off, y.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        scale, p, seed, off, ydt = ctx.meta
        dy = None
        if ctx.needs_input_grad[1]:
            L = _lib.lib()
            g = g.contiguous()
            dy = torch.empty(g.shape, dtype=ydt, device=g.device)
            _lib.check(L.pafc_residual_dropout(1, _lib.dtype_code(g.dtype), _lib.dtype_code(ydt), g.numel(), _lib.ptr(g), _lib.ptr(None),
                                               _lib.ptr(dy), scale, p, seed, off, _lib.stream_of(g)), "pafc_residual_dropout")
        return (g if ctx.needs_input_grad[0] else None), dy, None, None


class _SiluDropout(torch.autograd.Function):
    """dropout(silu(h), p): one kernel forward, one backward (from h and the recomputed mask; silu(h) is not kept)."""

    @staticmethod
    def forward(ctx, h, p):
        L = _lib.lib()
        h = h.contiguous()
        seed, off = _next_dropout_stream(h.device) if p > 0 else (0, 0)
        out = torch.empty_like(h)
        _lib.check(L.pafc_silu_dropout(0, _lib.dtype_code(h.dtype), h.numel(), _lib.ptr(h), _lib.ptr(None), _lib.ptr(out), float(p), seed, off,
                                       _lib.stream_of(h)), "pafc_silu_dropout")
        ctx.save_for_backward(h)
        ctx.meta = (float(p), seed, off)
        return out

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        p, seed, off = ctx.meta
        L = _lib.lib()
        g = g.contiguous()
        dh = torch.empty_like(h)
        _lib.check(L.pafc_silu_dropout(1, _lib.dtype_code(h.dtype), h.numel(), _lib.ptr(h), _lib.ptr(g), _lib.ptr(dh), p, seed, off,
                                       _lib.stream_of(h)), "pafc_silu_dropout")
        return dh, None


def train_elementwise_eligible(x: torch.Tensor, y: Optional[torch.Tensor] = None) -> bool:
    """The fused element-wise training kernels serve this call: GPU training step with the hand-written kernels on, fp32 or
    bf16 contiguous-izable tensors whose size is a multiple of 8 (a 512-wide stream always is)."""
    if not (train_kernels_enabled() and x.is_cuda and torch.is_grad_enabled() and x.numel() % 8 == 0 and x.numel() > 0):
        return False
    # the kernels want 16-byte aligned pointers: a contiguous view at an odd storage offset keeps the framework's operators
    # (a non-contiguous tensor is copied into a fresh, aligned allocation by the Function)
    for t in (x, y):
        if t is not None and t.is_contiguous() and t.data_ptr() % 16:
            return False
    pairs = {(torch.float32, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)}
    if y is not None:
        return (x.dtype, y.dtype) in pairs and y.shape == x.shape and y.is_cuda
    return x.dtype in (torch.float32, torch.bfloat16)


def residual_dropout(x: torch.Tensor, y: torch.Tensor, scale: float, p: float, training: bool) -> torch.Tensor:
    """x + scale * dropout(y, p) (encoder_layer.py:205-255) as one kernel forward and one backward in the GPU training step;
    the framework's operators otherwise."""
    p = float(p) if training else 0.0
    if train_elementwise_eligible(x, y) and (x.requires_grad or y.requires_grad):
        return _ResidualDropout.apply(x, y, float(scale), p)
    d = torch.nn.functional.dropout(y, p, training=training) if p > 0 else y
    return x + (d if scale == 1.0 else scale * d)


def silu_dropout(h: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    """dropout(silu(h), p) (positionwise_feed_forward.py:47-55) as one kernel forward and one backward in the GPU training step."""
    p = float(p) if training else 0.0
    if train_elementwise_eligible(h) and h.requires_grad:
        return _SiluDropout.apply(h, p)
    a = torch.nn.functional.silu(h)
    return torch.nn.functional.dropout(a, p, training=training) if p > 0 else a


# bf16 copies of fp32 master weights for the training step.  Under autocast every projection casts its weight and bias on
# every step (~400 small launches).  Inside `with train_shadows():` (utils.train_utils.train_step wraps the forward pass in
# it) the copy is kept beside the parameter and ALL copies are brought up to date by one multi-tensor copy when the context
# is entered -- unconditionally: fused optimizers update parameters without touching Tensor._version, so nothing cheaper can
# tell a stale copy.  Outside the context every use casts, as before.
_shadows = {}      # id(parameter) -> [weak reference to the parameter, bf16 copy]  (tensors compare element-wise: they cannot
                   # be keys of a WeakKeyDictionary)
_shadows_on = False
_wgroups = {}     # (id(p0), id(p1), ...) -> [weak references, (Z, N, K) bf16 copy]: equally shaped weights as ONE batched operand


def _param_of(p: torch.Tensor) -> torch.Tensor:
    """The parameter behind a reshaping view of it (a 1 x 1 convolution's `weight.squeeze(-1)`: a new tensor object on every
    call, which a registry keyed by object identity would never find again), else the tensor itself."""
    b = getattr(p, "_base", None)
    if b is not None and isinstance(b, torch.nn.Parameter) and b.numel() == p.numel() and b.is_contiguous() and p.is_contiguous():
        return b
    return p


def _bf16_shadow(p: torch.Tensor) -> torch.Tensor:
    if p.dtype == torch.bfloat16:
        return p
    if not _shadows_on:
        return p.to(torch.bfloat16)
    base = _param_of(p)
    if base is not p:
        return _bf16_shadow(base).view(p.shape)
    ent = _shadows.get(id(p))
    if ent is not None and ent[0]() is p and ent[1].device == p.device and ent[1].shape == p.shape:
        return ent[1]                                # refreshed when the context was entered
    sh = p.detach().to(torch.bfloat16)
    _shadows[id(p)] = [weakref.ref(p), sh]
    return sh


def _param_as(p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """A parameter in the dtype a training kernel wants (no autograd through the cast: callers sit inside Functions)."""
    if p.dtype == dtype:
        return p.detach()
    if dtype == torch.bfloat16 and p.dtype == torch.float32 and isinstance(p, torch.nn.Parameter):
        return _bf16_shadow(p).detach()
    return p.detach().to(dtype)


_shadows_t = {}    # id(parameter) -> [weak reference, bf16 copy of the TRANSPOSED matrix (K, N), (param epoch, version) of the copy]
_tr_table = None   # {device: (signature, device table of pafc_multi_transpose_bf16 descriptors, n, total tiles)}


def _bf16_shadow_t(w: torch.Tensor) -> torch.Tensor:
    """bf16 (K, N) copy of a weight (N, K) -- a parameter or a reshaping view of one -- for the input-gradient GEMM dX = dY W.
    The copies live beside their parameters; ALL of them are refreshed by ONE launch when train_shadows() is entered
    (pafc_multi_transpose_bf16) and stamped with the parameter epoch and the parameter's in-place version: a copy whose stamp is
    not the present one (a backward pass outside train_step, an update behind the registry's back) is re-made on the spot."""
    global _tr_table
    N, K = w.shape
    p = _param_of(w)
    stamp = (_param_epoch, p._version)
    ent = _shadows_t.get(id(p))
    if ent is not None and ent[0]() is p and ent[1].device == p.device and tuple(ent[1].shape) == (K, N):
        if ent[2] != stamp:
            with torch.no_grad():
                ent[1].copy_(p.detach().view(N, K).t())
            ent[2] = stamp
        return ent[1]
    if not isinstance(p, torch.nn.Parameter):
        return w.detach().t().to(torch.bfloat16).contiguous()     # not a parameter: nothing to keep it beside
    sh = p.detach().view(N, K).t().to(torch.bfloat16).contiguous()
    _shadows_t[id(p)] = [weakref.ref(p), sh, stamp]
    _tr_table = None
    return sh


def _refresh_transposed_shadows() -> None:
    """One pafc_multi_transpose_bf16 launch per DEVICE that holds registered parameters (descriptor table and launch on that
    device, on its current stream)."""
    global _tr_table
    by_dev = {}
    for key in list(_shadows_t):
        p = _shadows_t[key][0]()
        sh = _shadows_t[key][1]
        if (p is None or sh.device != p.device or sh.numel() != p.numel() or p.dtype not in (torch.float32, torch.bfloat16)
                or not p.is_contiguous()):
            del _shadows_t[key]
            _tr_table = None
        else:
            by_dev.setdefault(p.device, []).append((p, sh))
            _shadows_t[key][2] = (_param_epoch, p._version)
    if not by_dev:
        return
    if _tr_table is None:
        _tr_table = {}
    L = _lib.lib()
    for dev, live in by_dev.items():
        sig = tuple((p.data_ptr(), sh.data_ptr(), p.dtype) for p, sh in live)
        ent = _tr_table.get(dev)
        if ent is None or ent[0] != sig:
            rows, t0 = [], 0
            for p, sh in live:
                k_, n_ = sh.shape                  # the copy is (K, N); the parameter (N, K) or a reshaping view target of it
                # { src, dst, rows | cols << 32, src_f32 | tile0 << 32 } as four little-endian 64-bit words = the 32-byte descriptor
                rows.append([p.data_ptr(), sh.data_ptr(), n_ | (k_ << 32), int(p.dtype == torch.float32) | (t0 << 32)])
                t0 += ((n_ + 63) // 64) * ((k_ + 63) // 64)
            ent = _tr_table[dev] = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), len(live), t0)
        _, tab, n, tiles = ent
        with torch.cuda.device(dev):
            _lib.check(L.pafc_multi_transpose_bf16(_lib.ptr(tab), n, tiles, _lib.stream_of(tab)), "pafc_multi_transpose_bf16")


def refresh_train_shadows() -> None:
    """Bring every registered bf16 weight copy up to date with its parameter in one multi-tensor copy (and the transposed
    copies in one launch of their own)."""
    _refresh_transposed_shadows()
    live, dead = [], []
    for key, ent in _shadows.items():
        p = ent[0]()
        if p is None or ent[1].device != p.device or ent[1].shape != p.shape:
            dead.append(key)
        else:
            live.append((p, ent[1]))
    for key in dead:
        del _shadows[key]
    for key in list(_wgroups):                      # grouped bf16 copies (r / k / v of a time-mix block as one (3, N, K) operand)
        refs, g = _wgroups[key]
        ps = [r() for r in refs]
        if any(p is None or p.device != g.device or tuple(p.shape) != tuple(g.shape[1:]) for p in ps):
            del _wgroups[key]
        else:
            live.extend((p, g[i]) for i, p in enumerate(ps))
    if live:
        _multi_cast(live)


_cast_table = {}   # device -> (signature, device table of pafc_multi_cast_bf16 descriptors, n, total chunks)


def _multi_cast(pairs) -> None:
    """[(parameter, bf16 copy), ...]: copy <- parameter.  GPU tensors: ONE pafc_multi_cast_bf16 launch per device over a descriptor
    table that is rebuilt only when a pointer changes (torch._foreach_copy_ across dtypes is one launch per tensor on this build:
    108 of the training step's launches); anything else through torch._foreach_copy_."""
    by_dev, rest = {}, []
    for p, sh in pairs:
        if (p.is_cuda and sh.is_cuda and p.device == sh.device and sh.dtype == torch.bfloat16 and p.dtype in (torch.float32, torch.bfloat16)
                and p.is_contiguous() and sh.is_contiguous() and p.numel() == sh.numel() and 0 < p.numel() < (1 << 31)):
            by_dev.setdefault(p.device, []).append((p, sh))
        else:
            rest.append((p, sh))
    if rest:
        with torch.no_grad():
            torch._foreach_copy_([sh for _, sh in rest], [p.detach() for p, _ in rest])
    if not by_dev:
        return
    L = _lib.lib()
    for dev, live in by_dev.items():
        sig = tuple((p.data_ptr(), sh.data_ptr(), p.dtype, p.numel()) for p, sh in live)
        ent = _cast_table.get(dev)
        if ent is None or ent[0] != sig:
            rows, c0 = [], 0
            for p, sh in live:
                # { src, dst, rows | cols << 32, src_f32 | chunk0 << 32 }: the 32-byte descriptor of pafc_multi_transpose_bf16, rows x cols = numel
                rows.append([p.data_ptr(), sh.data_ptr(), p.numel() | (1 << 32), int(p.dtype == torch.float32) | (c0 << 32)])
                c0 += (p.numel() + 4095) // 4096
            ent = _cast_table[dev] = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), len(live), c0)
        _, tab, n, chunks = ent
        with torch.cuda.device(dev):
            _lib.check(L.pafc_multi_cast_bf16(_lib.ptr(tab), n, chunks, _lib.stream_of(tab)), "pafc_multi_cast_bf16")


@contextlib.contextmanager
def train_shadows():
    """The forward pass of one training step: projections take refreshed bf16 copies of their fp32 weights."""
    global _shadows_on
    refresh_train_shadows()
    prev, _shadows_on = _shadows_on, True
    try:
        yield
    finally:
        _shadows_on = prev


def _own_gemm_rows(t2: torch.Tensor) -> bool:
    return t2.dtype == torch.bfloat16 and t2.dim() == 2 and t2.stride(1) == 1 and t2.stride(0) % 8 == 0 and t2.data_ptr() % 16 == 0


class _LinearTrainBf16(torch.autograd.Function):
    """nn.Linear for the bf16 training step, every product on hand-written kernels: forward y = x W^T + b and input gradient
    dX = dY W on the tiled GEMMs (pafc_gemm_bf16; the latter against the bf16 copy of W^T that train_shadows() keeps, one
    multi-tensor transpose per step), the weight gradient through gemm_tn, straight into the weight's dtype -- fp32 master
    weights receive the fp32 sum.  Shapes the kernels do not take (K or N not a multiple of 64 / 8) keep the library."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        wb = _bf16_shadow(weight)
        bb = None if bias is None else _bf16_shadow(bias)
        ctx.save_for_backward(x, wb)
        # the kept W^T copies are only known to be current inside train_shadows() (refreshed on entry, whatever the optimizer did
        # to Tensor._version); a forward pass outside it cast the weight fresh, so its backward transposes THAT copy
        ctx.weight = weight if (_shadows_on and isinstance(_param_of(weight), torch.nn.Parameter)) else None
        ctx.w_dtype = weight.dtype
        ctx.b_dtype = None if bias is None else bias.dtype
        N, K = wb.shape
        x2 = x.reshape(-1, K)
        if (train_gemms_own() and K % 64 == 0 and N % 8 == 0 and _own_gemm_rows(x2) and wb.is_contiguous()
                and (bb is None or bb.dtype == torch.bfloat16)):
            return gemm_bf16(x2, wb.detach(), None if bb is None else bb.detach()).view(x.shape[:-1] + (N,))
        return torch.nn.functional.linear(x, wb, bb)

    @staticmethod
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        N, K = wb.shape
        dy2 = dy.reshape(-1, N)
        if dy2.stride(1) != 1 or dy2.stride(0) % 8 or dy2.data_ptr() % 16:
            dy2 = dy2.contiguous()
        x2 = x.reshape(-1, K)
        if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if train_gemms_own() and N % 64 == 0 and K % 8 == 0 and ctx.weight is not None and _own_gemm_rows(dy2):
                dx = gemm_bf16(dy2, _bf16_shadow_t(ctx.weight)).view(x.shape)      # dY (M, N) x (W^T)(K, N)^T
            elif train_gemms_own() and N % 64 == 0 and K % 8 == 0 and _own_gemm_rows(dy2) and wb.dtype == torch.bfloat16:
                dx = gemm_bf16(dy2, wb.detach().t().contiguous()).view(x.shape)    # the forward's own copy, transposed now
            else:
                dx = (dy2 @ wb).view(x.shape)
        want_b = ctx.b_dtype is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            od = ctx.w_dtype if ctx.w_dtype in (torch.float32, torch.bfloat16) else torch.float32
            if want_b:
                dw, db = gemm_tn(dy2, x2, od, want_bias=True)
                db = db.to(ctx.b_dtype)
            else:
                dw = gemm_tn(dy2, x2, od)
            dw = dw.to(ctx.w_dtype)
        elif want_b:
            db = dy2.sum(0, dtype=torch.float32).to(ctx.b_dtype)
        return dx, dw, db


class _MatmulTrainBf16(torch.autograd.Function):
    """y = act(x @ W + bias) for a parameter stored (K, N) -- the LoRA matrices of the time-mix (src/model.py:277,289) -- on the
    hand-written kernels: forward against the bf16 copy of W^T (N, K) that train_shadows() keeps, input gradient dx = dy W^T against
    W as it lies, weight gradient x^T dy through gemm_tn.  act "tanh" and a bias (the decay's `time_decay + ...`, model.py:289) ride in
    the forward GEMM's epilogue (round 6: one launch instead of three); backward: tanh' from the saved output, the bias gradient a
    column sum."""

    @staticmethod
    def forward(ctx, x, weight, act="none", bias=None):
        K, N = weight.shape
        x2 = x.reshape(-1, K)
        ctx.act, ctx.has_bias = act, bias is not None
        if train_gemms_own() and K % 64 == 0 and N % 8 == 0 and _own_gemm_rows(x2):
            if _shadows_on and isinstance(_param_of(weight), torch.nn.Parameter):
                wt = _bf16_shadow_t(weight)                 # kept beside the parameter, refreshed when train_shadows() was entered
            else:
                wt = weight.detach().t().contiguous()       # outside the step's context nothing vouches for a kept copy
            bb = None if bias is None else bias.detach().reshape(-1).to(torch.bfloat16)
            y = gemm_bf16(x2, wt, bb, act).view(x.shape[:-1] + (N,))                     # (M, K) x (W^T)(N, K)^T
        else:
            y = x @ weight
            if bias is not None:
                y = y + bias.reshape(-1).to(y.dtype)
            if act == "tanh":
                y = torch.tanh(y)
        ctx.save_for_backward(x, weight, y if act == "tanh" else None)
        ctx.bias_shape, ctx.bias_dtype = (None, None) if bias is None else (bias.shape, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        K, N = weight.shape
        if ctx.act == "tanh":
            dy = torch.ops.aten.tanh_backward(dy.contiguous(), y)
        dy2 = dy.reshape(-1, N)
        if dy2.stride(1) != 1 or dy2.stride(0) % 8 or dy2.data_ptr() % 16:
            dy2 = dy2.contiguous()
        x2 = x.reshape(-1, K)
        if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            if train_gemms_own() and N % 64 == 0 and K % 8 == 0 and weight.is_contiguous() and _own_gemm_rows(dy2):
                dx = gemm_bf16(dy2, weight.detach()).view(x.shape)                       # (M, N) x W (K, N)^T
            else:
                dx = (dy2 @ weight.t()).view(x.shape)
        dw = gemm_tn(x2, dy2, torch.bfloat16) if ctx.needs_input_grad[1] else None
        db = None
        if ctx.has_bias and ctx.needs_input_grad[3]:
            # (one reduction kernel: fp32 accumulation inside, one rounding to the bias's dtype -- the value of sum(float32).to())
            db = dy2.sum(0, dtype=ctx.bias_dtype).view(ctx.bias_shape)
        return dx, dw, None, db


def matmul_param(x: torch.Tensor, weight: torch.Tensor, act: str = "none", bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x @ weight + bias) for a 2-D bf16 parameter (act "none" | "tanh"); in the GPU training step on the hand-written kernels
    with the activation and the bias in the GEMM's epilogue."""
    if (x.is_cuda and torch.is_grad_enabled() and weight.requires_grad and weight.dim() == 2 and train_kernels_enabled()
            and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.shape[0] % 8 == 0
            and weight.shape[1] % 8 == 0 and x.numel() // x.shape[-1] >= 256
            and (bias is None or (bias.dtype == torch.bfloat16 and bias.numel() == weight.shape[1]))):
        return _MatmulTrainBf16.apply(x, weight, act, bias)
    y = x @ weight
    if bias is not None:
        y = bias + y
    return torch.tanh(y) if act == "tanh" else y


def linear_train_eligible(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """bf16 activations on the GPU under autograd (autocast(bfloat16) over fp32 master weights, or a bf16 module such
    as the time-mix slot), dims the kernel takes."""
    if not (x.is_cuda and torch.is_grad_enabled() and weight.requires_grad and weight.dim() == 2
            and train_kernels_enabled()):
        return False
    if weight.shape[0] % 8 or weight.shape[1] % 8 or x.numel() // max(1, x.shape[-1]) < 256:
        return False
    if weight.numel() > int(os.environ.get("PAFC_TRAIN_LINEAR_MAX_NUMEL", 2048 * 1024)):      # many output tiles already fill the chip: the library's kernel is as good
        return False
    if x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16:
        return True
    return (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
            and x.dtype in (torch.bfloat16, torch.float32) and weight.dtype in (torch.float32, torch.bfloat16))


def linear_train(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """F.linear whose weight gradient goes through the hand-written kernel (see linear_train_eligible)."""
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)          # what autocast does to F.linear's input
    return _LinearTrainBf16.apply(x, weight, bias)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The projections of the encoder layer as the modules call them: F.linear, except in the bf16 training step, where
    the weight gradient takes the hand-written kernel (linear_train)."""
    if linear_train_eligible(x, weight):
        return linear_train(x, weight, bias)
    return torch.nn.functional.linear(x, weight, bias)


class _LinearOwnF32(torch.autograd.Function):
    """x @ W^T + b of an fp32 model on the hand-written fp32 GEMM, forward and backward: the forward is linear_fused's exact
    product (the bits of the inference path), dX = dY W and dW = dY^T X go through the same kernel on transposed copies (the
    reduction over the rows zero-padded to a multiple of 4, which the kernel's K needs), db is a column sum."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return linear_fused(x, weight.detach(), None if bias is None else bias.detach(), "none", split_ok=False)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        N, K = weight.shape
        dy2 = dy.reshape(-1, N).contiguous()
        x2 = x.reshape(-1, K)
        R = dy2.shape[0]

        def rows_last(t):                                  # (R, C) -> (C, R rounded up to 4), zeros in the padding
            o = t.new_zeros(t.shape[1], -(-R // 4) * 4)
            o[:, :R] = t.t()
            return o
        dx = gemm_f32(dy2, weight.detach().t().contiguous()).view(x.shape) if ctx.needs_input_grad[0] else None
        dw = gemm_f32(rows_last(dy2), rows_last(x2)) if ctx.needs_input_grad[1] else None
        db = dy2.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db


def linear_own(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The projections of a module whose inference path runs on this package's GEMMs, under autograd: an fp32 model outside
    autocast keeps those GEMMs in both directions (_LinearOwnF32: the forward carries the inference path's bits); everything
    else is `linear` (the bf16 training GEMMs under bf16 autocast).  The conditions cover the backward's operands too: its
    three products run on fresh contiguous copies (16-byte aligned, rows padded to a multiple of 4), so beyond the forward's
    form they need only N % 4 == 0, the K of dX = dY W (tests/test_lca_train_gpu.py holds y, dX, dW and db to float64)."""
    if (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and not torch.is_autocast_enabled()
            and (bias is None or bias.dtype == torch.float32) and weight.shape[0] % 4 == 0
            and gemm_f32_ok(x.reshape(-1, weight.shape[1]), weight)):
        return _LinearOwnF32.apply(x, weight, bias)
    return linear(x, weight, bias)


def _weight_group(ws) -> Optional[torch.Tensor]:
    """Z equally shaped weights as ONE (Z, N, K) bf16 operand, inside train_shadows() only (None elsewhere).
    bf16 parameters (the time-mix slot): the parameters THEMSELVES are moved into one buffer the first time they are asked for
    together (`p.data = group[i]`: the Parameter objects, their optimizer state and their names stay; load_state_dict copies in
    place; a later `.to()` that breaks the layout is noticed here and mended) -- no copy to keep fresh, no launch per step.
    fp32 parameters: a grouped bf16 copy beside them, refreshed with the other copies when train_shadows() is entered."""
    if not _shadows_on or any(not isinstance(w, torch.nn.Parameter) or w.dim() != 2 or w.shape != ws[0].shape
                              or w.device != ws[0].device or w.dtype != ws[0].dtype for w in ws):
        return None
    if ws[0].dtype == torch.bfloat16:
        g = _as_batch([w.detach() for w in ws])
        if g is None or not g.is_contiguous():
            with torch.no_grad():
                g = torch.stack([w.detach() for w in ws]).contiguous()
                for i, w in enumerate(ws):
                    w.data = g[i]
            bump_param_epoch()        # the parameters moved: plans and captured graphs that hold their old addresses are stale
        return g
    if ws[0].dtype != torch.float32:
        return None
    key = tuple(id(w) for w in ws)
    ent = _wgroups.get(key)
    if ent is not None and all(r() is w for r, w in zip(ent[0], ws)) and ent[1].device == ws[0].device:
        return ent[1]
    g = torch.stack([w.detach().to(torch.bfloat16) for w in ws]).contiguous()
    _wgroups[key] = [[weakref.ref(w) for w in ws], g]
    return g


def _params_as_one(ps) -> Optional[torch.Tensor]:
    """Z equally shaped parameters of one dtype as ONE contiguous (Z, numel) tensor WITHOUT a copy per use: they are moved into one
    buffer the first time they are asked for together (`p.data = buffer[i].view(shape)`, as _weight_group does for the bf16
    projection weights) -- the four lerp coefficients time_maa_r / k / v / w of a time-mix block (src/model.py:236-240), which the
    training step otherwise stacks on every call (four device-to-device copies).  None when they are not such parameters."""
    p0 = ps[0]
    if any(not isinstance(p, torch.nn.Parameter) or p.shape != p0.shape or p.dtype != p0.dtype or p.device != p0.device
           or not p.is_contiguous() for p in ps) or p0.numel() % 8:
        return None
    g = _as_batch([p.detach().view(1, -1) for p in ps])
    if g is None or not g.is_contiguous():
        with torch.no_grad():
            g = torch.stack([p.detach().reshape(1, -1) for p in ps]).contiguous()
            for i, p in enumerate(ps):
                p.data = g[i].view(p.shape)
        bump_param_epoch()            # the parameters moved: plans and captured graphs that hold their old addresses are stale
    return g.view(len(ps), -1)


def _weight_t_group(ws) -> Optional[torch.Tensor]:
    """(Z, K, N) bf16: the transposed copies of _bf16_shadow_t for Z equally shaped weights, as views of ONE tensor (the
    multi-tensor transpose that refreshes the copies writes into the views)."""
    global _tr_table
    if not _shadows_on or any(not isinstance(w, torch.nn.Parameter) or w.dim() != 2 or w.shape != ws[0].shape for w in ws):
        return None
    N, K = ws[0].shape
    ents = [_shadows_t.get(id(w)) for w in ws]
    if all(e is not None and e[0]() is w for e, w in zip(ents, ws)):
        b = ents[0][1]._base
        if (b is not None and tuple(b.shape) == (len(ws), K, N) and b.is_contiguous()
                and all(e[1]._base is b and e[1].data_ptr() == b[i].data_ptr() for i, e in enumerate(ents))):
            for e, w in zip(ents, ws):                       # a copy whose stamp is not the present one is re-made on the spot
                stamp = (_param_epoch, w._version)
                if e[2] != stamp:
                    with torch.no_grad():
                        e[1].copy_(w.detach().t())
                    e[2] = stamp
            return b
    g = torch.empty((len(ws), K, N), dtype=torch.bfloat16, device=ws[0].device)
    with torch.no_grad():
        for i, w in enumerate(ws):
            g[i].copy_(w.detach().t())
            _shadows_t[id(w)] = [weakref.ref(w), g[i], (_param_epoch, w._version)]
    _tr_table = None
    return g


def _as_batch(ts) -> Optional[torch.Tensor]:
    """Z equally shaped 2-d row-major views of ONE storage at equal distances -> the (Z, M, K) strided view over them (no copy),
    else None.  (The lerp kernel leaves z_r, z_k, z_v as slices of one tensor; the WKV backward leaves g_r, g_k, g_v so.)"""
    a = ts[0]
    if a.dim() != 2 or a.stride(1) != 1 or any(t.shape != a.shape or t.stride() != a.stride() or t.dtype != a.dtype
                                                or t.untyped_storage().data_ptr() != a.untyped_storage().data_ptr() for t in ts):
        return None
    d = ts[1].storage_offset() - a.storage_offset()
    if d <= 0 or d % 8 or any(ts[i + 1].storage_offset() - ts[i].storage_offset() != d for i in range(len(ts) - 1)):
        return None
    return torch.as_strided(a, (len(ts),) + tuple(a.shape), (d,) + tuple(a.stride()), a.storage_offset())


class _LinearGroupTrainBf16(torch.autograd.Function):
    """Z bias-free nn.Linear of one shape on Z inputs -- the r / k / v projections of a time-mix block (src/model.py:286-288) -- as
    ONE batched launch each way: forward against the grouped bf16 weight copy, input gradients against the grouped transposed
    copies, the Z weight gradients from one batched gemm_tn pair.  (Three _LinearTrainBf16 nodes: 3 + 3 + 6 launches and three
    Python backward calls per direction and layer.)"""

    @staticmethod
    def forward(ctx, *args):
        Z = len(args) // 2
        xs, ws = args[:Z], args[Z:]
        N, K = ws[0].shape
        x2 = [x.reshape(-1, K) for x in xs]
        xb = _as_batch(x2)
        if xb is None:
            xb = torch.stack(x2)
        y = gemm_bf16(xb, _weight_group(ws))                           # (Z, M, N)
        ctx.save_for_backward(xb)
        ctx.ws, ctx.x_shape = ws, xs[0].shape
        return tuple(y[i].view(xs[0].shape[:-1] + (N,)) for i in range(Z))

    @staticmethod
    def backward(ctx, *dys):
        (xb,) = ctx.saved_tensors
        ws = ctx.ws
        Z = len(ws)
        N, K = ws[0].shape
        d2 = [(torch.zeros(xb.shape[1], N, dtype=xb.dtype, device=xb.device) if g is None else g.reshape(-1, N)) for g in dys]
        db = _as_batch(d2)
        if db is None:
            db = torch.stack(d2)
        dxs = [None] * Z
        if any(ctx.needs_input_grad[:Z]):
            wt = _weight_t_group(ws)
            if wt is None:                                               # (a backward pass outside train_shadows())
                wt = torch.stack([w.detach().t().to(torch.bfloat16) for w in ws]).contiguous()
            dx = gemm_bf16(db, wt)                                       # (Z, M, N) x (Z, K, N)^T -> (Z, M, K)
            dxs = [dx[i].view(ctx.x_shape) for i in range(Z)]
        dws = [None] * Z
        if any(ctx.needs_input_grad[Z:]):
            od = ws[0].dtype if ws[0].dtype in (torch.float32, torch.bfloat16) else torch.float32
            dw = gemm_tn(db, xb, od)                                     # (Z, N, K)
            dws = [dw[i] for i in range(Z)]
        return (*dxs, *dws)


def linear_group_train_eligible(xs, ws) -> bool:
    """Inside train_shadows(), own training GEMMs, bf16 inputs of one shape, equally shaped bias-free weights the tiles take."""
    if not (_shadows_on and train_gemms_own() and os.environ.get("PAFC_TRAIN_LINEAR_GROUP", "1") != "0"):
        return False
    w0, x0 = ws[0], xs[0]
    if not all(isinstance(w, torch.nn.Parameter) and w.requires_grad and w.dim() == 2 and w.shape == w0.shape and w.dtype == w0.dtype
               and w.is_contiguous() for w in ws):
        return False
    N, K = w0.shape
    return (K % 64 == 0 and N % 64 == 0 and w0.dtype in (torch.float32, torch.bfloat16)
            and all(x.is_cuda and x.dtype == torch.bfloat16 and x.shape == x0.shape and x.shape[-1] == K and x.is_contiguous() for x in xs)
            and x0.numel() // K >= 256 and torch.is_grad_enabled())


def linear_group_train(xs, ws):
    """[F.linear(x_i, w_i)] for equally shaped (x_i, w_i): see _LinearGroupTrainBf16."""
    return _LinearGroupTrainBf16.apply(*xs, *ws)


class _CtcHeadLoss(torch.autograd.Function):
    """CTC head + loss of the training step on hand-written kernels only: logits = x W^T + b (pafc_gemm_bf16), the loss from the
    logits (pafc_ctc_loss_forward: row statistics, the alpha / beta lattice over the label columns), and backwards the gradient
    through the log-softmax written once, bf16, into rows padded to a multiple of 64 columns (pafc_ctc_loss_backward), dX = dlogits W
    on pafc_gemm_bf16 against a zero-padded W^T, dW / db through gemm_tn.  The (B, T, V) log-probabilities never exist; no call
    waits for the host (torch's ctc_loss copies its length tensors back: five synchronising calls per step)."""

    @staticmethod
    def forward(ctx, x, weight, bias, hlens, ys, ylens, blank):
        B, T, C = x.shape
        V = weight.shape[0]
        Vp = (V + 63) // 64 * 64
        M = B * T
        xb = x.reshape(M, C).to(torch.bfloat16)
        wb = _bf16_shadow(weight).detach()
        bb = None if bias is None else _bf16_shadow(bias).detach()
        logits = torch.empty((M, Vp), dtype=torch.bfloat16, device=x.device)
        gemm_bf16(xb, wb, bb, out=logits[:, :V])
        hl = hlens.to(torch.int32).contiguous()
        yl = ylens.to(torch.int32).contiguous()
        ysc = ys.to(torch.int64).contiguous()
        Lmax = ysc.shape[1]
        L = _lib.lib()
        nbytes = L.pafc_ctc_loss_workspace_bytes(B, T, Lmax)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        nll = torch.empty(B, dtype=torch.float32, device=x.device)
        st = _lib.stream_of(x)
        _lib.check(L.pafc_ctc_loss_forward(_lib.PAFC_BF16, B, T, V, _lib.ptr(logits), Vp, _lib.ptr(hl), _lib.ptr(ysc), Lmax, _lib.ptr(yl),
                                           Lmax, int(blank), _lib.ptr(nll), _lib.ptr(ws), nbytes, st), "pafc_ctc_loss_forward")
        ctx.save_for_backward(xb, wb, logits, ws, nll, hl, ysc, yl)
        ctx.dims = (B, T, C, V, Vp, Lmax, int(blank))
        ctx.w_dtype, ctx.b_dtype, ctx.x_dtype = weight.dtype, None if bias is None else bias.dtype, x.dtype
        return nll.sum() / B                          # reduction="sum", then the batch-size average of ctc.py:77

    @staticmethod
    def backward(ctx, g):
        xb, wb, logits, ws, nll, hl, ysc, yl = ctx.saved_tensors
        B, T, C, V, Vp, Lmax, blank = ctx.dims
        M = B * T
        L = _lib.lib()
        dl = torch.empty((M, Vp), dtype=torch.bfloat16, device=xb.device)
        gf = g.detach().to(torch.float32).reshape(1).contiguous()
        _lib.check(L.pafc_ctc_loss_backward(_lib.PAFC_BF16, B, T, V, _lib.ptr(logits), Vp, _lib.ptr(hl), _lib.ptr(ysc), Lmax, _lib.ptr(yl),
                                            Lmax, blank, _lib.ptr(nll), _lib.ptr(gf), 1.0 / B, _lib.ptr(dl), Vp, _lib.ptr(ws), ws.numel(),
                                            _lib.stream_of(xb)), "pafc_ctc_loss_backward")
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wt = torch.zeros((C, Vp), dtype=torch.bfloat16, device=xb.device)       # W^T, zero beyond V: K = Vp is a multiple of 64
            wt[:, :V].copy_(wb.t())
            dx = gemm_bf16(dl, wt).view(B, T, C).to(ctx.x_dtype)
        want_b = ctx.b_dtype is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            od = ctx.w_dtype if ctx.w_dtype in (torch.float32, torch.bfloat16) else torch.float32
            if want_b:
                dw, db = gemm_tn(dl[:, :V], xb, od, want_bias=True)
                db = db.to(ctx.b_dtype)
            else:
                dw = gemm_tn(dl[:, :V], xb, od)
            dw = dw.to(ctx.w_dtype)
        elif want_b:
            db = dl[:, :V].sum(0, dtype=torch.float32).to(ctx.b_dtype)
        return dx, dw, db, None, None, None, None


# tests/test_train_loss_kernels_gpu.py calls the CTC loss kernels directly through this name; the signatures are _lib's.
_bind_ctc_loss = _lib.lib


def ctc_head_loss_eligible(x: torch.Tensor, weight: torch.Tensor, ys: torch.Tensor) -> bool:
    """The GPU training step under bf16 autocast (or a bf16 model): dims the kernels take."""
    if not (x.is_cuda and torch.is_grad_enabled() and train_kernels_enabled() and x.dim() == 3 and ys.dim() == 2):
        return False
    V, C = weight.shape
    if C % 64 or V % 8 or V * 4 > 150 * 1024 or x.shape[0] > 65535 or ys.shape[1] > 3000 or os.environ.get("PAFC_TRAIN_CTC", "1") == "0":
        return False
    if x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16:
        return True
    return (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
            and x.dtype in (torch.bfloat16, torch.float32) and weight.dtype in (torch.float32, torch.bfloat16))


def ctc_head_loss(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], hlens: torch.Tensor, ys: torch.Tensor,
                  ylens: torch.Tensor, blank: int = 0) -> torch.Tensor:
    """sum_b CTC(log_softmax(x_b W^T + b), y_b) / B with zero_infinity (ctc.py:53-82), see _CtcHeadLoss."""
    return _CtcHeadLoss.apply(x, weight, bias, hlens, ys, ylens, blank)


RNNT_SLAB_BYTES = 1 << 30     # backward's dz (rows, Vp) bf16 + dH (rows, J) fp32 slab: ~85 000 lattice rows at V = 5000, J = 640


class _RnntJointLoss(torch.autograd.Function):
    """RNN-T joint + loss of the training step on hand-written kernels only (csrc/rnnt_loss.hip, include/pafc_encoder_ops.h):
    h = tanh(E[n, t] + P[n, u]) written once as bf16 (R, J), the logits' row statistics from the epilogue of H W^T + b (the
    (R, V) logits are never stored), the lattice per utterance, and backwards dz in slabs of whole utterances, dH = dz W,
    dW / db = dz^T H and the tanh derivative reduced into dE / dP.  One host read of the lengths per call plans the row
    offsets and the slabs (forward_optimized + transducer_loss make 2 B + 2)."""

    @staticmethod
    def forward(ctx, E, P, weight, bias, hlens, ys, ylens, blank):
        B, T, J = E.shape
        Up1 = P.shape[1]
        V = weight.shape[0]
        Eb = E.detach().to(torch.bfloat16).contiguous()
        Pb = P.detach().to(torch.bfloat16).contiguous()
        wb = _bf16_shadow(weight).detach().contiguous()
        bb = None if bias is None else _bf16_shadow(bias).detach().contiguous()
        hl = hlens.to(device=E.device, dtype=torch.int32).contiguous()
        yl = ylens.to(device=E.device, dtype=torch.int32).contiguous()
        ysc = ys.to(device=E.device, dtype=torch.int64).contiguous()
        ldy = ysc.shape[1]
        lens = torch.stack([hl, yl]).cpu()             # the one host synchronisation of the call
        Ts, Us = lens[0].tolist(), lens[1].tolist()
        for n, (t, u) in enumerate(zip(Ts, Us)):
            if not (1 <= t <= T and 0 <= u < Up1 and u <= ldy):
                raise _lib.PafcError(f"rnnt_joint_loss: utterance {n} has {t} frames / {u} labels, outside E (T = {T}), "
                                     f"P (U + 1 = {Up1}) or ys ({ldy} columns)")
        row_off = [0]
        for t, u in zip(Ts, Us):
            row_off.append(row_off[-1] + t * (u + 1))
        R = row_off[-1]
        Vp = (V + 63) // 64 * 64
        slab_rows = max(max(t * (u + 1) for t, u in zip(Ts, Us)), min(R, RNNT_SLAB_BYTES // (2 * Vp + 4 * J)))
        L = _lib.lib()
        nbytes = L.pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, 0, None, 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=E.device)
        nll = torch.empty(B, dtype=torch.float32, device=E.device)
        _lib.check(L.pafc_rnnt_joint_loss_forward(B, T, Up1, J, V, _lib.ptr(Eb), J, T * J, _lib.ptr(Pb), J, Up1 * J, _lib.ptr(wb),
                                                  _lib.ptr(bb), _lib.ptr(hl), _lib.ptr(yl), _lib.ptr(ysc), ldy, int(blank), R,
                                                  _lib.ptr(nll), _lib.ptr(ws), nbytes, _lib.stream_of(E)),
                   "pafc_rnnt_joint_loss_forward")
        ctx.save_for_backward(Eb, Pb, wb, bb, ws, hl, yl, ysc)
        ctx.plan = (B, T, Up1, J, V, ldy, int(blank), R, row_off, slab_rows)
        ctx.dtypes = (E.dtype, P.dtype, weight.dtype, None if bias is None else bias.dtype)
        return nll

    @staticmethod
    def backward(ctx, g):
        Eb, Pb, wb, bb, ws, hl, yl, ysc = ctx.saved_tensors
        B, T, Up1, J, V, ldy, blank, R, row_off, slab_rows = ctx.plan
        e_dt, p_dt, w_dt, b_dt = ctx.dtypes
        L = _lib.lib()
        off = (ctypes.c_int64 * (B + 1))(*row_off)
        sbytes = L.pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, slab_rows, off, 1)
        if sbytes == 0:
            raise _lib.PafcError("pafc_rnnt_joint_loss_workspace_bytes: no backward plan for these lengths")
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=Eb.device)
        gdt = torch.bfloat16 if (e_dt == torch.bfloat16 and p_dt == torch.bfloat16) else torch.float32
        dE = torch.empty((B, T, J), dtype=gdt, device=Eb.device)
        dP = torch.empty((B, Up1, J), dtype=gdt, device=Eb.device)
        dW = torch.empty((V, J), dtype=torch.float32, device=Eb.device)
        db = torch.empty(V, dtype=torch.float32, device=Eb.device) if b_dt is not None else None
        gf = g.detach().to(torch.float32).contiguous()
        _lib.check(L.pafc_rnnt_joint_loss_backward(B, T, Up1, J, V, _lib.ptr(Eb), J, T * J, _lib.ptr(Pb), J, Up1 * J, _lib.ptr(wb),
                                                   _lib.ptr(bb), _lib.ptr(hl), _lib.ptr(yl), _lib.ptr(ysc), ldy, blank, R, off, slab_rows,
                                                   _lib.ptr(gf), 1.0, _lib.dtype_code(gdt), _lib.ptr(dE), _lib.ptr(dP), _lib.ptr(dW),
                                                   _lib.ptr(db), _lib.ptr(ws), ws.numel(), _lib.ptr(scratch), sbytes,
                                                   _lib.stream_of(Eb)), "pafc_rnnt_joint_loss_backward")
        return (dE.to(e_dt), dP.to(p_dt), dW.to(w_dt), None if db is None else db.to(b_dt), None, None, None, None)


def rnnt_joint_loss_unmet(enc_proj: torch.Tensor, pred_proj: torch.Tensor, weight: torch.Tensor) -> Optional[str]:
    """The condition the fused RNN-T joint + loss does not meet for these operands, or None (the same conditions as
    ctc_head_loss_eligible: the GPU training step under bf16 autocast or with a bf16 model, and dims the kernels take)."""
    if not enc_proj.is_cuda:
        return "the operands are not on the GPU"
    if not torch.is_grad_enabled():
        return "gradients are disabled"
    if not train_kernels_enabled():
        return "PAFC_TRAIN_KERNELS=0"
    if enc_proj.dim() != 3 or pred_proj.dim() != 3 or enc_proj.shape[0] != pred_proj.shape[0]:
        return "enc_proj (B, T, J) and pred_proj (B, U + 1, J) are expected"
    V, J = weight.shape
    if enc_proj.shape[2] != J or pred_proj.shape[2] != J:
        return "the joint dimension of enc_proj / pred_proj differs from the output layer's"
    if J % 64:
        return f"join_dim {J} is not a multiple of 64"
    if V % 8:
        return f"vocab_size {V} is not a multiple of 8"
    if enc_proj.shape[0] > 65535 or pred_proj.shape[1] > 2559:
        return "more than 65535 utterances or 2558 labels per utterance"
    bf16_model = enc_proj.dtype == torch.bfloat16 and pred_proj.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
    autocast_bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
    if not (bf16_model or autocast_bf16):
        return "neither bf16 autocast nor a bf16 model"
    return None


def rnnt_joint_loss_eligible(enc_proj: torch.Tensor, pred_proj: torch.Tensor, weight: torch.Tensor) -> bool:
    return rnnt_joint_loss_unmet(enc_proj, pred_proj, weight) is None


def rnnt_joint_loss(enc_proj: torch.Tensor, pred_proj: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                    hlens: torch.Tensor, ys: torch.Tensor, ylens: torch.Tensor, blank: int = 0) -> torch.Tensor:
    """Per-utterance RNN-T nll (B,) fp32 of the joint ffn_out(tanh(enc_proj[:, t] + pred_proj[:, u])) (joint.py:111-149 +
    the transducer loss of transducer.py:506-561), see _RnntJointLoss.  enc_proj (B, T, J), pred_proj (B, U + 1, J) over the
    blank-prepended targets, weight (V, J) / bias (V) of ffn_out, ys (B, >= U_n) targets."""
    return _RnntJointLoss.apply(enc_proj, pred_proj, weight, bias, hlens, ys, ylens, blank)


# Rows (utterance, frame, arc) one group of rnnt_score_hypotheses may hold.  The workspace takes 2 J + 8 ceil(V / 128) + 16
# bytes per row: 1 616 at J = 640, V = 5000, so 2^19 rows are 0.85 GB.
RNNT_SCORE_MAX_ROWS = 1 << 19


def rnnt_score_unmet(enc_proj: torch.Tensor, pred_nodes: torch.Tensor, weight: torch.Tensor) -> Optional[str]:
    """The condition rnnt_score_hypotheses does not meet for these operands, or None: the dims of rnnt_joint_loss_unmet."""
    if not (enc_proj.is_cuda and pred_nodes.is_cuda and weight.is_cuda):
        return "the operands are not on the GPU"
    if enc_proj.dim() != 3 or pred_nodes.dim() < 2:
        return "enc_proj (B, T, J) and pred_nodes (..., J) are expected"
    V, J = weight.shape
    if enc_proj.shape[2] != J or pred_nodes.shape[-1] != J:
        return "the joint dimension of enc_proj / pred_nodes differs from the output layer's"
    if J % 64:
        return f"join_dim {J} is not a multiple of 64"
    if V % 8:
        return f"vocab_size {V} is not a multiple of 8"
    return None


def rnnt_score_hypotheses(enc_proj: torch.Tensor, pred_nodes: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                          hlens: Optional[torch.Tensor], tables, blank: int = 0, max_rows: int = RNNT_SCORE_MAX_ROWS) -> torch.Tensor:
    """log p(y | x) of every hypothesis of a batch of n-best lists, (N,) fp32 on the device, scored over the prefix trie of each
    list (csrc/rnnt_loss.hip: pafc_rnnt_score, include/pafc_search.h).  enc_proj (B, T, J) = enc_ffn(encoder_out), once per
    utterance; pred_nodes (N, tables.pred_stride, J) = pred_ffn(predictor(blank-prepended padded hypotheses)); weight (V, J) /
    bias (V) of ffn_out; hlens (B) frames on the device (a hypothesis of an utterance whose length there is not the tables' gets
    NaN), or None when the tables were built from lengths the caller holds on the host; tables: transducer.search.rescoring.build_arc_tables of the same lengths.  Casts as
    _RnntJointLoss.forward does (bf16 operands, the cached bf16 copies of the weights), and a hypothesis gets the bits of
    -rnnt_joint_loss of that hypothesis alone.  One upload (the packed tables), no read of the host.  The batch runs in groups
    of whole utterances of at most max_rows rows each, which bounds the workspace (RNNT_SCORE_MAX_ROWS: 0.85 GB at J = 640,
    V = 5000); an utterance that alone has more rows raises PafcError."""
    unmet = rnnt_score_unmet(enc_proj, pred_nodes, weight)
    if unmet is not None:
        raise _lib.PafcError(f"rnnt_score_hypotheses: {unmet}")
    B, T, J = enc_proj.shape
    V = weight.shape[0]
    dev = enc_proj.device
    if hlens is not None and hlens.numel() != B:
        raise _lib.PafcError(f"rnnt_score_hypotheses: {hlens.numel()} lengths for {B} utterances")
    score = torch.empty(tables.nhyp, dtype=torch.float32, device=dev)
    if tables.nhyp == 0:
        return score
    groups, start, acc = [], 0, 0                      # consecutive whole utterances, at most max_rows rows each
    for b, r in enumerate(tables.utt_rows):
        if r > max_rows:
            raise _lib.PafcError(f"rnnt_score_hypotheses: utterance {b} alone has {r} rows (frames x arcs), more than max_rows = "
                                 f"{max_rows}")
        if acc + r > max_rows:
            groups.append((start, b, acc))
            start, acc = b, 0
        acc += r
    groups.append((start, tables.nutt, acc))
    groups = [g for g in groups if g[2] > 0]
    Eb = enc_proj.detach().to(torch.bfloat16).contiguous()
    Pb = pred_nodes.detach().to(torch.bfloat16).reshape(-1, J).contiguous()
    wb = _bf16_shadow(weight).detach().contiguous()
    bb = None if bias is None else _bf16_shadow(bias).detach().contiguous()
    hl = None if hlens is None else hlens.to(device=dev, dtype=torch.int32).contiguous()
    tab = tables.packed.to(dev, non_blocking=True)     # the one upload
    L = _lib.lib()
    nbytes = max(L.pafc_rnnt_score_workspace_bytes(u1 - u0, J, V, rows) for u0, u1, rows in groups)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for u0, u1, _ in groups:
        _lib.check(L.pafc_rnnt_score(B, T, J, V, _lib.ptr(Eb), J, T * J, _lib.ptr(Pb), J, Pb.shape[0], _lib.ptr(wb), _lib.ptr(bb),
                                     _lib.ptr(hl), tables.nutt, tables.nhyp, tables.narc, tables.ncol, _lib.ptr(tables.packed),
                                     _lib.ptr(tab), u0, u1, int(blank), _lib.ptr(score), _lib.ptr(ws), nbytes, _lib.stream_of(Eb)),
                   "pafc_rnnt_score")
    return score


RNNT_GREEDY_CHUNK = 32     # lockstep steps between two reads of the running-row count, after the first T steps


class _Packed:
    """Several result arrays in one uint8 device buffer, so that one copy brings them all to the host.  fields: (name, dtype,
    shape) in the order they are laid out, those of 8-byte elements first, so every field is aligned to its element size."""

    def __init__(self, fields, device):
        self._at, off = {}, 0
        for name, dtype, shape in sorted(fields, key=lambda f: f[1].itemsize != 8):
            end = off + dtype.itemsize * math.prod(shape)
            self._at[name] = (off, end, dtype, tuple(shape))
            off = end
        self.nbytes = off
        self.buf = torch.empty(off, dtype=torch.uint8, device=device)
        self._host = None

    def offset(self, name: str) -> int:
        return self._at[name][0]

    def ptr(self, name: str):
        a, b = self._at[name][:2]
        return _lib.ptr(self.buf[a:b])

    def read(self):
        """The one copy to the host."""
        self._host = self.buf.cpu()
        return self

    def host(self, name: str) -> torch.Tensor:
        """The field as the last read() brought it, typed and shaped."""
        a, b, dtype, shape = self._at[name]
        return self._host[a:b].view(dtype).view(shape)


class _RowStream:
    """What the chunk-by-chunk searches of B rows share: the library, the workspace (_ws, _nbytes), the frame counts of the next
    chunk (_nf), the row mask of a reset and, for the two beam searches, the drain."""

    _pinned = False       # host frame counts and `from` offsets go up from pinned memory, without a synchronising call

    def _device(self, device) -> torch.device:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.PafcError(f"{type(self).__name__} runs on the MI355X only (device {dev}); there is no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev

    def _init_rows(self, B: int, dev, fn: str, args, why: str = "unsupported dimensions"):
        """The workspace of the size the library's `fn(*args)` gives, and the per-row device buffers."""
        self.B, self.device, self._L = B, dev, _lib.lib()
        self._nbytes = getattr(self._L, fn)(*args)
        if self._nbytes == 0:
            raise _lib.PafcError(f"{fn}: {why}")
        self._ws = torch.empty(self._nbytes, dtype=torch.uint8, device=dev)
        self._nf = torch.zeros(B, dtype=torch.int64, device=dev)
        self._mask = torch.zeros(B, dtype=torch.int32, device=dev)

    def _up(self, dst: torch.Tensor, src: torch.Tensor):
        if self._pinned and not src.is_cuda:
            dst.copy_(src.pin_memory(), non_blocking=True)     # (the pinned block is not reused before the copy ran)
        else:
            dst.copy_(src)

    def _row_mask(self, rows):
        """The pointer a reset takes: null for all rows, else the device mask with the given rows set."""
        if rows is None:
            return None
        m = torch.zeros(self.B, dtype=torch.int32)
        m[torch.as_tensor(list(rows), dtype=torch.long)] = 1
        self._mask.copy_(m)
        return _lib.ptr(self._mask)

    def _set_nframes(self, nframes, n: int):
        """The frame counts of a chunk of n frames into _nf: n for every row when None, else (B,) counts clamped to [0, n]."""
        if nframes is None:
            self._nf.fill_(n)
            return
        nf = torch.as_tensor(nframes, dtype=torch.int64)
        if nf.shape != (self.B,):
            raise _lib.PafcError(f"{type(self).__name__}.feed: nframes must be ({self.B},)")
        self._up(self._nf, nf.clamp(0, n))

    def _init_drain(self):
        self._from = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._from_h = [0] * self.B
        self.last_read_bytes = 0

    def _drain_nbest(self, call, counts, ld: int):
        """The drain of a beam search: counts into the `from` buffer, call(out, ld) launches the drain kernel into the packed
        buffer `out`: score (B, beam) f64 | len (B, beam) | count | committed | overflow (B) | tokens (B, beam, ld) i32; then
        the one read and the dict of host lists."""
        B, beam = self.B, self.beam
        counts = [0] * B if counts is None else [int(c) for c in counts]
        if counts != self._from_h:
            self._up(self._from, torch.tensor(counts, dtype=torch.int32))
            self._from_h = counts
        ld = max(1, int(ld))
        i32 = torch.int32
        out = _Packed([("score", torch.float64, (B, beam)), ("len", i32, (B, beam)), ("count", i32, (B,)),
                       ("committed", i32, (B,)), ("overflow", i32, (B,)), ("tokens", i32, (B, beam, ld))], self.device)
        call(out, ld)
        out.read()
        self.last_read_bytes = out.nbytes
        res = {k: out.host(k).tolist() for k in ("score", "len", "count", "committed", "overflow")}
        lens, toks = res["len"], out.host("tokens").tolist()
        res["tokens"] = [[toks[b][n][:max(0, min(ld, lens[b][n] - counts[b]))] for n in range(beam)] for b in range(B)]
        return res


class _GreedyNet(ctypes.Structure):
    """include/pafc_search.h: pafc_rnnt_greedy_net."""
    _PP = ctypes.POINTER(c_void_p)
    _fields_ = [("dtype", c_int), ("num_layers", c_int), ("embed_dim", c_int), ("hidden", c_int), ("pred_dim", c_int),
                ("join_dim", c_int), ("vocab", c_int), ("embed_rows", c_int), ("embed", c_void_p), ("w_ih", _PP), ("w_hh", _PP),
                ("b_ih", _PP), ("b_hh", _PP), ("proj_w", c_void_p), ("proj_b", c_void_p), ("pred_ffn_w", c_void_p),
                ("pred_ffn_b", c_void_p), ("out_w", c_void_p), ("out_b", c_void_p)]


def _greedy_net(predictor, joint):
    """The weights as a pafc_rnnt_greedy_net, and the tensors it points into (kept alive by the caller)."""
    rnn = predictor.rnn
    nl, H = rnn.num_layers, rnn.hidden_size
    keep = []

    def p(t):
        if t is None:
            return None
        t = t.detach().contiguous()
        keep.append(t)
        return t.data_ptr()

    def arr(name):
        ptrs = [p(getattr(rnn, f"{name}_l{l}", None)) for l in range(nl)]
        return None if any(v is None for v in ptrs) else (c_void_p * nl)(*ptrs)

    w_ih, w_hh, b_ih, b_hh = arr("weight_ih"), arr("weight_hh"), arr("bias_ih"), arr("bias_hh")
    keep += [w_ih, w_hh, b_ih, b_hh]
    cast = lambda a: ctypes.cast(a, ctypes.POINTER(c_void_p)) if a is not None else None
    proj, pf, out = predictor.projection, joint.pred_ffn, joint.ffn_out
    net = _GreedyNet(_lib.dtype_code(out.weight.dtype), nl, predictor.embed.embedding_dim, H, proj.out_features, out.in_features,
                     out.out_features, predictor.embed.num_embeddings, p(predictor.embed.weight), cast(w_ih), cast(w_hh), cast(b_ih),
                     cast(b_hh), p(proj.weight), p(proj.bias), p(pf.weight), p(pf.bias), p(out.weight), p(out.bias))
    return net, keep


def _enc_ffn(joint, as_is: bool = False):
    """joint.enc_ffn's (weight, bias), detached and contiguous (as_is: detached only, strides as the module holds them)."""
    ef, fix = joint.enc_ffn, (torch.Tensor.detach if as_is else lambda t: t.detach().contiguous())
    return fix(ef.weight), None if ef.bias is None else fix(ef.bias)


def _enc_project(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """E = enc_ffn(x) for rows x (rows, D) through gemm_f32 / gemm_bf16 by the weight's dtype, (w, b) from _enc_ffn."""
    return (gemm_f32 if w.dtype == torch.float32 else gemm_bf16)(x, w, b, out=out)


def _shape_like(B: int, T: int, D: int, device) -> torch.Tensor:
    """An expanded view of one element: what the *_unmet checks read of a (B, T, D) buffer, without allocating it."""
    return torch.empty(1, 1, 1, device=device).expand(B, T, D)


def rnnt_greedy_unmet(predictor, joint, encoder_out: torch.Tensor, n_steps: int = 64) -> Optional[str]:
    """The condition the greedy-search kernels (csrc/rnnt_greedy.hip) do not meet for this predictor / joint / encoder output,
    or None.  The kernels take the paper's modules: an LSTM predictor with its projection, a joint with pre-join projections,
    tanh and no post-join projection or HAT; every weight fp32 or every weight bf16; eval-mode arithmetic."""
    rnn = getattr(predictor, "rnn", None)
    if not isinstance(rnn, torch.nn.LSTM) or getattr(predictor, "embed", None) is None or getattr(predictor, "projection", None) is None:
        return "the predictor is not an LSTM predictor (embedding, nn.LSTM, projection)"
    if rnn.bidirectional or rnn.proj_size or not rnn.batch_first:
        return "the predictor's LSTM is bidirectional, has proj_size or is not batch_first"
    if not getattr(joint, "prejoin_linear", False) or joint.enc_ffn is None or joint.pred_ffn is None:
        return "the joint has no pre-join projections (prejoin_linear: false)"
    if joint.postjoin_linear:
        return "the joint has a post-join projection (postjoin_linear: true)"
    if getattr(joint, "hat_joint", False):
        return "hat_joint"
    if not isinstance(joint.activatoin, torch.nn.Tanh):
        return "the joint's activation is not tanh"
    for m in (predictor, joint):
        if m.training and any(isinstance(d, torch.nn.Dropout) and d.p > 0 for d in m.modules()):
            return "the predictor or joint is in training mode with dropout (call .eval())"
    if predictor.training and rnn.dropout > 0 and rnn.num_layers > 1:
        return "the predictor's LSTM is in training mode with dropout between layers (call .eval())"
    params = list(predictor.parameters()) + list(joint.parameters())
    dt = joint.ffn_out.weight.dtype
    if dt not in (torch.float32, torch.bfloat16) or any(q.dtype != dt for q in params):
        return "the predictor and joint weights are not all fp32 or all bf16"
    if not encoder_out.is_cuda:
        return "the encoder output is not on the GPU"
    if any(not q.is_cuda or q.device != encoder_out.device for q in params):
        return "the predictor / joint weights are not on the encoder output's GPU"
    if encoder_out.dim() != 3 or encoder_out.shape[0] == 0 or encoder_out.shape[1] == 0:
        return "encoder_out must be (B, T, D) with B, T >= 1"
    B, T, D = encoder_out.shape
    E, Hd, Pd, J = predictor.embed.embedding_dim, rnn.hidden_size, predictor.projection.out_features, joint.ffn_out.in_features
    V = joint.ffn_out.out_features
    if any(d % 4 for d in (E, Hd, Pd, J)):
        return "the embedding, hidden, projection and join dimensions must be multiples of 4"
    if J > 2048:
        return f"join_dim {J} is above 2048"
    if predictor.embed.num_embeddings < V:
        return "the predictor's embedding has fewer rows than the joint's vocabulary"
    if dt == torch.float32 and D % 4:
        return f"encoder dimension {D} is not a multiple of 4 (gemm_f32)"
    if dt == torch.bfloat16 and (D % 64 or J % 8):
        return f"encoder dimension {D} is not a multiple of 64 or join_dim {J} not of 8 (gemm_bf16)"
    if B > 256:
        return f"{B} utterances: at most 256 per call"
    if n_steps < 1 or T * n_steps >= 2 ** 31:
        return "n_steps must be >= 1 and T * n_steps below 2^31"
    return None


def rnnt_greedy_search(predictor, joint, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, blank: int = 0,
                       n_steps: int = 64, chunk: int = RNNT_GREEDY_CHUNK):
    """Greedy search (basic_greedy_search, wenet/transducer/search/greedy_search.py) of every utterance of encoder_out (B, T, D)
    on the lockstep kernels of csrc/rnnt_greedy.hip (include/pafc_search.h: pafc_rnnt_greedy_*).  E = enc_ffn(encoder_out) once
    through gemm_f32 / gemm_bf16, then T steps -- the number every utterance of length T needs at least -- and chunks of
    `chunk` steps until no row is running.  Host reads per call: one 4-byte read of the running-row count after the first T
    steps and after every further chunk, plus one read of the packed results: 2 + ceil(max(0, S - T) / chunk), S the largest
    number of decisions of one utterance.  Returns (tokens, frames, scores): per utterance its token list, the frame of each
    token, and the path log-probability (sum of log p over every decision, blanks included, float64)."""
    unmet = rnnt_greedy_unmet(predictor, joint, encoder_out, n_steps)
    if unmet is not None:
        raise _lib.PafcError(f"rnnt_greedy_search: {unmet}")
    B, T, D = encoder_out.shape
    dev = encoder_out.device
    wdt = joint.ffn_out.weight.dtype
    x = encoder_out.detach().to(wdt).reshape(B * T, D).contiguous()
    E = _enc_project(x, *_enc_ffn(joint, as_is=wdt == torch.float32))      # (the fp32 GEMM takes the weight's own strides)
    lens = encoder_out_lens.detach().to(device=dev, dtype=torch.int64).contiguous()
    if lens.shape != (B,):
        raise _lib.PafcError("rnnt_greedy_search: encoder_out_lens must be (B,)")
    L = _lib.lib()
    net, keep = _greedy_net(predictor, joint)
    pnet = ctypes.byref(net)
    nbytes = L.pafc_rnnt_greedy_workspace_bytes(pnet, B, T, n_steps)
    if nbytes == 0:
        raise _lib.PafcError("pafc_rnnt_greedy_workspace_bytes: unsupported dimensions")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    running = torch.empty(1, dtype=torch.int32, device=dev)
    st = _lib.stream_of(E)
    _lib.check(L.pafc_rnnt_greedy_init(pnet, B, T, n_steps, int(blank), _lib.ptr(lens), _lib.ptr(ws), nbytes, st),
               "pafc_rnnt_greedy_init")
    args = (pnet, B, T, n_steps, int(blank), _lib.ptr(E), _lib.ptr(ws), nbytes, _lib.ptr(running), st)
    steps, todo = 0, T
    while True:
        for _ in range(todo):
            _lib.check(L.pafc_rnnt_greedy_step(*args), "pafc_rnnt_greedy_step")
        steps += todo
        if int(running.item()) == 0:               # the host read of this chunk
            break
        if steps > T * (n_steps + 1):              # every row ends within T (n_steps + 1) decisions
            raise _lib.PafcError("rnnt_greedy_search: rows still running after T * (n_steps + 1) steps")
        todo = chunk
    ld = steps                                     # a row emits at most one token per step
    out = _Packed([("score", torch.float64, (B,)), ("ntok", torch.int32, (B,)), ("tokens", torch.int32, (B, ld)),
                   ("frames", torch.int32, (B, ld))], dev)
    _lib.check(L.pafc_rnnt_greedy_finish(pnet, B, T, n_steps, _lib.ptr(ws), nbytes, ld, out.ptr("tokens"), out.ptr("frames"),
                                         out.ptr("ntok"), out.ptr("score"), None, st), "pafc_rnnt_greedy_finish")
    out.read()                                     # the final read
    del keep
    n_h, t_h, f_h = out.host("ntok").tolist(), out.host("tokens"), out.host("frames")
    return ([t_h[b, :n_h[b]].tolist() for b in range(B)], [f_h[b, :n_h[b]].tolist() for b in range(B)],
            out.host("score").tolist())


def rnnt_greedy_stream_unmet(predictor, joint, B: int, Tmax: int, D: int, device, n_steps: int = 64) -> Optional[str]:
    """The condition the streaming greedy search (RnntGreedyStream) does not meet for B streams of chunks of at most Tmax
    frames of dimension D on `device`, or None: rnnt_greedy_unmet's conditions, and Tmax >= 1."""
    if Tmax < 1:
        return f"Tmax {Tmax}: a chunk must hold at least one frame"
    if B < 1:
        return f"{B} streams: at least one"
    return rnnt_greedy_unmet(predictor, joint, _shape_like(B, Tmax, D, device), n_steps)


class RnntGreedyStream(_RowStream):
    """Greedy search of B streams chunk by chunk on the lockstep kernels of csrc/rnnt_greedy.hip (include/pafc_search.h:
    pafc_rnnt_greedy_stream_*), the decoder state carried from one chunk to the next.  The object owns the workspace, a fixed
    (B, Tmax, D) input buffer, the fixed (B, Tmax, J) E = enc_ffn buffer (gemm_f32 / gemm_bf16 into it) and the weights'
    net struct.  Given the same E rows, the tokens, frames and scores over a stream equal rnnt_greedy_search over the
    concatenated frames bit for bit: a row leaves a chunk at a frame boundary, in the state the whole-utterance decode
    holds there.

    feed(chunk (B, n <= Tmax, D), nframes=None): row b decodes its first nframes[b] frames (default n; 0 = the row sits the
    chunk out with its state unchanged).  Steps: n -- what every row with n frames needs at least --, then chunks of
    RNNT_GREEDY_CHUNK until no row runs.  Host reads per feed: one 4-byte read of the running-row count after the first n
    steps and after every further chunk, plus one read of the results: 2 + ceil(max(0, S - n) / chunk), S the largest number
    of decisions a row makes in this chunk.  Launches per feed: the chunk copied into the input buffer and nframes written to
    its device buffer (a fill, or a copy of the given counts -- pass a device int64 tensor to keep it off the host), both
    eager because their sources change from feed to feed; then the fixed part -- E projection, feed kernel, n steps --
    replayed from a hipGraph captured once per n (eager only where the capture is refused); then the eager chunks of
    steps, the drain and its read.  Only the package's own kernels run, so a streamer may live on a side stream."""

    def __init__(self, predictor, joint, B: int, Tmax: int, n_steps: int = 64, blank: int = 0, D: Optional[int] = None,
                 chunk: int = RNNT_GREEDY_CHUNK, use_graph: bool = True):
        D = joint.enc_ffn.in_features if D is None and getattr(joint, "enc_ffn", None) is not None else D
        dev = joint.ffn_out.weight.device
        unmet = rnnt_greedy_stream_unmet(predictor, joint, B, Tmax, D or 0, dev, n_steps)
        if unmet is not None:
            raise _lib.PafcError(f"RnntGreedyStream: {unmet}")
        self.Tmax, self.D, self.n_steps, self.blank, self.chunk = Tmax, D, n_steps, int(blank), chunk
        self.use_graph = use_graph
        self.dtype = joint.ffn_out.weight.dtype
        self._w, self._b = _enc_ffn(joint)
        J = joint.ffn_out.in_features
        self._net, self._keep = _greedy_net(predictor, joint)
        self._pnet = ctypes.byref(self._net)
        self._init_rows(B, dev, "pafc_rnnt_greedy_stream_workspace_bytes", (self._pnet, B, Tmax, n_steps))
        self._x = torch.zeros(B * Tmax, D, dtype=self.dtype, device=dev)
        self._E = torch.empty(B * Tmax, J, dtype=self.dtype, device=dev)
        self._running = torch.zeros(1, dtype=torch.int32, device=dev)
        self._graphs = {}
        self._last_n = None
        self._score = [0.0] * B
        self.last_steps = 0
        self.reset()

    def reset(self, rows=None):
        """Restart the given rows (all when None): a fresh decode from their next chunk on; other rows are untouched."""
        st = _lib.stream_of(self._ws)
        mask = self._row_mask(rows)
        for b in (range(self.B) if rows is None else rows):
            self._score[b] = 0.0
        _lib.check(self._L.pafc_rnnt_greedy_stream_reset(self._pnet, self.B, self.Tmax, self.n_steps, self.blank, mask,
                                                          _lib.ptr(self._ws), self._nbytes, st), "pafc_rnnt_greedy_stream_reset")

    def _step(self, st):
        _lib.check(self._L.pafc_rnnt_greedy_step(self._pnet, self.B, self.Tmax, self.n_steps, self.blank, _lib.ptr(self._E),
                                                 _lib.ptr(self._ws), self._nbytes, _lib.ptr(self._running), st),
                   "pafc_rnnt_greedy_step")

    def _fixed(self, n):
        """The fixed part of a feed of n frames: E projection, feed kernel, n steps."""
        st = _lib.stream_of(self._ws)
        _enc_project(self._x, self._w, self._b, out=self._E)
        _lib.check(self._L.pafc_rnnt_greedy_stream_feed(self._pnet, self.B, self.Tmax, self.n_steps, self.blank,
                                                         _lib.ptr(self._nf), _lib.ptr(self._ws), self._nbytes,
                                                         _lib.ptr(self._running), st), "pafc_rnnt_greedy_stream_feed")
        for _ in range(n):
            self._step(st)

    def _run_fixed(self, n):
        g = self._graphs.get(n, False)
        if g is False and self.use_graph:
            # capture once per n; only a REFUSED capture (nothing ran: the state is as before) finishes eagerly, for good
            g = self._graphs[n] = graph_step.capture(lambda: self._fixed(n), self.device)[0]
        if g:
            g.replay()
        else:
            self._fixed(n)

    @property
    def graphed(self) -> bool:
        """Whether the last feed replayed a captured graph."""
        return bool(self._graphs.get(self._last_n, None)) if self.use_graph else False

    def feed(self, encoder_chunk: torch.Tensor, nframes=None):
        """Decode one chunk (B, n, D), n <= Tmax.  Returns (tokens, frames): per row the tokens emitted in this chunk and
        their absolute frame indices (frames since the row's reset)."""
        B, Tmax = self.B, self.Tmax
        if encoder_chunk.dim() != 3 or encoder_chunk.shape[0] != B or encoder_chunk.shape[2] != self.D:
            raise _lib.PafcError(f"RnntGreedyStream.feed: the chunk must be ({B}, n, {self.D})")
        n = encoder_chunk.shape[1]
        if not 0 <= n <= Tmax:
            raise _lib.PafcError(f"RnntGreedyStream.feed: {n} frames, at most Tmax = {Tmax}")
        if encoder_chunk.device != self.device:
            raise _lib.PafcError("RnntGreedyStream.feed: the chunk is not on the weights' GPU")
        if n:
            self._x.view(B, Tmax, self.D)[:, :n].copy_(encoder_chunk.detach())
        self._set_nframes(nframes, n)
        self._last_n = n
        self._run_fixed(n)
        st = _lib.stream_of(self._ws)
        steps = n
        limit = n * (self.n_steps + 1)                 # every row ends its frames within n (n_steps + 1) decisions
        while int(self._running.item()) != 0:          # the host read after the fixed part and after every further chunk
            if steps >= limit:
                raise _lib.PafcError("RnntGreedyStream.feed: rows still running after n * (n_steps + 1) steps")
            for _ in range(self.chunk):
                self._step(st)
            steps += self.chunk
        self.last_steps = steps
        ld = max(1, steps)                             # a row emits at most one token per step
        out = _Packed([("score", torch.float64, (B,)), ("frames", torch.int64, (B, ld)), ("ntok", torch.int32, (B,)),
                       ("tokens", torch.int32, (B, ld))], self.device)
        _lib.check(self._L.pafc_rnnt_greedy_stream_drain(self._pnet, B, Tmax, self.n_steps, _lib.ptr(self._ws), self._nbytes, ld,
                                                          out.ptr("tokens"), out.ptr("frames"), out.ptr("ntok"),
                                                          out.ptr("score"), None, st), "pafc_rnnt_greedy_stream_drain")
        out.read()                                     # the final read
        self._score = out.host("score").tolist()
        f_h, n_h, t_h = out.host("frames"), out.host("ntok").tolist(), out.host("tokens")
        return [t_h[b, :n_h[b]].tolist() for b in range(B)], [f_h[b, :n_h[b]].tolist() for b in range(B)]

    @property
    def score(self) -> List[float]:
        """Per row the path score (float64 sum of log p over every decision) since its reset, as of the last feed."""
        return list(self._score)


PAFC_SPLIT_BF16 = 2      # output form: an fp32 value as bf16 planes [hi | lo] (include/pafc_wkv6.h)


def add_layernorm(x: torch.Tensor, y: Optional[torch.Tensor], alpha: float, gamma1, beta1, *, out1: torch.Tensor = None,
                  out_dtype: Optional[torch.dtype] = None, silu: bool = False, zero_rows: bool = False,
                  lens: Optional[torch.Tensor] = None, T: int = 0, mask_y: bool = False, gamma2=None, beta2=None,
                  want_ln: bool = True, want_x: bool = True, eps: float = 1e-5, split1: bool = False, split2: bool = False,
                  stats_x: Optional[torch.Tensor] = None, stats_out1: Optional[torch.Tensor] = None):
    """x_new = x + alpha*y; out1 = LN1(x_new) [silu] [rows >= len zeroed]; out2 = LN2(out1).
    Returns (x_new or x, out1 or None, out2 or None).  `out1` may be a pre-allocated (rows, ld) view (last-dim
    slice of a wider buffer) so that two LayerNorms can land side by side.
    split1 / split2 (fp32 x only): that output comes as bf16 planes (..., 2C) = [hi | lo] of the fp32 result, the A operand
    of gemm_ph_ex(a_split=True); split1 implies split2.
    stats_x / stats_out1: float32 (rows, 8, 2) buffers that receive the row statistics of x_new / of out1 (gemm_bf16_ln)."""
    _lib.require_gpu(x, y, gamma1, beta1, gamma2, beta2, lens)
    C = x.shape[-1]
    rows = x.numel() // C
    out_dtype = out_dtype or x.dtype
    if (split1 or split2) and (x.dtype != torch.float32 or out_dtype != torch.float32 or out1 is not None):
        raise _lib.PafcError("add_layernorm: plane outputs are a form of an fp32 result")
    x_out = torch.empty_like(x) if (y is not None and want_x) else None
    o1 = None
    ld1 = C
    planes = lambda: torch.empty(x.shape[:-1] + (2 * C,), dtype=torch.bfloat16, device=x.device)
    if want_ln:
        if split1:
            o1, ld1 = planes(), 2 * C
        elif out1 is None:
            o1 = torch.empty(x.shape, dtype=out_dtype, device=x.device)
        else:
            o1 = out1
            ld1 = out1.stride(-2)
            if out1.stride(-1) != 1 or out1.dtype != out_dtype:
                raise _lib.PafcError("out1 must be a unit-stride view in the output dtype")
    s2 = split1 or split2
    o2 = None
    if gamma2 is not None:
        o2 = planes() if s2 else torch.empty(x.shape, dtype=out_dtype, device=x.device)
    L = _lib.lib()
    code = _lib.dtype_code(out_dtype)
    rc = L.pafc_add_layernorm_ex(
        _lib.dtype_code(x.dtype), PAFC_SPLIT_BF16 if split1 else code, PAFC_SPLIT_BF16 if s2 else code, rows, C, _lib.ptr(x),
        _lib.ptr(y), float(alpha), _lib.ptr(lens), int(T), int(mask_y), _lib.ptr(x_out), _lib.ptr(gamma1), _lib.ptr(beta1),
        _lib.ptr(o1), ld1, int(silu), int(zero_rows), _lib.ptr(gamma2), _lib.ptr(beta2), _lib.ptr(o2), 2 * C if s2 else C,
        float(eps), _lib.ptr(stats_x), _lib.ptr(stats_out1), _lib.stream_of(x))
    _lib.check(rc, "pafc_add_layernorm")
    return (x_out if y is not None else x), o1, o2  # first item is None when want_x=False


def gemm_bf16_ln(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stats: torch.Tensor, *, act: str = "none",
                 alpha: float = 1.0, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 csum: Optional[torch.Tensor] = None, ln_c: int = 0, eps: float = 1e-5) -> torch.Tensor:
    """The bf16 GEMMs either side of a folded pre-norm LayerNorm (include/pafc_encoder_ops.h: pafc_gemm_bf16_ph_ln).
    csum given: the CONSUMER -- act(rstd (a w^T) - rstd mean csum + bias), a = the un-normalised rows, w = gamma * W, act
    "silu" | "glu", row statistics READ from stats (rows, 8, 2) fp32.  csum None: the PRODUCER -- alpha a w^T + bias + residual
    (N = 512) with the rows' statistics WRITTEN to stats."""
    _lib.require_gpu(bias, stats, csum)
    for t in (a, w, residual, out):
        if t is not None and (not t.is_cuda or t.dtype != torch.bfloat16 or t.stride(-1) != 1 or t.dim() != 2):
            raise _lib.PafcError("gemm_bf16_ln: 2-d bf16 GPU tensors with unit stride in the last dimension")
    M, K = a.shape
    N = w.shape[0]
    No = N // 2 if act == "glu" else N
    if stats.dtype != torch.float32 or stats.numel() != M * 16 or not stats.is_contiguous():
        raise _lib.PafcError("gemm_bf16_ln: stats is a contiguous float32 (M, 8, 2) buffer")
    if out is None:
        out = torch.empty((M, No), dtype=a.dtype, device=a.device)
    L = _lib.lib()
    from .profiling import op_timer
    with op_timer("gemm_%dx%d" % (K, N), sample=12, flops=2.0 * M * N * K):
        rc = L.pafc_gemm_bf16_ph_ln(M, N, K, _lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(bias), _lib.ptr(residual),
                                    residual.stride(0) if residual is not None else 0, _lib.ptr(out), out.stride(0), float(alpha),
                                    _ACTS[act], 1 if csum is not None else 2, _lib.ptr(stats), _lib.ptr(csum),
                                    int(ln_c or (K if csum is not None else N)),
                                    float(eps), _ph_tile_m(M, N, min_tm=128), _lib.stream_of(a))
    _lib.check(rc, "pafc_gemm_bf16_ph_ln")
    return out


def split_planes(x: torch.Tensor, triple: bool = False) -> torch.Tensor:
    """fp32 (..., K) -> bf16 (..., 2K) = [hi | lo] with hi = bf16(x), lo = bf16(x - hi) (an activation for
    gemm_ph_ex(a_split=True)), or, triple, (..., 3K) = [hi | hi | lo] (its weight)."""
    _lib.require_gpu(x)
    if x.dtype != torch.float32 or x.stride(-1) != 1:
        raise _lib.PafcError("split_planes: contiguous fp32 input")
    K = x.shape[-1]
    rows = x.numel() // K
    out = torch.empty(x.shape[:-1] + ((3 if triple else 2) * K,), dtype=torch.bfloat16, device=x.device)
    L = _lib.lib()
    _lib.check(L.pafc_split_planes(rows, K, _lib.ptr(x), K, _lib.ptr(out), out.shape[-1], K, int(triple), _lib.stream_of(x)),
               "pafc_split_planes")
    return out


def _ph_tile_m(M: int, N: int, batch: int = 1, min_tm: int = 64) -> int:
    """Rows per tile of the phase-pipelined GEMM for this problem (the count that needs the fewest rounds of one-tile-per-CU
    work, a round weighted by its rows plus a fixed per-tile part worth ~64 rows), as csrc/gemm_bf16.hip:ph_tile_m."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    nt = (N + 255) // 256
    best = None
    for tm in (256, 192, 128, 64):      # (64: a few thousand fp32 rows as split operands, profiles/r05_split_mid_rows.txt)
        if tm < min_tm:
            continue
        tiles = ((M + tm - 1) // tm) * nt * batch
        cost = ((tiles + cus - 1) // cus) * (tm + 64)
        if best is None or cost < best[0]:
            best = (cost, tm)
    return best[1]


def _ph_ktail_plan(M: int, N: int, K: int, cus: int, batch: int = 1, min_k: Optional[int] = None):
    """The tail plan of a split-operand, fp32-output problem on 256-row tiles (as csrc/gemm_bf16.hip:pafc_gemm_ph_ktail_plan):
    (split_row, kslices = 2) when the last round of one-tile-per-CU work covers at most half of the CUs -- its row tiles then
    run once per half of K (pafc_gemm_ph_ktail) -- or None.  At most one tail round is split, and in two."""
    min_k = DISPATCH["ktail_min_k"] if min_k is None else min_k
    if M <= 0 or N <= 0 or K <= 0 or batch != 1 or cus <= 0:
        return None
    ntiles = (N + 255) // 256
    tiles = ((M + 255) // 256) * ntiles
    full = tiles // cus * cus
    tail = tiles - full
    if full <= 0 or tail <= 0 or 2 * tail > cus or full % ntiles:
        return None
    if K % 128 or K < min_k:            # K / 32 steps: an even number of them in each of the two slices
        return None
    return full // ntiles * 256, 2


_TAIL_AUTO = object()           # tail_split left to _ph_ktail_plan


def gemm_ph_ex(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none", alpha: float = 1.0,
               residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, a_split: bool = False,
               out_kind: str = "bf16", tile_m: int = 0, a_plane_block: int = 0, tail_split=_TAIL_AUTO) -> torch.Tensor:
    """The phase-pipelined GEMM with every operand form (include/pafc_encoder_ops.h: pafc_gemm_ph_ex).
    a: (M, K) bf16, or with a_split (M, 2K) planes [hi | lo] of an fp32 activation, then w: (N, 3K) = split_planes(W, triple=True);
    out_kind "bf16" | "f32" | "planes" ((M, 2N) bf16 = [hi | lo] of the fp32 result); residual bf16 (out bf16) or fp32 (out f32),
    may be `out`; bias bf16 for out_kind bf16, fp32 otherwise; act as gemm_bf16 (GLU: glu_interleave(w, 32) rows before splitting).
    a_plane_block: the planes of a split `a` alternate in blocks of that many columns ([hi PB | lo PB] ...; 0: [hi K | lo K]).
    tail_split: (split_row, kslices) runs the rows from split_row on as K slices + a fix-up pass (pafc_gemm_ph_ktail); None /
    False: one launch; by default _ph_ktail_plan decides (split operands -> fp32 without an activation, no tile_m given)."""
    _lib.require_gpu(bias)
    for t in (a, w, residual, out):
        if t is not None and (not t.is_cuda or t.stride(-1) != 1):
            raise _lib.PafcError("gemm_ph_ex: GPU tensors with unit stride in the last dimension")
    if a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or a.dim() != 2 or w.dim() != 2:
        raise _lib.PafcError("gemm_ph_ex: a and w are 2-d bf16 (planes of fp32 operands with a_split)")
    M = a.shape[0]
    N = w.shape[0]
    K = w.shape[1] // 3 if a_split else w.shape[1]
    if a.shape[1] != (2 * K if a_split else K) or (a_split and w.shape[1] != 3 * K):
        raise _lib.PafcError("gemm_ph_ex: a (M, K) x w (N, K); split: a (M, 2K) x w (N, 3K)")
    No = N // 2 if act == "glu" else N
    kinds = {"bf16": (0, torch.bfloat16, No), "f32": (1, torch.float32, No), "planes": (2, torch.bfloat16, 2 * No)}
    ok, odt, ocols = kinds[out_kind]
    if out is None:
        out = torch.empty((M, ocols), dtype=odt, device=a.device)
    if out.dtype != odt or tuple(out.shape) != (M, ocols):
        raise _lib.PafcError("gemm_ph_ex: out must be (M, N) in the output form's dtype ((M, 2N) bf16 for planes)")
    rk = 0
    if residual is not None:
        rk = 1 if residual.dtype == torch.bfloat16 else 2
        if tuple(residual.shape) != (M, N) or residual.dtype != (torch.bfloat16 if ok == 0 else torch.float32) or ok == 2:
            raise _lib.PafcError("gemm_ph_ex: residual (M, N) in the output dtype (bf16 / fp32), not with planes")
    if bias is not None and (bias.dtype != (torch.bfloat16 if ok == 0 else torch.float32) or bias.numel() != N):
        raise _lib.PafcError("gemm_ph_ex: bias (N) bf16 for a bf16 output, fp32 otherwise")
    L = _lib.lib()
    from .profiling import op_timer
    pb_ok = not a_plane_block or (a_split and a_plane_block >= 64 and a_plane_block & (a_plane_block - 1) == 0 and K % a_plane_block == 0)
    if (M <= _SPLIT_SMALL_MAX_ROWS and M * N <= _SPLIT_SMALL_MAX_OUT and ok != 0 and act in ("none", "silu", "tanh", "relu")
            and pb_ok and not tile_m and K % 64 == 0 and (tail_split is _TAIL_AUTO or not tail_split)):
        # few rows: the small tiles of csrc/gemm_bf16.hip (same operand forms, same epilogue order)
        nws = L.pafc_gemm_bf16_f32out_workspace_bytes(M, N, K, int(a_split))     # > 0: few rows x long K, K split over blocks
        ws = torch.empty(nws, dtype=torch.uint8, device=a.device) if nws else None
        with op_timer("gemm%ss_%dx%d" % ("3" if a_split else "", K, N), sample=12, flops=2.0 * M * N * K * (3 if a_split else 1)):
            rc = L.pafc_gemm_bf16_f32out_pb(M, N, K, _lib.ptr(a), a.stride(0), int(a_split), int(a_plane_block), _lib.ptr(w), w.stride(0),
                                            _lib.ptr(bias), _lib.ptr(residual), residual.stride(0) if residual is not None else 0,
                                            _lib.ptr(out), ok, out.stride(0), No if ok == 2 else 0, float(alpha), _ACTS[act], _lib.ptr(ws),
                                            nws, _lib.stream_of(a))
        _lib.check(rc, "pafc_gemm_bf16_f32out")
        return out
    if tail_split is _TAIL_AUTO:
        tail_split = None
        if a_split and ok == 1 and act == "none" and not tile_m and os.environ.get("PAFC_SPLIT_WALK") != "hilohi":
            cus = torch.cuda.get_device_properties(a.device).multi_processor_count
            tail_split = _ph_ktail_plan(M, N, K, cus)
    if tail_split:
        split_row, kslices = tail_split
        # the slices' partial products: allocated on the current stream (capture-safe, one per call: batches in flight share nothing)
        nws = max(0, kslices * (M - split_row) * N * 4)
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=a.device)
        with op_timer("gemm%s_%dx%d" % ("3" if a_split else "", K, N), sample=12, flops=2.0 * M * N * K * (3 if a_split else 1)):
            rc = L.pafc_gemm_ph_ktail(M, N, K, 1, _lib.ptr(a), a.stride(0), 0, int(a_split), int(a_plane_block), _lib.ptr(w),
                                      w.stride(0), 0, _lib.ptr(bias), 0, _lib.ptr(residual), rk,
                                      residual.stride(0) if residual is not None else 0, 0, _lib.ptr(out), ok, out.stride(0),
                                      No if ok == 2 else 0, 0, float(alpha), _ACTS[act], int(tile_m or 256), _lib.ptr(ws), nws,
                                      int(split_row), int(kslices), _lib.stream_of(a))
        _lib.check(rc, "pafc_gemm_ph_ktail")
        return out
    with op_timer("gemm%s_%dx%d" % ("3" if a_split else "", K, N), sample=12, flops=2.0 * M * N * K * (3 if a_split else 1)):
        rc = L.pafc_gemm_ph_ex2(M, N, K, 1, _lib.ptr(a), a.stride(0), 0, int(a_split), int(a_plane_block), _lib.ptr(w), w.stride(0), 0,
                                _lib.ptr(bias), 0,
                               _lib.ptr(residual), rk, residual.stride(0) if residual is not None else 0, 0, _lib.ptr(out), ok,
                               out.stride(0), No if ok == 2 else 0, 0, float(alpha), _ACTS[act], int(tile_m or _ph_tile_m(M, N)),
                               _lib.stream_of(a))
    _lib.check(rc, "pafc_gemm_ph_ex")
    return out


_SPLIT_SMALL_MAX_ROWS = DISPATCH["split_small_max_rows"]
_SPLIT_SMALL_MAX_OUT = 1 << 22          # ... and at most this many outputs (rows x columns)


def wkv6_single_chunk(B: int, T: int, C: int, H: int) -> bool:
    """Does the library walk a (B, T, C) one-direction scan as ONE chunk (then the carried state may be updated in place)?"""
    return _lib.lib().pafc_wkv6_pick_chunk_len(B, T, C, H, 1) >= T


def _check_prev(prev: Optional[torch.Tensor], x: torch.Tensor):
    """prev: (B, 1, C) / (B, C) = the frame before each sequence's first one (streaming), same dtype as x, contiguous."""
    if prev is not None and (prev.dtype != x.dtype or prev.numel() != x.shape[0] * x.shape[2] or not prev.is_contiguous()
                             or prev.device != x.device):
        raise _lib.PafcError("tmix: prev must be a contiguous (B, C) tensor of x's dtype on x's device")


def tmix_shift_mix(x: torch.Tensor, maa_x0: torch.Tensor, maa_x1: Optional[torch.Tensor], reverse0: bool = False,
                   prev: Optional[torch.Tensor] = None):
    """(B, T, C) -> (ndir, B, T, C): x + (shift_d(x) - x) * maa_x_d.  prev: the frame before the chunk (streaming), or None."""
    _lib.require_gpu(x, maa_x0, maa_x1, prev)
    _check_prev(prev, x)
    B, T, C = x.shape
    ndir = 2 if maa_x1 is not None else 1
    out = torch.empty((ndir, B, T, C), dtype=x.dtype, device=x.device)
    rc = _lib.lib().pafc_tmix_shift_mix_prev(_lib.dtype_code(x.dtype), B, T, C, ndir, int(reverse0), _lib.ptr(x),
                                             _lib.ptr(maa_x0), _lib.ptr(maa_x1), _lib.ptr(prev), _lib.ptr(out), _lib.stream_of(x))
    _lib.check(rc, "pafc_tmix_shift_mix")
    return out


def tmix_mix4(x: torch.Tensor, m: torch.Tensor, maa: torch.Tensor, reverse0: bool = False):
    """x (B,T,C), m (ndir,4,B*T,C), maa (ndir,4,C) -> z (4,ndir,B*T,C)."""
    _lib.require_gpu(x, m, maa)
    B, T, C = x.shape
    ndir = m.shape[0]
    if m.dtype != x.dtype or maa.dtype != x.dtype:
        raise _lib.PafcError("tmix_mix4: x, m and maa must share one dtype")
    z = torch.empty((4, ndir, B * T, C), dtype=x.dtype, device=x.device)
    rc = _lib.lib().pafc_tmix_mix4(_lib.dtype_code(x.dtype), B, T, C, ndir, int(reverse0), _lib.ptr(x), _lib.ptr(m),
                                   _lib.ptr(maa), _lib.ptr(z), _lib.stream_of(x))
    _lib.check(rc, "pafc_tmix_mix4")
    return z


class _ShiftMixTrain(torch.autograd.Function):
    """xxx = x + (shift(x) - x) * maa_x (src/model.py:274-276) for one direction: forward tmix_shift_mix, backward one
    pass (pafc_tmix_shift_mix_bwd) instead of the framework's pad / sub / mul / add chain and its reduction."""

    @staticmethod
    def forward(ctx, x, maa_x, reverse):
        mx = maa_x.reshape(-1).to(x.dtype).contiguous()
        ctx.save_for_backward(x, mx)
        ctx.reverse, ctx.maa_shape, ctx.maa_dtype = reverse, maa_x.shape, maa_x.dtype
        return tmix_shift_mix(x, mx, None, reverse)[0]

    @staticmethod
    def backward(ctx, dxxx):
        x, mx = ctx.saved_tensors
        B, T, C = x.shape
        L = _lib.lib()
        nbytes = L.pafc_tmix_bwd_workspace_bytes(B * T, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        dx = torch.empty_like(x)
        dmaa = torch.empty(C, dtype=torch.float32, device=x.device)
        dxxx = dxxx.contiguous()
        rc = L.pafc_tmix_shift_mix_bwd(_lib.dtype_code(x.dtype), B, T, C, int(ctx.reverse), _lib.ptr(x), _lib.ptr(mx),
                                       _lib.ptr(dxxx), _lib.ptr(dx), _lib.ptr(dmaa), _lib.ptr(ws), nbytes, _lib.stream_of(x))
        _lib.check(rc, "pafc_tmix_shift_mix_bwd")
        return dx, dmaa.to(ctx.maa_dtype).view(ctx.maa_shape), None


class _Mix4Train(torch.autograd.Function):
    """z_q = x + (shift(x) - x) * (maa_q + m_q), q = r, k, v, w (src/model.py:280-284) for one direction: forward
    tmix_mix4, backward one pass (pafc_tmix_mix4_bwd).  Returns the four maps as separate outputs so that autograd hands
    back four gradients instead of assembling one stacked tensor."""

    @staticmethod
    def forward(ctx, x, m, maa4, reverse):
        B, T, C = x.shape
        mm = m.reshape(1, 4, B * T, C).to(x.dtype).contiguous()     # under autocast the LoRA product is bf16, x may be fp32
        a4 = maa4.reshape(1, 4, C).to(x.dtype).contiguous()
        z = tmix_mix4(x, mm, a4, reverse)                           # (4, 1, B*T, C)
        ctx.save_for_backward(x, mm, a4)
        ctx.reverse, ctx.maa_shape, ctx.maa_dtype, ctx.m_shape, ctx.m_dtype = reverse, maa4.shape, maa4.dtype, m.shape, m.dtype
        return tuple(z[q, 0].view(B, T, C) for q in range(4))

    @staticmethod
    def backward(ctx, *dz):
        x, mm, a4 = ctx.saved_tensors
        B, T, C = x.shape
        dz = [(torch.zeros_like(x) if g is None else g.contiguous()) for g in dz]
        L = _lib.lib()
        nbytes = L.pafc_tmix_bwd_workspace_bytes(B * T, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        dx = torch.empty_like(x)
        dm = torch.empty_like(mm)
        dmaa = torch.empty(4, C, dtype=torch.float32, device=x.device)
        P = _lib.ptr
        rc = L.pafc_tmix_mix4_bwd(_lib.dtype_code(x.dtype), B, T, C, int(ctx.reverse), P(x), P(mm), P(a4), P(dz[0]), P(dz[1]),
                                  P(dz[2]), P(dz[3]), P(dx), P(dm), P(dmaa), P(ws), nbytes, _lib.stream_of(x))
        _lib.check(rc, "pafc_tmix_mix4_bwd")
        return dx, dm.view(ctx.m_shape).to(ctx.m_dtype), dmaa.to(ctx.maa_dtype).view(ctx.maa_shape), None


_eye4 = {}      # device -> (4, 1, 4, 1) bf16 identity: the block-diagonal placement of the four LoRA-up matrices


class _LoraMix4Train(torch.autograd.Function):
    """m_q = t_q W2_q (the LoRA-up products, src/model.py:277-278: `torch.bmm` over four (B*T, 32) x (32, C) pairs) followed by the
    four lerps z_q = x + (shift(x) - x) (maa_q + m_q) (280-284), for one direction, every product on the hand-written kernels:
      forward   m = t (B*T, 128) against the four matrices laid out block-diagonally along K ((4, C, 128): block q of the K axis
                holds W2_q^T, zeros elsewhere -- 4 x the flops of a product that is 2 GFLOP) as ONE batched pafc_gemm_bf16, then
                pafc_tmix_mix4;
      backward  pafc_tmix_mix4_bwd_rows leaves dm as (B*T, 4, C); dt = ONE batched pafc_gemm_bf16 (dm's four column blocks against
                W2_q as they lie, into the four column blocks of dt); dW2 = the diagonal blocks of ONE pafc_gemm_tn_bf16
                t^T (128, B*T) x dm (B*T, 4 C).
    Round 5 ran the three products through the library (Cijk MT256x256x32 32 us, MT32x128x32 19 us, MT16x16x128 74 us per direction
    and layer) with a transposed copy of t in front of the last one."""

    @staticmethod
    def forward(ctx, x, t, w2, maa_r, maa_k, maa_v, maa_w, reverse):
        B, T, C = x.shape
        M, R = B * T, w2.shape[1]
        maas = (maa_r, maa_k, maa_v, maa_w)
        maa4 = _params_as_one(maas)                                               # (4, C): no launch once the four live in one buffer
        if maa4 is None:
            maa4 = torch.stack([m_.detach().reshape(C) for m_ in maas])
        tb = t.reshape(M, 4 * R)
        if tb.dtype != torch.bfloat16 or not tb.is_contiguous():
            tb = tb.to(torch.bfloat16).contiguous()
        w2b = _param_as(w2, torch.bfloat16).contiguous()                          # (4, R, C)
        eye = _eye4.get(x.device)
        if eye is None:
            eye = _eye4[x.device] = torch.eye(4, dtype=torch.bfloat16, device=x.device).view(4, 1, 4, 1)
        w2p = torch.empty((4, C, 4, R), dtype=torch.bfloat16, device=x.device)
        torch.mul(w2b.transpose(1, 2).unsqueeze(2), eye, out=w2p)                  # one launch
        w2p = w2p.view(4, C, 4 * R)
        m = gemm_bf16(tb.unsqueeze(0).expand(4, M, 4 * R), w2p)                    # (4, M, C)
        mm = m.view(1, 4, M, C) if x.dtype == torch.bfloat16 else m.view(1, 4, M, C).to(x.dtype)
        a4 = maa4.reshape(1, 4, C).to(x.dtype).contiguous()
        z = tmix_mix4(x, mm, a4, reverse)                                          # (4, 1, M, C)
        ctx.save_for_backward(x, tb, w2b, mm, a4)
        ctx.reverse, ctx.maa_shape, ctx.maa_dtype, ctx.t_shape, ctx.t_dtype, ctx.w2_dtype = (reverse, maa_r.shape, maa_r.dtype, t.shape,
                                                                                             t.dtype, w2.dtype)
        return tuple(z[q, 0].view(B, T, C) for q in range(4))

    @staticmethod
    def backward(ctx, *dz):
        x, tb, w2b, mm, a4 = ctx.saved_tensors
        B, T, C = x.shape
        M, R = B * T, w2b.shape[1]
        dz = [(torch.zeros_like(x) if g is None else g.contiguous()) for g in dz]
        L = _lib.lib()
        nbytes = L.pafc_tmix_bwd_workspace_bytes(M, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        dx = torch.empty_like(x)
        dm = torch.empty((M, 4, C), dtype=x.dtype, device=x.device)
        dmaa = torch.empty(4, C, dtype=torch.float32, device=x.device)
        P = _lib.ptr
        rc = L.pafc_tmix_mix4_bwd_rows(_lib.dtype_code(x.dtype), B, T, C, int(ctx.reverse), P(x), P(mm), P(a4), P(dz[0]), P(dz[1]),
                                       P(dz[2]), P(dz[3]), P(dx), P(dm), P(dmaa), P(ws), nbytes, _lib.stream_of(x))
        _lib.check(rc, "pafc_tmix_mix4_bwd_rows")
        if dm.dtype != torch.bfloat16:
            dm = dm.to(torch.bfloat16)
        dt = dw2 = None
        if ctx.needs_input_grad[1]:
            dt = torch.empty((M, 4 * R), dtype=torch.bfloat16, device=x.device)
            gemm_bf16(dm.transpose(0, 1), w2b, out=dt.view(M, 4, R).transpose(0, 1))    # (4, M, C) x (4, R, C)^T -> (4, M, R)
            dt = dt.view(ctx.t_shape).to(ctx.t_dtype)
        if ctx.needs_input_grad[2]:
            od = ctx.w2_dtype if ctx.w2_dtype in (torch.float32, torch.bfloat16) else torch.float32
            full = gemm_tn(tb, dm.view(M, 4 * C), od)                                  # (4 R, 4 C): its diagonal blocks
            dw2 = torch.stack([full[q * R:(q + 1) * R, q * C:(q + 1) * C] for q in range(4)]).to(ctx.w2_dtype)
        dm4 = dmaa.to(ctx.maa_dtype)
        return (dx, dt, dw2, dm4[0].view(ctx.maa_shape), dm4[1].view(ctx.maa_shape), dm4[2].view(ctx.maa_shape),
                dm4[3].view(ctx.maa_shape), None)


def lora_mix4_train_eligible(x: torch.Tensor, t: torch.Tensor, w2: torch.Tensor) -> bool:
    """The LoRA-up + lerp group on own kernels: the element-wise group's conditions, bf16 LoRA activations, four (R, C) matrices with
    4 R a multiple of 64 (the K axis of the block-diagonal product) and C of 64 (that of the input-gradient product)."""
    if os.environ.get("PAFC_TRAIN_LORA_UP", "1") == "0":          # A/B runs: torch.bmm + mix4_train, as in round 5
        return False
    return (tmix_train_eligible(x) and train_gemms_own() and t.dtype == torch.bfloat16 and w2.dim() == 3 and w2.shape[0] == 4
            and (4 * w2.shape[1]) % 64 == 0 and w2.shape[2] == x.shape[-1] and x.shape[-1] % 64 == 0
            and w2.dtype in (torch.float32, torch.bfloat16) and t.numel() == x.shape[0] * x.shape[1] * 4 * w2.shape[1])


def lora_mix4_train(x: torch.Tensor, t: torch.Tensor, w2: torch.Tensor, maas, reverse: bool):
    """t: (B, T, 4 R) = tanh(xxx W1); w2: (4, R, C); maas: the four lerp coefficients (time_maa_r, _k, _v, _w), C elements each.
    -> z_r, z_k, z_v, z_w (B, T, C)."""
    return _LoraMix4Train.apply(x.contiguous(), t, w2, *maas, reverse)


def tmix_train_eligible(x: torch.Tensor) -> bool:
    return (x.is_cuda and torch.is_grad_enabled() and train_kernels_enabled() and x.dim() == 3
            and x.dtype in (torch.float32, torch.bfloat16) and x.shape[-1] % 8 == 0 and x.shape[-1] <= 1024)


def shift_mix_train(x: torch.Tensor, maa_x: torch.Tensor, reverse: bool) -> torch.Tensor:
    return _ShiftMixTrain.apply(x.contiguous(), maa_x, reverse)


def mix4_train(x: torch.Tensor, m: torch.Tensor, maa4: torch.Tensor, reverse: bool):
    """m: (4, B, T, C) LoRA outputs in the order r, k, v, w; maa4: (4, C) (or anything that reshapes to it)."""
    return _Mix4Train.apply(x.contiguous(), m, maa4, reverse)


def _gemm_operands(op: str, dtype: torch.dtype, a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor],
                   residual: Optional[torch.Tensor], out: Optional[torch.Tensor], act: str):
    """The operand checks of the dense GEMM front ends (gemm_f32, gemm_bf16, gemm_skinny, gemm_bf16_ph): a (M, K) x w (N, K), or
    both with a leading batch Z, in `dtype` with unit stride in the last dimension; bias (N) or (Z, N); residual / out (M, N_out)
    per batch entry, N_out = N / 2 for act "glu".  Allocates `out` when it is None.  Returns (Z, M, N, K, out, the 18 leading
    arguments of the kernels: M, N, K, Z, then pointer, row stride and batch stride of a, w, residual and out, and of bias
    pointer and batch stride)."""
    _lib.require_gpu(bias)
    for t in (a, w, residual, out):
        if t is not None and (not t.is_cuda or t.dtype != dtype or t.stride(-1) != 1):
            raise _lib.PafcError(f"{op}: {_DT_NAMES[dtype]} GPU tensors with unit stride in the last dimension")
    batched = a.dim() == 3
    Z = a.shape[0] if batched else 1
    M, K = a.shape[-2], a.shape[-1]
    N = w.shape[-2]
    if w.shape[-1] != K or (batched and (w.dim() != 3 or w.shape[0] != Z)) or (not batched and (a.dim() != 2 or w.dim() != 2)):
        raise _lib.PafcError(f"{op}: a (M, K) x w (N, K), or both with a leading batch")
    No = N // 2 if act == "glu" else N
    shape = (Z, M, No) if batched else (M, No)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=a.device)
    for t in (residual, out):
        if t is not None and tuple(t.shape) != shape:
            raise _lib.PafcError(f"{op}: residual / out must be (M, N) per batch entry")
    if bias is not None and (bias.dtype != dtype or bias.shape[-1] != N):
        raise _lib.PafcError(f"{op}: bias must be (N) or (Z, N) {_DT_NAMES[dtype]}")
    bs = lambda t: t.stride(0) if batched and t is not None else 0
    return Z, M, N, K, out, (M, N, K, Z, _lib.ptr(a), a.stride(-2), bs(a), _lib.ptr(w), w.stride(-2), bs(w), _lib.ptr(bias),
                             bias.stride(0) if (bias is not None and bias.dim() == 2) else 0, _lib.ptr(residual),
                             residual.stride(-2) if residual is not None else 0, bs(residual), _lib.ptr(out), out.stride(-2),
                             bs(out))


_DT_NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none", alpha: float = 1.0,
             residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Hand-written fp32 GEMM with a fused epilogue on the fp32 matrix cores (include/pafc_encoder_ops.h: pafc_gemm_f32; exact
    fp32 products, fp32 accumulation): act(alpha * a w^T + bias + residual).  a: (M, K) or (Z, M, K); w: (N, K) or (Z, N, K) in
    nn.Linear layout; bias (N) or (Z, N); residual / out (M, N) or (Z, M, N), `out` may be `residual`.  Rows and batch entries
    may be strided views (unit stride in the last dimension; K and the strides of a and w multiples of 4).  act: none / silu /
    tanh / relu.  No workspace, no plan objects: safe to issue from several streams at once."""
    if act not in ("none", "silu", "tanh", "relu"):
        raise _lib.PafcError("gemm_f32: act is none / silu / tanh / relu")
    Z, M, N, K, out, args = _gemm_operands("gemm_f32", torch.float32, a, w, bias, residual, out, act)
    from .profiling import op_timer
    with op_timer("gemmf32_%dx%d%s" % (K, N, "x%d" % Z if a.dim() == 3 else ""), sample=12, flops=2.0 * Z * M * N * K):
        rc = _lib.lib().pafc_gemm_f32(*args, float(alpha), _ACTS[act], _lib.stream_of(a))
    _lib.check(rc, "pafc_gemm_f32")
    return out


def gemm_f32_ok(a: torch.Tensor, w: torch.Tensor) -> bool:
    """Operand forms pafc_gemm_f32 takes: fp32, unit stride along K, K and the row / batch strides multiples of 4, 16-byte bases."""
    return (a.is_cuda and a.dtype == torch.float32 and w.dtype == torch.float32 and a.shape[-1] % 4 == 0
            and all(t.stride(-1) == 1 and all(st % 4 == 0 for st in t.stride()[:-1]) and t.data_ptr() % 16 == 0 for t in (a, w)))


def linear_bias_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "silu",
                    alpha: float = 1.0, residual: Optional[torch.Tensor] = None, inplace: bool = False):
    """act(alpha * x @ weight.T + bias), or alpha * x @ weight.T + bias + residual, as ONE GEMM with a fused epilogue (act:
    'silu' or 'none'; not an activation together with a residual: the layer never pairs them), for the operands
    the tiled bf16 kernels do not take: fp32 (exact fp32 products on the fp32 matrix cores, pafc_gemm_f32) and bf16 shapes off the
    bf16 kernels' grid (K % 64 or N % 8: through the same kernel in fp32, one rounding at the end).  bias is added as given
    (not scaled by alpha).  inplace: write the result over ``residual``.

    Until round 6 this was a hipBLASLt plan per problem, falling back to the framework's F.linear where the library offered no
    workspace-free kernel.  Both are gone from the inference paths: the framework's fp32 GEMM stalls when two HIP streams issue
    it at once (DESIGN.md section 4 "the c2 stall"), and decode batches are issued two or three streams deep."""
    _lib.require_gpu(x, weight, bias, residual)
    N, K = weight.shape
    rows = x.numel() // K
    if x.shape[-1] != K or weight.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise _lib.PafcError("linear_bias_act: shape/dtype mismatch")
    if residual is not None and (residual.dtype != x.dtype or residual.numel() != rows * N):
        raise _lib.PafcError("linear_bias_act: residual must be (rows, N) in the activation dtype")
    if act not in ("silu", "none"):
        raise _lib.PafcError("linear_bias_act: act is 'silu' or 'none'")
    if act != "none" and residual is not None:
        # pafc_gemm_f32 applies the activation after the residual add, the bf16 kernels before it
        raise _lib.PafcError("linear_bias_act: an activation with a residual (the layer never pairs them)")
    x2 = x.reshape(rows, K)
    r2 = residual.reshape(rows, N) if residual is not None else None
    if x.dtype == torch.float32 and gemm_f32_ok(x2, weight):
        out = gemm_f32(x2, weight, bias, act, alpha=alpha, residual=r2, out=r2 if (inplace and r2 is not None) else None)
        return residual if (inplace and residual is not None) else out.view(x.shape[:-1] + (N,))
    if x.dtype == torch.bfloat16 and K % 4 == 0:
        y = gemm_f32(x2.float(), weight.float(), None if bias is None else bias.float(), act, alpha=alpha,
                     residual=None if r2 is None else r2.float())
        if inplace and residual is not None:
            r2.copy_(y)
            return residual
        return y.to(torch.bfloat16).view(x.shape[:-1] + (N,))
    # K not a multiple of 4 (no layer of this package has one): the framework's operators, still on the GPU
    y = torch.nn.functional.linear(x, weight)
    if alpha != 1.0:
        y = y * alpha
    if bias is not None:
        y = y + bias
    if residual is not None:
        y = y + residual.view(y.shape)
    if act == "silu":
        y = torch.nn.functional.silu(y)
    if residual is not None and inplace:
        residual.view(y.shape).copy_(y)
        return residual
    return y


# fp32 GEMMs of long inputs run on the bf16 matrix cores with split operands (csrc/gemm_ph.hip: three bf16 products per fp32
# product, fp32 accumulation, ~2^-16 relative); shorter ones take exact fp32 products on the fp32 matrix cores (gemm_f32).
_SPLIT_GEMM_MIN_ROWS = DISPATCH["split_gemm_min_rows"]
_split_weights = {}      # id(weight) -> (stamp, [hi | hi | lo] planes, weakref to the weight); bounded

# Derived copies of parameters (stacked / transposed / split / LayerNorm-folded weights of the inference plans) are keyed on
# (storage, Tensor._version).  Fused optimizers (`torch.optim.Adam(fused=True)`, `p.data` writes) update parameters WITHOUT
# touching `_version`, so the keys carry this process-wide epoch as well: it is bumped after every optimizer step of
# utils.train_utils.train_step and whenever an encoder switches between train() and eval() -- a CV pass between training
# steps therefore never multiplies stale weights.  Code that updates parameters behind torch's back calls it itself.
_param_epoch = 0


def param_epoch() -> int:
    return _param_epoch


def bump_param_epoch() -> None:
    global _param_epoch
    _param_epoch += 1


class DerivedFill:
    """Which stream issued the kernels that FILL a set of derived tensors (a plan's stacked / split / folded weights).  The fill
    is asynchronous: a forward pass on ANOTHER stream (utils.longform runs decode batches on side streams that only wait for the
    caller's stream) must wait for it before its kernels read the tensors.  `DerivedFill()` right after the fill records an event
    on the filling stream; `use()` at the top of every consumer makes the current stream wait for that event the first time it
    meets the fill (one dictionary look-up afterwards).  Under graph capture nothing is waited for: an eager pass on the same
    stream always precedes a capture (the graph caches capture a shape's SECOND sighting)."""
    __slots__ = ("event", "seen")

    def __init__(self, device=None):
        self.event, self.seen = None, set()
        if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            st = torch.cuda.current_stream(device)
            self.event = torch.cuda.Event()
            self.event.record(st)
            self.seen.add(st.cuda_stream)

    # an event belongs to the process and stream that recorded it: a copy (copy.deepcopy of a model for EMA / averaging,
    # pickling for spawn / torch.save) starts empty -- its tensors are copies that nobody is still filling
    def __deepcopy__(self, memo):
        return _empty_fill()

    def __reduce__(self):
        return (_empty_fill, ())

    def use(self, device=None) -> None:
        if self.event is None:
            return
        raw = _lib._raw_stream(device.index if device is not None and device.index is not None else torch.cuda.current_device()) \
            if _lib._raw_stream is not None else torch.cuda.current_stream(device).cuda_stream
        if raw in self.seen or torch.cuda.is_current_stream_capturing():
            return
        torch.cuda.current_stream(device).wait_event(self.event)
        self.seen.add(raw)



def _empty_fill() -> DerivedFill:
    f = DerivedFill.__new__(DerivedFill)
    f.event, f.seen = None, set()
    return f


def split_weight_cached(weight: torch.Tensor) -> torch.Tensor:
    """[hi | hi | lo] planes of a weight, cached per weight OBJECT: an entry is valid only for the very tensor it was made
    from (a weak reference is compared by identity -- a freed tensor's id and allocator block can both come back for a new
    tensor of the same shape, whose `_version` is 0 again) and for its stamp (storage, in-place version, shape)."""
    import weakref
    stamp = (weight.data_ptr(), weight._version, tuple(weight.shape), _param_epoch)
    ent = _split_weights.get(id(weight))
    if ent is None or ent[0] != stamp or ent[2]() is not weight:
        if len(_split_weights) > 64:
            _split_weights.clear()
        planes = split_planes(weight.detach().contiguous(), triple=True)
        ent = _split_weights[id(weight)] = (stamp, planes, weakref.ref(weight), DerivedFill(weight.device))
    else:
        ent[3].use(weight.device)            # filled on another stream: that fill first
    return ent[1]


def split_gemm_takes(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> bool:
    """The one rule for sending an fp32 projection x @ weight.T to the split-operand GEMM (gemm_ph_ex(a_split=True), ~2^-16 per
    product) instead of exact fp32 products: inference, a long input (DISPATCH["split_gemm_min_rows"] rows) and dims the kernel
    takes.  The caller adds its own conditions (its split_ok switch, the epilogue: no activation into an fp32 output)."""
    N, K = weight.shape
    return (x.dtype == torch.float32 and weight.dtype == torch.float32 and x.is_cuda and K % 128 == 0 and N % 8 == 0 and N >= 256
            and x.numel() // K >= _SPLIT_GEMM_MIN_ROWS and not torch.is_grad_enabled()
            and (bias is None or bias.dtype == torch.float32))


def linear_fused(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "none",
                 split_ok: bool = True) -> torch.Tensor:
    """act(x @ weight.T + bias) with the epilogue fused: bf16 operands on the hand-written GEMM (K % 64 == 0, N % 8 == 0),
    long fp32 inputs on the same kernel with split operands (unless split_ok is False: a pure-fp32 model's exact products),
    anything else through linear_bias_act (the hand-written fp32 GEMM)."""
    N, K = weight.shape
    rows = x.numel() // K
    if (x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and x.is_cuda and weight.is_contiguous()
            and skinny_ok(rows, N, K) and act != "glu"):         # a streaming chunk: the few-rows kernel
        return gemm_skinny(x.reshape(-1, K), weight, bias, act).view(x.shape[:-1] + (N,))
    if x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and K % 64 == 0 and N % 8 == 0:
        return gemm_bf16(x.reshape(-1, K), weight, bias, act).view(x.shape[:-1] + (N,))
    if split_ok and act == "none" and split_gemm_takes(x, weight, bias):
        planes = split_planes(x.reshape(rows, K) if x.is_contiguous() else x.reshape(rows, K).contiguous())
        return gemm_ph_ex(planes, split_weight_cached(weight), bias, a_split=True, out_kind="f32").view(x.shape[:-1] + (N,))
    return linear_bias_act(x, weight, bias, act)


def tmix_lora_mix4(x: torch.Tensor, t: torch.Tensor, w2t: torch.Tensor, maa: torch.Tensor, reverse0: bool = False,
                   prev: Optional[torch.Tensor] = None):
    """bf16: x (B,T,C), t (ndir,B*T,128) = tanh(xxx W1), w2t (ndir,4,C,32), maa (ndir,4,C) -> z (4,ndir,B*T,C).
    prev: the frame before the chunk (streaming), or None."""
    _lib.require_gpu(x, t, w2t, maa, prev)
    _check_prev(prev, x)
    B, T, C = x.shape
    ndir = t.shape[0]
    if x.dtype != torch.bfloat16 or t.shape != (ndir, B * T, 128) or w2t.shape != (ndir, 4, C, 32):
        raise _lib.PafcError("tmix_lora_mix4: bf16 only, t (ndir, B*T, 128), w2t (ndir, 4, C, 32)")
    z = torch.empty((4, ndir, B * T, C), dtype=x.dtype, device=x.device)
    rc = _lib.lib().pafc_tmix_lora_mix4_bf16_prev(B, T, C, ndir, int(reverse0), _lib.ptr(x), _lib.ptr(t), _lib.ptr(w2t),
                                                  _lib.ptr(maa), _lib.ptr(prev), _lib.ptr(z), _lib.stream_of(x))
    _lib.check(rc, "pafc_tmix_lora_mix4_bf16")
    return z


# The one-pass LoRA kernels stage 128 KiB of weights into LDS per block: worth it from a couple of thousand rows on (30-minute
# file: 45 k rows, a c2 batch: ~16 k) and, as ONE launch instead of two or three, in the launch-bound streaming chunk step
# (`one_pass=True`, fused.layer_forward_carry); below it the small-GEMM path (DISPATCH table at the top of this file).
_LDS_RESIDENT_MIN_ROWS = DISPATCH["lds_resident_min_rows"]


def tmix_lora_down(x: torch.Tensor, maa_x: torch.Tensor, w1n: torch.Tensor, reverse0: bool = False,
                   prev: Optional[torch.Tensor] = None, one_pass: Optional[bool] = None):
    """bf16: t = tanh((x + (x_nb - x) * maa_x) w1n^T) in one pass.  x (B, T, C), maa_x (ndir, C), w1n (ndir, N, C) ->
    (ndir, B*T, N).  C = 512, N = 128 run the fused kernel (weights resident in LDS); other sizes take the shift/lerp pass and
    a GEMM with the same roundings."""
    _lib.require_gpu(x, maa_x, w1n, prev)
    _check_prev(prev, x)
    L = _lib.lib()
    B, T, C = x.shape
    ndir, N = w1n.shape[0], w1n.shape[1]
    if x.dtype != torch.bfloat16 or w1n.shape != (ndir, N, C) or maa_x.shape != (ndir, C):
        raise _lib.PafcError("tmix_lora_down: bf16 only, maa_x (ndir, C), w1n (ndir, N, C)")
    for a in (x, maa_x, w1n):
        if not a.is_contiguous() or a.dtype != torch.bfloat16:
            raise _lib.PafcError("tmix_lora_down: contiguous bf16 tensors")
    if C == 512 and N == 128 and (B * T >= _LDS_RESIDENT_MIN_ROWS if one_pass is None else one_pass):
        t = torch.empty((ndir, B * T, N), dtype=x.dtype, device=x.device)
        from .profiling import op_timer
        with op_timer("tmix_lora_down"):
            rc = L.pafc_tmix_lora_down_bf16_prev(B, T, C, N, ndir, int(reverse0), _lib.ptr(x), _lib.ptr(maa_x), _lib.ptr(w1n),
                                                 _lib.ptr(prev), _lib.ptr(t), _lib.stream_of(x))
        _lib.check(rc, "pafc_tmix_lora_down_bf16")
        return t
    xxx = tmix_shift_mix(x, maa_x[0], maa_x[1] if ndir == 2 else None, reverse0=reverse0, prev=prev)
    return gemm_bf16(xxx.view(ndir, B * T, C), w1n, act="tanh")


def decay_lora_one_pass(rows: int, C: int, H: int) -> bool:
    """Does decay_lora take its one-pass kernel (where a bias costs nothing) at this size?"""
    return C == 512 and H == 64 and rows >= _LDS_RESIDENT_MIN_ROWS


def decay_lora(zw: torch.Tensor, d1n: torch.Tensor, d2n: torch.Tensor, bias: Optional[torch.Tensor] = None,
               one_pass: Optional[bool] = None):
    """bf16: w = bf16(bf16(tanh(zw d1n^T)) d2n^T) [+ bias] in one pass.  zw (ndir, rows, C), d1n (ndir, H, C), d2n (ndir, C, H),
    bias (ndir, C) or None -> (ndir, rows, C).  C = 512, H = 64 run the fused kernel (weights resident in LDS); other sizes
    take two GEMMs with the same roundings."""
    _lib.require_gpu(zw, d1n, d2n, bias)
    L = _lib.lib()
    ndir, rows, C = zw.shape
    H = d1n.shape[1]
    if zw.dtype != torch.bfloat16 or d1n.shape != (ndir, H, C) or d2n.shape != (ndir, C, H) or \
            (bias is not None and bias.numel() != ndir * C):
        raise _lib.PafcError("decay_lora: bf16 only, zw (ndir, rows, C), d1n (ndir, H, C), d2n (ndir, C, H), bias (ndir, C)")
    for a in (zw, d1n, d2n) + ((bias,) if bias is not None else ()):
        if not a.is_contiguous() or a.dtype != torch.bfloat16:
            raise _lib.PafcError("decay_lora: contiguous bf16 tensors")
    if C == 512 and H == 64 and (decay_lora_one_pass(rows, C, H) if one_pass is None else one_pass):
        w = torch.empty_like(zw)
        from .profiling import op_timer
        with op_timer("decay_lora"):
            rc = L.pafc_decay_lora_bf16(rows, C, H, ndir, _lib.ptr(zw), _lib.ptr(d1n), _lib.ptr(d2n), _lib.ptr(bias),
                                        _lib.ptr(w), _lib.stream_of(zw))
        _lib.check(rc, "pafc_decay_lora_bf16")
        return w
    w = gemm_bf16(gemm_bf16(zw, d1n, act="tanh"), d2n)
    return w if bias is None else w + bias.view(ndir, 1, C)


def conv3x3s2_nhwc(x: torch.Tensor, w_tap_co_ci: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = True):
    """x (B, T1, F1, Ci) bf16 NHWC, w (9, Co, Ci) -> (B, T2, F2, Co) = relu(conv3x3 stride 2 + bias)."""
    _lib.require_gpu(x, w_tap_co_ci, bias)
    L = _lib.lib()
    B, T1, F1, Ci = x.shape
    Co = w_tap_co_ci.shape[1]
    if x.dtype != torch.bfloat16 or w_tap_co_ci.shape != (9, Co, Ci) or w_tap_co_ci.dtype != x.dtype:
        raise _lib.PafcError("conv3x3s2_nhwc: bf16 NHWC input and a (9, Co, Ci) weight")
    out = torch.empty((B, (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1, Co), dtype=x.dtype, device=x.device)
    from .profiling import op_timer
    with op_timer("conv3x3s2", flops=2.0 * out.numel() * 9 * Ci):
        rc = L.pafc_conv3x3s2_nhwc_bf16(B, T1, F1, Ci, Co, _lib.ptr(x), _lib.ptr(w_tap_co_ci), _lib.ptr(bias),
                                        _lib.ptr(out), int(relu), _lib.stream_of(x))
    _lib.check(rc, "pafc_conv3x3s2_nhwc_bf16")
    return out


def conv3x3s2_nhwc_ph(x: torch.Tensor, w_tap_co_ci: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = True,
                      tile_m: int = 256):
    """The phase-pipelined implicit GEMM (csrc/gemm_ph.hip) by itself -- same arguments as conv3x3s2_nhwc, which picks it
    for the long-form shapes."""
    _lib.require_gpu(x, w_tap_co_ci, bias)
    L = _lib.lib()
    B, T1, F1, Ci = x.shape
    Co = w_tap_co_ci.shape[1]
    if x.dtype != torch.bfloat16 or w_tap_co_ci.shape != (9, Co, Ci) or w_tap_co_ci.dtype != x.dtype:
        raise _lib.PafcError("conv3x3s2_nhwc_ph: bf16 NHWC input and a (9, Co, Ci) weight")
    out = torch.empty((B, (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1, Co), dtype=x.dtype, device=x.device)
    _lib.check(L.pafc_conv3x3s2_nhwc_bf16_ph(B, T1, F1, Ci, Co, _lib.ptr(x), _lib.ptr(w_tap_co_ci), _lib.ptr(bias), _lib.ptr(out),
                                             int(relu), int(tile_m), _lib.stream_of(x)), "pafc_conv3x3s2_nhwc_bf16_ph")
    return out


def ctc_greedy(scores: torch.Tensor, lens: Optional[torch.Tensor], blank_id: int = 0, want_frames: bool = False):
    """GPU-resident CTC greedy search (include/pafc_search.h): (B, T, V) scores -> (tokens (B, T) int32, ntok (B) int32
    [, first-frame index per token]).  Row b of ``tokens`` holds ``ntok[b]`` collapsed ids."""
    _lib.require_gpu(scores, lens)
    if scores.dim() != 3:
        raise _lib.PafcError("ctc_greedy wants (B, T, V) scores")
    L = _lib.lib()
    B, T, V = scores.shape
    lens64 = None if lens is None else lens.to(torch.int64).contiguous()
    best = torch.empty(B, T, dtype=torch.int32, device=scores.device)
    tokens = torch.empty(B, T, dtype=torch.int32, device=scores.device)
    ntok = torch.empty(B, dtype=torch.int32, device=scores.device)
    frames = torch.empty(B, T, dtype=torch.int32, device=scores.device) if want_frames else None
    _lib.check(L.pafc_ctc_greedy(_lib.dtype_code(scores.dtype), B, T, V, _lib.ptr(scores), _lib.ptr(lens64), int(blank_id),
                                 _lib.ptr(best), _lib.ptr(tokens), _lib.ptr(ntok), _lib.ptr(frames),
                                 _lib.stream_of(scores)), "pafc_ctc_greedy")
    return (tokens, ntok, frames) if want_frames else (tokens, ntok)


def ctc_align(lp: torch.Tensor, hlens: torch.Tensor, ys: torch.Tensor, ylens: torch.Tensor, blank_id: int = 0,
              workspace: Optional[torch.Tensor] = None):
    """GPU-resident CTC forced alignment (include/pafc_search.h: pafc_ctc_align, csrc/ctc_align.hip).  lp (B, T, V) float32 or
    bfloat16 log-probabilities (a view with row stride >= V is taken as it is), hlens (B) frames, ys (B, Lmax) labels, ylens (B)
    label counts -> (align (B, T) int32 [-1 beyond hlens], first (B, Lmax) int32, last (B, Lmax) int32 [-1 beyond ylens],
    score (B) float32, ok (B) int32).  One launch, no host read: the call can be captured or its results fetched later.
    workspace: a uint8 tensor of at least pafc_ctc_align_workspace_bytes(B, T, Lmax) bytes that the caller owns and keeps to
    itself until the call has run (tools/bench_ctc_align.py reads the kernel's stamps from it); by default the call makes its own."""
    for t in (lp, hlens, ys, ylens):
        if not t.is_cuda:
            raise _lib.PafcError("this op runs on the MI355X only (tensor is on %s); there is no CPU fallback" % t.device)
    if lp.dim() != 3 or ys.dim() != 2 or ys.shape[0] != lp.shape[0] or hlens.numel() != lp.shape[0] or ylens.numel() != lp.shape[0]:
        raise _lib.PafcError("ctc_align wants lp (B, T, V), hlens (B), ys (B, Lmax), ylens (B)")
    B, T, V = lp.shape
    if lp.stride(2) != 1 or lp.stride(1) < V or lp.stride(0) != T * lp.stride(1):
        lp = lp.contiguous()
    L = _lib.lib()
    dev, Lmax = lp.device, ys.shape[1]
    h32, y64, l32 = hlens.to(torch.int32).contiguous(), ys.to(torch.int64).contiguous(), ylens.to(torch.int32).contiguous()
    align = torch.empty(B, T, dtype=torch.int32, device=dev)
    first = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    last = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    ok = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0 or T == 0:
        return align, first, last, score, ok
    nws = L.pafc_ctc_align_workspace_bytes(B, T, Lmax)
    # the workspace is the call's own: the caching allocator hands a block of this size back to the next call on the stream,
    # and inside a capture the block belongs to the graph's pool, so a replay never writes into memory another tensor owns
    if workspace is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    else:
        ws = workspace
        if not ws.is_cuda or ws.device != dev or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < nws:
            raise _lib.PafcError("ctc_align: workspace must be a contiguous uint8 tensor of >= %d bytes on %s" % (nws, dev))
    _lib.check(L.pafc_ctc_align(_lib.dtype_code(lp.dtype), B, T, V, _lib.ptr(lp), lp.stride(1), _lib.ptr(h32), _lib.ptr(y64), Lmax,
                                _lib.ptr(l32), int(blank_id), _lib.ptr(ws), nws, _lib.ptr(align), _lib.ptr(first), _lib.ptr(last),
                                Lmax, _lib.ptr(score), _lib.ptr(ok), _lib.stream_of(lp)), "pafc_ctc_align")
    return align, first, last, score, ok


_ACTS = {"none": 0, "silu": 1, "tanh": 2, "relu": 3, "glu": 4}


def gemm_bf16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
              alpha: float = 1.0, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """Hand-written bf16 GEMM with fused epilogue (include/pafc_encoder_ops.h: pafc_gemm_bf16).
    a: (M, K) or (Z, M, K); w: (N, K) or (Z, N, K) in nn.Linear layout; bias: (N) or (Z, N); residual / out:
    (M, N) or (Z, M, N), ``out`` may be ``residual``.  Rows may be strided views (unit stride in the last dim).
    act "glu": w / bias rows come in blocks of 128 = 64 value rows + the 64 gate rows of the same channels
    (``glu_interleave``); out is (M, N / 2)."""
    Z, M, N, K, out, args = _gemm_operands("gemm_bf16", torch.bfloat16, a, w, bias, residual, out, act)
    from .profiling import op_timer
    with op_timer("gemm_%dx%d%s" % (K, N, "x%d" % Z if a.dim() == 3 else ""), sample=12, flops=2.0 * Z * M * N * K):
        rc = _lib.lib().pafc_gemm_bf16(*args, float(alpha), _ACTS[act], _lib.stream_of(a))
    _lib.check(rc, "pafc_gemm_bf16")
    return out


SKINNY_MAX_ROWS = DISPATCH["skinny_max_rows"]      # (the table at the top of this file)


_chunk_step = threading.local()


@contextlib.contextmanager
def chunk_step():
    """Inside: the caller is a streaming chunk step (encoder.forward_chunk_carry) -- its few-row projections run on
    csrc/gemm_skinny.hip.  Outside (offline inputs that merely happen to be short) they keep the kernels the goldens of the
    offline path were recorded with."""
    prev = getattr(_chunk_step, "on", False)
    _chunk_step.on = True
    try:
        yield
    finally:
        _chunk_step.on = prev


def skinny_ok(rows: int, N: int, K: int, glu: bool = False) -> bool:
    """Shapes csrc/gemm_skinny.hip takes, asked from inside a streaming chunk step."""
    return (getattr(_chunk_step, "on", False) and 0 < rows <= SKINNY_MAX_ROWS and K % 32 == 0
            and N % (32 if glu else 16) == 0)


def decay_lora_skinny(x: torch.Tensor, d1n: torch.Tensor, d2n: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decay LoRA for a handful of rows in one launch: bf16(bf16(tanh(x d1n^T)) d2n^T) [+ bias, rounded again] -- bit-identical
    to gemm_skinny(gemm_skinny(x, d1n, None, "tanh"), d2n, bias, round_first=True) (include/pafc_encoder_ops.h:
    pafc_decay_lora_skinny_bf16).  x (M, C) bf16 rows (unit column stride), d1n (64, C), d2n (C, 64), bias (C) -> (M, C)."""
    _lib.require_gpu(x, d1n, d2n, bias)
    M, C = x.shape
    H = d1n.shape[0]
    if x.dtype != torch.bfloat16 or x.stride(1) != 1 or d1n.shape != (H, C) or d2n.shape != (C, H) or \
            not (d1n.is_contiguous() and d2n.is_contiguous()) or (bias is not None and (bias.numel() != C or not bias.is_contiguous())):
        raise _lib.PafcError("decay_lora_skinny: x (M, C) bf16 rows, d1n (H, C), d2n (C, H), bias (C), contiguous weights")
    L = _lib.lib()
    out = torch.empty((M, C), dtype=x.dtype, device=x.device)
    rc = L.pafc_decay_lora_skinny_bf16(M, C, H, _lib.ptr(x), x.stride(0), _lib.ptr(d1n), _lib.ptr(d2n), _lib.ptr(bias), _lib.ptr(out), C,
                                       _lib.stream_of(x))
    _lib.check(rc, "pafc_decay_lora_skinny_bf16")
    return out


def gemm_skinny(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none", alpha: float = 1.0,
                residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, ln_stats: Optional[torch.Tensor] = None,
                ln_csum: Optional[torch.Tensor] = None, ln_eps: float = 1e-5, stats_out: Optional[torch.Tensor] = None,
                ln_self: bool = False, round_first: bool = False, mix_maa: Optional[torch.Tensor] = None,
                mix_prev: Optional[torch.Tensor] = None, mix_T: int = 0, norm_silu: Optional[tuple] = None):
    """The few-rows bf16 GEMM of the streaming chunk step (include/pafc_encoder_ops.h: pafc_gemm_skinny_bf16[_ex]), arguments as
    gemm_bf16 except act "glu": w is the module's own (2C, K) weight (value rows, then gate rows), out (M, C).
    ln_csum (N) fp32 with ln_stats (M, P, 2) fp32 or ln_self: the LayerNorm in front of the projection folded in (a = the
    UN-normalised rows, w / bias = the folded ones; statistics from a producer's partials or formed in the launch);
    stats_out (M, N_out / 16, 2) fp32 receives the partial row statistics of the result; round_first: bf16(alpha a w^T) + bias;
    mix_maa (K) [+ mix_prev (B, K)], mix_T: a = x of B sequences of mix_T rows, the operand is x + (x_prev - x) * maa;
    norm_silu = (gamma (K), beta (K), eps): the operand is silu(LayerNorm(a)), each rounded to bf16."""
    ng, nb, neps = norm_silu if norm_silu is not None else (None, None, 0.0)
    _lib.require_gpu(ln_stats, ln_csum, stats_out, mix_maa, mix_prev, ng, nb)
    Z, M, N, K, out, args = _gemm_operands("gemm_skinny", torch.bfloat16, a, w, bias, residual, out, act)
    batched = a.dim() == 3
    parts = 0
    if ln_stats is not None or ln_self:
        if ln_csum is None or batched or ln_csum.dtype != torch.float32 or ln_csum.numel() != N or (ln_stats is not None and ln_self):
            raise _lib.PafcError("gemm_skinny: a folded LayerNorm wants ln_csum (N) fp32 and ln_stats or ln_self, unbatched")
        if ln_stats is not None:
            if ln_stats.dtype != torch.float32 or ln_stats.dim() != 3 or ln_stats.shape[0] != M or ln_stats.shape[2] != 2:
                raise _lib.PafcError("gemm_skinny: ln_stats (M, P, 2) fp32")
            parts = ln_stats.shape[1]
    elif ln_csum is not None:
        raise _lib.PafcError("gemm_skinny: ln_csum without ln_stats / ln_self")
    if stats_out is not None and (stats_out.dtype != torch.float32 or stats_out.numel() != Z * M * (out.shape[-1] // 16) * 2):
        raise _lib.PafcError("gemm_skinny: stats_out must be fp32 (M, N_out / 16, 2) per batch entry")
    if mix_maa is not None:
        if (batched or mix_T <= 0 or M % mix_T or mix_maa.dtype != a.dtype or mix_maa.numel() != K or not a.is_contiguous()
                or (mix_prev is not None and (mix_prev.dtype != a.dtype or mix_prev.numel() != (M // mix_T) * K))):
            raise _lib.PafcError("gemm_skinny: mix wants contiguous a = (B * T, K), maa (K) and prev (B, K) of a's dtype")
    elif mix_prev is not None:
        raise _lib.PafcError("gemm_skinny: mix_prev without mix_maa")
    if ng is not None and (batched or ng.dtype != a.dtype or nb.dtype != a.dtype or ng.numel() != K or nb.numel() != K):
        raise _lib.PafcError("gemm_skinny: norm_silu wants gamma, beta (K) of a's dtype, unbatched")
    rc = _lib.lib().pafc_gemm_skinny_bf16_ex(*args, float(alpha), _ACTS[act], int(round_first), _lib.ptr(ln_stats), parts,
                                             int(ln_self), _lib.ptr(ln_csum), float(ln_eps), _lib.ptr(stats_out), _lib.ptr(mix_maa),
                                             _lib.ptr(mix_prev), int(mix_T), _lib.ptr(ng), _lib.ptr(nb), float(neps), _lib.stream_of(a))
    _lib.check(rc, "pafc_gemm_skinny_bf16")
    return out


def gemm_bf16_ph(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
                 alpha: float = 1.0, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 tile_n: int = 256, tile_m: int = 256):
    """The phase-pipelined tile_m x tile_n kernel (csrc/gemm_ph.hip) by itself -- same arguments as gemm_bf16, which picks
    it for the long-form shapes; act "glu" wants glu_interleave(w, tile_n // 8)."""
    _, _, _, _, out, args = _gemm_operands("gemm_bf16_ph", torch.bfloat16, a, w, bias, residual, out, act)
    rc = _lib.lib().pafc_gemm_bf16_ph(*args, float(alpha), _ACTS[act], int(tile_n), int(tile_m), _lib.stream_of(a))
    _lib.check(rc, "pafc_gemm_bf16_ph")
    return out


def gemm_glu_half(M: int, N: int, K: int, batch: int = 1) -> int:
    """Row-block half size (64 or 32) pafc_gemm_bf16 wants for act "glu" on this problem (it depends on the kernel chosen)."""
    return int(_lib.lib().pafc_gemm_bf16_glu_half(M, N, K, batch))


def log_softmax_rows(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """log_softmax over the last dimension in one pass over HBM (include/pafc_search.h: pafc_log_softmax_rows)."""
    _lib.require_gpu(x)
    L = _lib.lib()
    V = x.shape[-1]
    out = x if inplace else torch.empty_like(x)
    _lib.check(L.pafc_log_softmax_rows(_lib.dtype_code(x.dtype), x.numel() // V, V, _lib.ptr(x), _lib.ptr(out),
                                       _lib.stream_of(x)), "pafc_log_softmax_rows")
    return out


def glu_interleave(t: torch.Tensor, half: int = 64) -> torch.Tensor:
    """(2C, ...) parameter of a Linear followed by F.glu (values = rows [0, C), gates = rows [C, 2C)) -> the row order
    the GEMM kernels want for act "glu": blocks of `half` value rows followed by the `half` gate rows of the same channels
    (half = 64: pafc_gemm_bf16's 128 x 128 kernel; 32 / 16: the phase-pipelined kernel at tile_n 256 / 128, where a wave's
    columns are one block)."""
    C = t.shape[0] // 2
    if C % half:
        raise _lib.PafcError(f"glu_interleave: channels must be a multiple of {half}")
    v = t[:C].reshape(C // half, half, *t.shape[1:])
    g = t[C:].reshape(C // half, half, *t.shape[1:])
    return torch.cat([v, g], dim=1).reshape(t.shape).contiguous()


def conv3x3s2_c1_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = True):
    """First subsampling convolution (1 input channel): x (B, T, F) bf16, weight (C, 1, 3, 3) -> (B, T1, F1, C)."""
    _lib.require_gpu(x, weight, bias)
    if x.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16 or x.dim() != 3 or weight.shape[1:] != (1, 3, 3):
        raise _lib.PafcError("conv3x3s2_c1_nhwc: bf16 x (B, T, F) and weight (C, 1, 3, 3)")
    L = _lib.lib()
    B, T, Fd = x.shape
    C = weight.shape[0]
    out = torch.empty((B, (T - 3) // 2 + 1, (Fd - 3) // 2 + 1, C), dtype=x.dtype, device=x.device)
    _lib.check(L.pafc_conv3x3s2_c1_nhwc_bf16(B, T, Fd, C, _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out),
                                             int(relu), _lib.stream_of(x)), "pafc_conv3x3s2_c1_nhwc_bf16")
    return out


def conv3x3s2_c1_wgrad(x: torch.Tensor, act: torch.Tensor, dact: torch.Tensor) -> torch.Tensor:
    """Weight and bias gradient of relu(Conv2d(1, C, 3, 2)) (pafc_conv3x3s2_c1_wgrad_bf16): x (B, T, F) bf16 features, act
    (B, T1, F1, C) bf16 the forward's ReLU output, dact its incoming gradient.  Returns (10, C) fp32: rows kh * 3 + kw of dW,
    then db; the partial sums are added in a fixed order."""
    B, T, Fd = x.shape
    C = act.shape[-1]
    L = _lib.lib()
    nbytes = L.pafc_conv3x3s2_c1_wgrad_workspace_bytes(B, T, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(10, C, dtype=torch.float32, device=x.device)
    dact = dact.contiguous()
    rc = L.pafc_conv3x3s2_c1_wgrad_bf16(B, T, Fd, C, _lib.ptr(x), _lib.ptr(act), _lib.ptr(dact), _lib.ptr(out), _lib.ptr(ws),
                                        nbytes, _lib.stream_of(x))
    _lib.check(rc, "pafc_conv3x3s2_c1_wgrad_bf16")
    return out


class _Conv1Train(torch.autograd.Function):
    """relu(Conv2d(1, C, 3, 2)(x)) in NHWC for the GPU training step (subsampling.py:201-226, conv[0:2]): forward = the
    inference kernel, backward = pafc_conv3x3s2_c1_wgrad_bf16 (the library runs this layer as im2col + one small GEMM per
    batch entry: 6 ms forward + backward at the c4 shape).  x: (B, T, F) bf16 features (no gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        wb = weight.to(torch.bfloat16)
        a = conv3x3s2_c1_nhwc(x, wb, None if bias is None else bias.to(torch.bfloat16), relu=True)
        ctx.save_for_backward(x, a)
        ctx.w_dtype, ctx.b_dtype, ctx.w_shape = weight.dtype, (None if bias is None else bias.dtype), weight.shape
        return a

    @staticmethod
    def backward(ctx, da):
        x, a = ctx.saved_tensors
        out = conv3x3s2_c1_wgrad(x, a, da)
        dw = out[:9].t().reshape(ctx.w_shape).to(ctx.w_dtype)
        db = out[9].to(ctx.b_dtype) if ctx.b_dtype is not None else None
        return None, dw, db


class _Conv2Train(torch.autograd.Function):
    """relu(Conv2d(C, C, 3, 2)(a)) NHWC -> NHWC for the GPU training step (subsampling.py conv[2:4]): forward = the
    hand-written implicit GEMM (1.0 PFLOP/s; the library's forward runs at a third of that), backward = the library's
    convolution backward on channels_last views of the same memory."""

    @staticmethod
    def forward(ctx, a, weight, bias):
        Co, Ci = weight.shape[0], weight.shape[1]
        wb = weight.to(torch.bfloat16)
        taps = wb.permute(2, 3, 0, 1).reshape(9, Co, Ci).contiguous()
        y = conv3x3s2_nhwc(a, taps, None if bias is None else bias.to(torch.bfloat16), relu=True)
        ctx.save_for_backward(a, y, wb)
        ctx.w_dtype, ctx.b_dtype = weight.dtype, (None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, y, wb = ctx.saved_tensors
        # relu's backward as the framework's own one-pass kernel (`dy * (y > 0)` was a compare, a 150 MB bool tensor and a
        # mixed-dtype multiply: 0.4 ms); NCHW view of NHWC memory (channels_last)
        g = torch.ops.aten.threshold_backward(dy.contiguous(), y, 0.0).permute(0, 3, 1, 2)
        gi, gw, gb = torch.ops.aten.convolution_backward(g, a.permute(0, 3, 1, 2), wb, [wb.shape[0]], [2, 2], [0, 0], [1, 1],
                                                         False, [0, 0], 1, [ctx.needs_input_grad[0], True,
                                                                            ctx.b_dtype is not None])
        da = gi.permute(0, 2, 3, 1).contiguous() if gi is not None else None
        return da, gw.to(ctx.w_dtype), (gb.to(ctx.b_dtype) if gb is not None else None)


def conv_sub_train(x: torch.Tensor, c1_weight, c1_bias, c2_weight, c2_bias) -> torch.Tensor:
    """The two subsampling convolutions + ReLUs of the bf16 training step, NHWC: x (B, T, F) -> (B, T', F', C) bf16."""
    a = _Conv1Train.apply(x.to(torch.bfloat16).contiguous(), c1_weight, c1_bias)
    return _Conv2Train.apply(a, c2_weight, c2_bias)


class _CtxGraph(ctypes.Structure):
    """pafc_ctc_context_graph (include/pafc_search.h)"""
    _fields_ = [("num_nodes", c_int), ("child_begin", c_void_p), ("child_token", c_void_p), ("child_node", c_void_p),
                ("fail", c_void_p), ("token_score", c_void_p), ("node_score", c_void_p), ("output_score", c_void_p)]


def _ctx_graph(g: dict, dev, who: str) -> _CtxGraph:
    """The C struct over ContextGraph.device_tables(dev); the tables must outlive it."""
    for k, dt in (("child_begin", torch.int32), ("child_token", torch.int32), ("child_node", torch.int32),
                  ("fail", torch.int32), ("token_score", torch.float64), ("node_score", torch.float64),
                  ("output_score", torch.float64)):
        if g[k].dtype != dt or g[k].device != dev or not g[k].is_contiguous():
            raise _lib.PafcError(f"{who}: graph table {k} must be contiguous {dt} on {dev}")
    return _CtxGraph(int(g["fail"].numel()), *[_lib.ptr(g[k]) for k in ("child_begin", "child_token", "child_node", "fail",
                                                                        "token_score", "node_score", "output_score")])


def ctc_prefix_beam(top_logp: torch.Tensor, top_idx: torch.Tensor, lens: Optional[torch.Tensor], beam: int,
                    blank_id: int = 0, graph_tables: Optional[dict] = None, want_times: bool = True):
    """GPU-resident CTC prefix beam search (include/pafc_search.h: pafc_ctc_prefix_beam_search_ex).  top_logp (B, T, K)
    float32 / top_idx (B, T, K) = torch.topk of the CTC log-probs.  graph_tables: ContextGraph.device_tables(device) for
    context biasing, or None.  Returns (tokens (B, beam, T) int32, lengths (B, beam) int32 [-1 = unused],
    scores (B, beam) float64, times (B, beam, T) int32 [frames of each prefix's tokens, then -1] or None), best first."""
    _lib.require_gpu(top_logp, top_idx, lens)
    L = _lib.lib()
    if top_logp.dtype != torch.float32 or top_logp.shape != top_idx.shape or top_logp.dim() != 3:
        raise _lib.PafcError("ctc_prefix_beam: top_logp float32 (B, T, K) and top_idx of the same shape")
    B, T, K = top_logp.shape
    idx32 = top_idx.to(torch.int32).contiguous()
    lens64 = None if lens is None else lens.to(torch.int64).contiguous()
    dev = top_logp.device
    graph = None if graph_tables is None else _ctx_graph(graph_tables, dev, "ctc_prefix_beam")
    nws = L.pafc_ctc_prefix_beam_ex_workspace_bytes(B, T, beam)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
    tokens = torch.empty(B, beam, T, dtype=torch.int32, device=dev)
    lengths = torch.empty(B, beam, dtype=torch.int32, device=dev)
    scores = torch.empty(B, beam, dtype=torch.float64, device=dev)
    times = torch.empty(B, beam, T, dtype=torch.int32, device=dev) if want_times else None
    _lib.check(L.pafc_ctc_prefix_beam_search_ex(B, T, K, _lib.ptr(top_logp), _lib.ptr(idx32), _lib.ptr(lens64),
                                                int(beam), int(blank_id),
                                                None if graph is None else ctypes.addressof(graph),
                                                _lib.ptr(tokens), _lib.ptr(lengths), _lib.ptr(scores), _lib.ptr(times),
                                                _lib.ptr(ws), nws, _lib.stream_of(top_logp)),
               "pafc_ctc_prefix_beam_search_ex")
    return tokens, lengths, scores, times


class CtcBeamStream(_RowStream):
    """CTC prefix beam search of B streams chunk by chunk (include/pafc_search.h: pafc_ctc_beam_stream_*,
    csrc/ctc_beam_stream.hip): the beam of every stream lives in the workspace between feeds, and the n-best lists over a
    stream equal ctc_prefix_beam on the concatenated frames bit for bit.  The object owns the workspace, the fixed
    (B, Tmax, K) top-k buffers, the frame counts and the `from` offsets.

    feed(top_logp (B, n <= Tmax, K), top_idx, nframes=None) copies the chunk into the fixed buffers and launches the feed
    kernel; launch_feed() is that launch alone, on whatever the buffers hold -- nothing but the package's kernel, so it
    can be captured in a graph.  drain(counts, ld) returns host lists: the one read of a feed.  A row that would pass
    max_total_frames consumes nothing and is reported by drain's `overflow`; reset(rows) starts rows again."""

    def __init__(self, B: int, Tmax: int, K: int, beam: int, device, blank_id: int = 0, graph_tables: Optional[dict] = None,
                 max_total_frames: int = 4096, want_times: bool = True):
        dev = self._device(device)
        if B < 1 or Tmax < 1 or max_total_frames < 1:
            raise _lib.PafcError(f"CtcBeamStream: B {B}, Tmax {Tmax}, max_total_frames {max_total_frames} must be >= 1")
        if not 1 <= beam <= 16 or not 1 <= K <= 16:
            raise _lib.PafcError(f"CtcBeamStream: beam {beam} and K {K} must be in 1 .. 16")
        self.Tmax, self.K, self.beam, self.blank = Tmax, K, beam, int(blank_id)
        self.max_total, self.times = int(max_total_frames), int(bool(want_times))
        self._tables = graph_tables
        self._graph = None if graph_tables is None else _ctx_graph(graph_tables, dev, "CtcBeamStream")
        self._pgraph = None if self._graph is None else ctypes.addressof(self._graph)
        self._init_rows(B, dev, "pafc_ctc_beam_stream_workspace_bytes", (B, self.max_total, beam, self.times),
                        "unsupported dimensions (max_total_frames * beam < 2^31)")
        self._init_drain()
        self._top_p = torch.zeros(B, Tmax, K, dtype=torch.float32, device=dev)
        self._top_i = torch.zeros(B, Tmax, K, dtype=torch.int32, device=dev)
        self.reset()

    def reset(self, rows=None):
        """Restart the given rows (all when None) from the empty prefix at frame 0; other rows are untouched."""
        _lib.check(self._L.pafc_ctc_beam_stream_reset(self.B, self.max_total, self.beam, self.times, self._row_mask(rows),
                                                       _lib.ptr(self._ws), self._nbytes, _lib.stream_of(self._ws)),
                   "pafc_ctc_beam_stream_reset")

    def launch_feed(self):
        """The feed kernel on the fixed buffers (top-k, frame counts): reads nothing from the host, allocates nothing."""
        _lib.check(self._L.pafc_ctc_beam_stream_feed(self.B, self.Tmax, self.K, _lib.ptr(self._top_p), _lib.ptr(self._top_i),
                                                      _lib.ptr(self._nf), self.max_total, self.beam, self.blank, self._pgraph,
                                                      self.times, _lib.ptr(self._ws), self._nbytes, _lib.stream_of(self._ws)),
                   "pafc_ctc_beam_stream_feed")

    def load(self, top_logp: torch.Tensor, top_idx: torch.Tensor, nframes=None):
        """Copy a chunk's top-k (B, n <= Tmax, K) and its frame counts (default n for every row) into the fixed buffers."""
        B, Tmax, K = self.B, self.Tmax, self.K
        if top_logp.dim() != 3 or top_logp.shape != top_idx.shape or top_logp.shape[0] != B or top_logp.shape[2] != K:
            raise _lib.PafcError(f"CtcBeamStream.feed: top_logp and top_idx must be ({B}, n, {K})")
        n = top_logp.shape[1]
        if n > Tmax:
            raise _lib.PafcError(f"CtcBeamStream.feed: {n} frames, at most Tmax = {Tmax}")
        if top_logp.device != self.device or top_idx.device != self.device or top_logp.dtype != torch.float32:
            raise _lib.PafcError(f"CtcBeamStream.feed: top_logp float32 and top_idx on {self.device}")
        if n:
            self._top_p[:, :n].copy_(top_logp)
            self._top_i[:, :n].copy_(top_idx)
        self._set_nframes(nframes, n)

    def feed(self, top_logp: torch.Tensor, top_idx: torch.Tensor, nframes=None):
        self.load(top_logp, top_idx, nframes)
        self.launch_feed()

    def drain(self, counts=None, ld: int = 1, want_times: bool = False):
        """The n-best of every row as if its stream ended here.  counts: per row the tokens the caller already holds as
        final (an earlier drain's `committed`), default 0.  Returns a dict of host lists: count (B), committed (B),
        overflow (B), len (B, beam: total token counts, -1 unused), score (B, beam), tokens (B, beam: the tokens from
        counts[b] on, at most ld of them) and, with want_times, times (B, beam: the whole frame list)."""
        B, beam = self.B, self.beam
        if want_times and not self.times:
            raise _lib.PafcError("CtcBeamStream.drain: the stream was made with want_times=False")
        ntim = tim = None

        def call(out, ld):
            nonlocal ntim, tim
            ldt = 0
            if want_times:           # the frame lists' lengths first: they size the second call's copy
                ntim = torch.empty(B, beam, dtype=torch.int32, device=self.device)
                self._drain(out, ld, 0, None, ntim)
                ldt = max(1, int(ntim.max()))
                tim = torch.empty(B, beam, ldt, dtype=torch.int32, device=self.device)
            self._drain(out, ld, ldt, tim, ntim)

        res = self._drain_nbest(call, counts, ld)
        if want_times:
            nt_h, tm_h = ntim.tolist(), tim.tolist()
            res["times"] = [[tm_h[b][n][:nt_h[b][n]] for n in range(beam)] for b in range(B)]
        return res

    def _drain(self, out, ld, ldt, tim, ntim):
        _lib.check(self._L.pafc_ctc_beam_stream_drain(self.B, self.max_total, self.beam, self._pgraph, self.times,
                                                       _lib.ptr(self._ws), self._nbytes, _lib.ptr(self._from), ld,
                                                       out.ptr("tokens"), out.ptr("len"), out.ptr("score"), out.ptr("count"),
                                                       out.ptr("committed"), out.ptr("overflow"), ldt, _lib.ptr(tim),
                                                       _lib.ptr(ntim), _lib.stream_of(self._ws)), "pafc_ctc_beam_stream_drain")


class CtcGreedyStream(_RowStream):
    """CTC greedy search of B streams chunk by chunk (pafc_ctc_greedy_stream, csrc/ctc_greedy.hip): the offline argmax
    kernel on the chunk and a collapse that carries the previous frame's argmax and the frame base per row, so the tokens
    and absolute frames over a stream equal ctc_greedy(want_frames=True) on the concatenated frames."""

    def __init__(self, B: int, Tmax: int, device, blank_id: int = 0):
        dev = self._device(device)
        if B < 1 or Tmax < 1:
            raise _lib.PafcError(f"CtcGreedyStream: B {B} and Tmax {Tmax} must be >= 1")
        self.Tmax, self.blank = Tmax, int(blank_id)
        self._init_rows(B, dev, "pafc_ctc_greedy_stream_workspace_bytes", (B,))
        self._best = torch.empty(B, Tmax, dtype=torch.int32, device=dev)
        # (a feed of n frames uses rows of n: the chunk's own frame count is the row stride)
        self._out = _Packed([("frames", torch.int64, (B * Tmax,)), ("ntok", torch.int32, (B,)),
                             ("tokens", torch.int32, (B * Tmax,))], dev)
        self.reset()

    def reset(self, rows=None):
        _lib.check(self._L.pafc_ctc_greedy_stream_reset(self.B, self._row_mask(rows), _lib.ptr(self._ws), self._nbytes,
                                                         _lib.stream_of(self._ws)),
                   "pafc_ctc_greedy_stream_reset")

    def feed(self, scores: torch.Tensor, nframes=None):
        """scores (B, n <= Tmax, V) float32 / bfloat16.  Returns (tokens, frames): per row what this chunk adds."""
        B, Tmax = self.B, self.Tmax
        if scores.dim() != 3 or scores.shape[0] != B or scores.shape[1] > Tmax:
            raise _lib.PafcError(f"CtcGreedyStream.feed: the chunk must be ({B}, n <= {Tmax}, V)")
        if scores.device != self.device:
            raise _lib.PafcError(f"CtcGreedyStream.feed: the chunk is not on {self.device}")
        n, V = scores.shape[1], scores.shape[2]
        if n == 0:
            return [[] for _ in range(B)], [[] for _ in range(B)]
        scores = scores.contiguous()
        self._set_nframes(nframes, n)
        out = self._out
        _lib.check(self._L.pafc_ctc_greedy_stream(_lib.dtype_code(scores.dtype), B, n, V, _lib.ptr(scores), _lib.ptr(self._nf),
                                                   self.blank, _lib.ptr(self._ws), self._nbytes, _lib.ptr(self._best),
                                                   out.ptr("tokens"), out.ptr("ntok"), out.ptr("frames"),
                                                   _lib.stream_of(scores)), "pafc_ctc_greedy_stream")
        out.read()
        cnt = out.host("ntok").tolist()
        fr, tk = out.host("frames")[:B * n].view(B, n), out.host("tokens")[:B * n].view(B, n)
        return [tk[b, :cnt[b]].tolist() for b in range(B)], [fr[b, :cnt[b]].tolist() for b in range(B)]


class RnntBeamState:
    """Device-side beams of the CTC-fused RNN-T prefix beam search (include/pafc_search.h: pafc_rnnt_beam_*)."""

    def __init__(self, B: int, T: int, beam: int, blank: int, device):
        L = _lib.lib()
        self._L, self.B, self.T, self.beam, self.blank = L, B, T, beam, blank
        self._nbytes = L.pafc_rnnt_beam_workspace_bytes(B, T, beam)
        if self._nbytes == 0:
            raise _lib.PafcError("rnnt beam search: B, T, beam must be positive")
        self._ws = torch.empty(self._nbytes, dtype=torch.uint8, device=device)
        self.next_idx = torch.empty(B * beam, dtype=torch.int64, device=device)
        self.last_tok = torch.empty(B * beam, dtype=torch.int64, device=device)
        self.stream = _lib.stream_of(self._ws)
        _lib.check(L.pafc_rnnt_beam_init(B, T, beam, blank, _lib.ptr(self._ws), self._nbytes, _lib.ptr(self.next_idx),
                                         _lib.ptr(self.last_tok), self.stream), "pafc_rnnt_beam_init")

    def step(self, t: int, lens64: Optional[torch.Tensor], top_val: torch.Tensor, top_idx: torch.Tensor,
             t_dev: Optional[torch.Tensor] = None):
        """t_dev: device int64 scalar holding the frame index (graph replay); otherwise ``t``."""
        _lib.require_gpu(top_val, top_idx, lens64, t_dev)
        if top_val.dtype != torch.float32 or top_idx.dtype != torch.int64 or top_val.numel() != self.B * self.beam * self.beam:
            raise _lib.PafcError("rnnt beam step: top_val float32 / top_idx int64 of (B, beam, beam)")
        _lib.check(self._L.pafc_rnnt_beam_step(self.B, self.T, self.beam, self.blank, int(t), _lib.ptr(t_dev),
                                              _lib.ptr(lens64), _lib.ptr(top_val), _lib.ptr(top_idx), _lib.ptr(self._ws),
                                              self._nbytes, _lib.ptr(self.next_idx), _lib.ptr(self.last_tok),
                                              _lib.stream_of(top_val)), "pafc_rnnt_beam_step")

    def finish(self):
        dev = self._ws.device
        tokens = torch.empty(self.B, self.beam, self.T, dtype=torch.int32, device=dev)
        lengths = torch.empty(self.B, self.beam, dtype=torch.int32, device=dev)
        scores = torch.empty(self.B, self.beam, dtype=torch.float64, device=dev)
        _lib.check(self._L.pafc_rnnt_beam_finish(self.B, self.T, self.beam, _lib.ptr(self._ws), self._nbytes, _lib.ptr(tokens),
                                                _lib.ptr(lengths), _lib.ptr(scores), self.stream), "pafc_rnnt_beam_finish")
        return tokens, lengths, scores


class RnntBeamStream(_RowStream):
    """Device-side beams of the CTC-fused RNN-T prefix beam search for B streams fed chunk by chunk (include/pafc_search.h:
    pafc_rnnt_beam_stream_*, csrc/rnnt_beam_stream.hip).  The object owns the workspace, `next_idx` / `last_tok` of the
    B x beam slots, the frame counts and the `from` offsets; the caller owns the frame body and the LSTM state.  Per chunk:
    feed(nframes), then for every chunk frame j the caller's body and step(j, top_val, top_idx) (j_dev: the frame from a
    device int64, for a captured body) and select_state(...); drain() is the one host read.  Given the same top_val /
    top_idx, every frame's next_idx / last_tok and the drained lists equal RnntBeamState's over the concatenated frames,
    bit for bit.  A row that would pass max_total_frames takes nothing and is reported by drain's `overflow`."""

    _pinned = True

    def __init__(self, B: int, Tmax: int, beam: int, blank: int, device, max_total_frames: int = 4096):
        dev = self._device(device)
        if B < 1 or Tmax < 1 or max_total_frames < 1:
            raise _lib.PafcError(f"RnntBeamStream: B {B}, Tmax {Tmax}, max_total_frames {max_total_frames} must be >= 1")
        if not 1 <= beam <= 16:
            raise _lib.PafcError(f"RnntBeamStream: beam {beam} must be in 1 .. 16")
        self.Tmax, self.beam, self.blank = Tmax, beam, int(blank)
        self.max_total = int(max_total_frames)
        self._init_rows(B, dev, "pafc_rnnt_beam_stream_workspace_bytes", (B, self.max_total, beam),
                        "unsupported dimensions (max_total_frames * beam < 2^31)")
        self._init_drain()
        self.next_idx = torch.empty(B * beam, dtype=torch.int64, device=dev)
        self.last_tok = torch.empty(B * beam, dtype=torch.int64, device=dev)
        self.reset()

    def reset(self, rows=None):
        """Restart the given rows (all when None): one live beam of score 0, the root node, last_tok = blank, the identity
        next_idx, no frames consumed, overflow flag cleared; other rows are untouched."""
        _lib.check(self._L.pafc_rnnt_beam_stream_reset(self.B, self.max_total, self.beam, self.blank, self._row_mask(rows),
                                                       _lib.ptr(self._ws), self._nbytes, _lib.ptr(self.next_idx),
                                                       _lib.ptr(self.last_tok), _lib.stream_of(self._ws)),
                   "pafc_rnnt_beam_stream_reset")

    def load(self, nframes, n: Optional[int] = None):
        """The frame counts of the next chunk into their device buffer (an int: every row; else (B,) counts, clamped to
        [0, n]; a device int64 tensor stays off the host)."""
        n = self.Tmax if n is None else n
        if isinstance(nframes, int):
            self._nf.fill_(max(0, min(n, nframes)))
        else:
            self._set_nframes(nframes, n)

    def launch_feed(self):
        """The feed kernel on the frame-count buffer: reads nothing from the host, allocates nothing."""
        _lib.check(self._L.pafc_rnnt_beam_stream_feed(self.B, self.Tmax, self.max_total, self.beam, _lib.ptr(self._nf),
                                                     _lib.ptr(self._ws), self._nbytes, _lib.stream_of(self._ws)),
                   "pafc_rnnt_beam_stream_feed")

    def feed(self, nframes, n: Optional[int] = None):
        """Begin a chunk: row b takes clamp(nframes[b], 0, min(n, Tmax)) frames."""
        self.load(nframes, n)
        self.launch_feed()

    def step(self, j: int, top_val: torch.Tensor, top_idx: torch.Tensor, j_dev: Optional[torch.Tensor] = None):
        """Frame j of the chunk (from the device int64 scalar j_dev when given) for every row that took more than j frames."""
        _lib.require_gpu(top_val, top_idx, j_dev)
        if top_val.dtype != torch.float32 or top_idx.dtype != torch.int64 or top_val.numel() != self.B * self.beam * self.beam \
                or top_idx.numel() != top_val.numel():
            raise _lib.PafcError("rnnt beam stream step: top_val float32 / top_idx int64 of (B, beam, beam)")
        _lib.check(self._L.pafc_rnnt_beam_stream_step(self.B, self.Tmax, self.max_total, self.beam, self.blank, int(j),
                                                     _lib.ptr(j_dev), _lib.ptr(top_val), _lib.ptr(top_idx), _lib.ptr(self._ws),
                                                     self._nbytes, _lib.ptr(self.next_idx), _lib.ptr(self.last_tok),
                                                     _lib.stream_of(top_val)), "pafc_rnnt_beam_stream_step")

    def select_state(self, h: torch.Tensor, c: torch.Tensor, h_new: torch.Tensor, c_new: torch.Tensor,
                     next_idx: Optional[torch.Tensor] = None):
        """h, c (layers, B * beam, hidden) in place: slot i takes row next_idx[i] of [old | new] (default: the last step's)."""
        rnnt_beam_select_state(h, c, h_new, c_new, self.next_idx if next_idx is None else next_idx, self.B, self.beam)

    def drain(self, counts=None, ld: int = 1):
        """The n-best of every row as if its stream ended here.  counts: per row the tokens the caller already holds as
        final (an earlier drain's `committed`), default 0.  Returns a dict of host lists: count (B), committed (B),
        overflow (B), len (B, beam: total token counts, -1 unused), score (B, beam), tokens (B, beam: the tokens from
        counts[b] on, at most ld of them).  One device-to-host copy."""
        def call(out, ld):
            _lib.check(self._L.pafc_rnnt_beam_stream_drain(self.B, self.max_total, self.beam, _lib.ptr(self._ws), self._nbytes,
                                                           _lib.ptr(self._from), ld, out.ptr("tokens"), out.ptr("len"),
                                                           out.ptr("score"), out.ptr("count"), out.ptr("committed"),
                                                           out.ptr("overflow"), _lib.stream_of(self._ws)),
                       "pafc_rnnt_beam_stream_drain")
        return self._drain_nbest(call, counts, ld)


def rnnt_beam_select_state(h: torch.Tensor, c: torch.Tensor, h_new: torch.Tensor, c_new: torch.Tensor, next_idx: torch.Tensor,
                           B: int, beam: int):
    """pafc_rnnt_beam_select_state: for h and c (layers, n = B * beam, hidden), in place and in one launch,
    h[l, i] = (next_idx[i] < n ? h : h_new)[l, next_idx[i] mod n] -- bit-equal to torch.cat([h, h_new], 1).index_select(1,
    next_idx) copied back.  next_idx must stay within each utterance's slots, as the step kernels emit it."""
    _lib.require_gpu(h, c, h_new, c_new, next_idx)
    if h.dim() != 3 or h.shape[1] != B * beam or not (h.shape == c.shape == h_new.shape == c_new.shape) \
            or not (h.dtype == c.dtype == h_new.dtype == c_new.dtype):
        raise _lib.PafcError("rnnt_beam_select_state: h, c, h_new, c_new must share the shape (layers, B * beam, hidden) and dtype")
    if next_idx.dtype != torch.int64 or next_idx.numel() != B * beam:
        raise _lib.PafcError("rnnt_beam_select_state: next_idx int64 of (B * beam)")
    _lib.check(_lib.lib().pafc_rnnt_beam_select_state(_lib.dtype_code(h.dtype), h.shape[0], B, beam, h.shape[2], _lib.ptr(h),
                                                      _lib.ptr(c), _lib.ptr(h_new), _lib.ptr(c_new), _lib.ptr(next_idx),
                                                      _lib.stream_of(h)), "pafc_rnnt_beam_select_state")


RNNT_BEAM_BODY_MAX_BEAM = 16


def rnnt_beam_body_unmet(predictor, joint, encoder_out: torch.Tensor, beam: int) -> Optional[str]:
    """The condition the frame-body kernels of the RNN-T prefix beam search (csrc/rnnt_beam_body.hip) do not meet for this
    predictor / joint, encoder output (B, T, D) -- or a tensor of its shape, dtype and device -- and beam, or None:
    rnnt_greedy_unmet's conditions, 1 <= beam <= 16 and a vocabulary of at least `beam` tokens."""
    if not 1 <= beam <= RNNT_BEAM_BODY_MAX_BEAM:
        return f"beam {beam} is outside 1 .. {RNNT_BEAM_BODY_MAX_BEAM}"
    unmet = rnnt_greedy_unmet(predictor, joint, encoder_out, 1)
    if unmet is not None:
        return unmet
    if joint.ffn_out.out_features < beam:
        return f"the vocabulary ({joint.ffn_out.out_features}) is smaller than beam {beam}"
    return None


class RnntBeamBody:
    """One frame of the RNN-T prefix beam search for B x beam slots as kernels (include/pafc_search.h: pafc_rnnt_beam_body).
    The object holds the net struct with the tensors it points into, the workspace and the frame's outputs: h_new, c_new
    (layers, B * beam, hidden) of the weights' dtype and top_val float32 / top_idx int64 (B, beam, beam), all at fixed
    addresses, so a frame can be captured.  The caller checks rnnt_beam_body_unmet first."""

    def __init__(self, predictor, joint, B: int, beam: int):
        self.B, self.beam, self.n = B, beam, B * beam
        self.dtype = joint.ffn_out.weight.dtype
        self.device = dev = joint.ffn_out.weight.device
        self._L = _lib.lib()
        self._net, self._keep = _greedy_net(predictor, joint)
        self._pnet = ctypes.byref(self._net)
        self._nbytes = self._L.pafc_rnnt_beam_body_workspace_bytes(self._pnet, B, beam)
        if self._nbytes == 0:
            raise _lib.PafcError("pafc_rnnt_beam_body_workspace_bytes: unsupported dimensions")
        self._w, self._b = _enc_ffn(joint)
        self.layers, self.hidden, self.join_dim = predictor.rnn.num_layers, predictor.rnn.hidden_size, joint.ffn_out.in_features
        self.vocab = joint.ffn_out.out_features
        self._ws = torch.empty(self._nbytes, dtype=torch.uint8, device=dev)
        self.h_new = torch.empty(self.layers, self.n, self.hidden, dtype=self.dtype, device=dev)
        self.c_new = torch.empty_like(self.h_new)
        self.top_val = torch.empty(B, beam, beam, dtype=torch.float32, device=dev)
        self.top_idx = torch.empty(B, beam, beam, dtype=torch.int64, device=dev)

    def zero_state(self):
        """(h, c) of a fresh search: zeros (layers, B * beam, hidden)."""
        return torch.zeros_like(self.h_new), torch.zeros_like(self.c_new)

    def project(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """E = enc_ffn(x) for rows x (rows, D) through gemm_f32 / gemm_bf16, as rnnt_greedy_search computes it."""
        return _enc_project(x, self._w, self._b, out=out)

    def frame(self, E: torch.Tensor, ctc: torch.Tensor, w_rnnt: float, w_ctc: float, last_tok: torch.Tensor, h: torch.Tensor,
              c: torch.Tensor, t: int = 0, t_dev: Optional[torch.Tensor] = None):
        """Frame t (from the device int64 scalar t_dev when given; clamped to T - 1) of E (B, T, J) and of the log-probabilities
        ctc (B, T, V), fp32 or bf16, rows of any stride: (h, c) and last_tok (B * beam) in; h_new, c_new, top_val, top_idx out."""
        B, n = self.B, self.n
        _lib.require_gpu(E, last_tok, h, c, t_dev)
        if E.dim() != 3 or E.shape[0] != B or E.shape[2] != self.join_dim or E.dtype != self.dtype:
            raise _lib.PafcError(f"rnnt beam body: E must be ({B}, T, {self.join_dim}) of {self.dtype}")
        T = E.shape[1]
        ok = ctc.is_cuda and ctc.dim() == 3 and ctc.shape[:2] == E.shape[:2] and ctc.shape[2] >= self.vocab and ctc.stride(2) == 1
        # the row stride (a dimension of extent 1 reports any stride)
        ldc = (ctc.stride(1) if T > 1 else ctc.stride(0) if B > 1 else ctc.shape[2]) if ok else 0
        if not ok or ldc < self.vocab or (B > 1 and T > 1 and ctc.stride(0) != T * ldc):
            raise _lib.PafcError(f"rnnt beam body: ctc must be ({B}, {T}, >= {self.vocab}) on the GPU, rows of one stride, unit "
                                 "stride along the vocabulary")
        state = (self.layers, n, self.hidden)
        if tuple(h.shape) != state or tuple(c.shape) != state or h.dtype != self.dtype or c.dtype != self.dtype:
            raise _lib.PafcError(f"rnnt beam body: h, c must be {state} of {self.dtype}")
        if last_tok.dtype != torch.int64 or last_tok.numel() != n or (t_dev is not None and t_dev.dtype != torch.int64):
            raise _lib.PafcError(f"rnnt beam body: last_tok int64 of ({n}), t_dev int64")
        _lib.check(self._L.pafc_rnnt_beam_body(self._pnet, B, T, self.beam, int(t), _lib.ptr(t_dev), _lib.ptr(E),
                                               _lib.dtype_code(ctc.dtype), _lib.ptr(ctc), ldc, float(w_rnnt), float(w_ctc),
                                               _lib.ptr(last_tok), _lib.ptr(h), _lib.ptr(c), _lib.ptr(self.h_new),
                                               _lib.ptr(self.c_new), _lib.ptr(self.top_val), _lib.ptr(self.top_idx),
                                               _lib.ptr(self._ws), self._nbytes, _lib.stream_of(E)), "pafc_rnnt_beam_body")

    def advance(self, t_dev: torch.Tensor):
        """t_dev += 1 as a kernel of the library's: the last launch of a captured frame."""
        _lib.require_gpu(t_dev)
        _lib.check(self._L.pafc_rnnt_beam_body_advance(_lib.ptr(t_dev), _lib.stream_of(t_dev)), "pafc_rnnt_beam_body_advance")


def rnnt_beam_frame(predictor, joint, E: torch.Tensor, ctc: torch.Tensor, last_tok: torch.Tensor, h: torch.Tensor,
                    c: torch.Tensor, beam: int, t: int = 0, t_dev: Optional[torch.Tensor] = None, ctc_weight: float = 0.3,
                    transducer_weight: float = 0.7):
    """One frame of the frame-body kernels on explicit tensors (tests and tools): E (B, T, J) = enc_ffn(encoder_out), ctc
    (B, T, V) log-probabilities, last_tok (B * beam), h / c (layers, B * beam, hidden).  Returns (top_val, top_idx, h_new,
    c_new), top_* of (B, beam, beam)."""
    D = joint.enc_ffn.in_features if getattr(joint, "enc_ffn", None) is not None else 4
    unmet = rnnt_beam_body_unmet(predictor, joint, _shape_like(E.shape[0], E.shape[1], D, E.device), beam)
    if unmet is not None:
        raise _lib.PafcError(f"rnnt_beam_frame: {unmet}")
    body = RnntBeamBody(predictor, joint, E.shape[0], beam)
    body.frame(E, ctc, transducer_weight, ctc_weight, last_tok, h, c, t, t_dev)
    return body.top_val, body.top_idx, body.h_new, body.c_new


def split_bf16(t: torch.Tensor):
    """fp32 tensor -> (hi, lo) bf16 planes with t ~= hi + lo (16 significant bits)."""
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


def conv_sub_f32split(x: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2_hi: torch.Tensor,
                      w2_lo: torch.Tensor, b2: Optional[torch.Tensor]) -> torch.Tensor:
    """Both subsampling convolutions (+ ReLU) for fp32 activations on the bf16 matrix cores with split operands
    (include/pafc_encoder_ops.h: pafc_conv3x3s2_*_f32split).  x (B, T, F) fp32; w1 (C, 1, 3, 3) fp32; w2_hi / w2_lo
    (9, C, C) bf16 = split_bf16 of the second Conv2d weight in (tap, co, ci) order -> (B, T', F', C) fp32."""
    _lib.require_gpu(x, w1, b1, w2_hi, w2_lo, b2)
    if x.dtype != torch.float32 or w1.dtype != torch.float32 or w2_hi.dtype != torch.bfloat16 or x.dim() != 3:
        raise _lib.PafcError("conv_sub_f32split: fp32 x (B, T, F) / w1, bf16 split planes for w2")
    L = _lib.lib()
    B, T, Fd = x.shape
    C = w1.shape[0]
    T1, F1 = (T - 3) // 2 + 1, (Fd - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    hi = torch.empty((B, T1, F1, C), dtype=torch.bfloat16, device=x.device)
    lo = torch.empty_like(hi)
    st = _lib.stream_of(x)
    _lib.check(L.pafc_conv3x3s2_c1_nhwc_f32split(B, T, Fd, C, _lib.ptr(x), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(hi),
                                                 _lib.ptr(lo), 1, st), "pafc_conv3x3s2_c1_nhwc_f32split")
    out = torch.empty((B, T2, F2, C), dtype=torch.float32, device=x.device)
    _lib.check(L.pafc_conv3x3s2_nhwc_f32split(B, T1, F1, C, C, _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(w2_hi), _lib.ptr(w2_lo),
                                              _lib.ptr(b2), _lib.ptr(out), 1, st), "pafc_conv3x3s2_nhwc_f32split")
    return out


def conv_sub_f32split_planes(x: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2_3: torch.Tensor,
                             b2: Optional[torch.Tensor]) -> torch.Tensor:
    """Both subsampling convolutions (+ ReLU) of an fp32 model at long-form sizes: conv1 in fp32 arithmetic writing planes
    [hi C | lo C] per pixel, conv2 as the split-operand implicit GEMM of csrc/gemm_ph.hip (include/pafc_encoder_ops.h:
    pafc_conv3x3s2_nhwc_split_ph).  x (B, T, F) fp32; w1 (C, 1, 3, 3) fp32; w2_3 (9, C, 3 C) = split_planes(w2 taps, triple)
    -> (B, T', F', 2 C) bf16 planes [hi C | lo C] of the fp32 result, the A operand of gemm_ph_ex(a_split, a_plane_block=C)."""
    _lib.require_gpu(x, w1, b1, w2_3, b2)
    B, T, Fd = x.shape
    C = w1.shape[0]
    if x.dtype != torch.float32 or w1.dtype != torch.float32 or w2_3.dtype != torch.bfloat16 or tuple(w2_3.shape) != (9, C, 3 * C):
        raise _lib.PafcError("conv_sub_f32split_planes: fp32 x (B, T, F) / w1, w2 as (9, C, 3C) bf16 planes")
    L = _lib.lib()
    T1, F1 = (T - 3) // 2 + 1, (Fd - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    y1 = torch.empty((B, T1, F1, 2 * C), dtype=torch.bfloat16, device=x.device)
    st = _lib.stream_of(x)
    lo = c_void_p(y1.data_ptr() + 2 * C)
    _lib.check(L.pafc_conv3x3s2_c1_nhwc_f32split_ps(B, T, Fd, C, _lib.ptr(x), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(y1), lo, 2 * C, 1, st),
               "pafc_conv3x3s2_c1_nhwc_f32split_ps")
    out = torch.empty((B, T2, F2, 2 * C), dtype=torch.bfloat16, device=x.device)
    from .profiling import op_timer
    with op_timer("conv3x3s2_split", flops=2.0 * B * T2 * F2 * C * 9 * C * 3):
        rc = L.pafc_conv3x3s2_nhwc_split_ph(B, T1, F1, C, C, _lib.ptr(y1), _lib.ptr(w2_3), _lib.ptr(b2), _lib.ptr(out), 1,
                                            _ph_tile_m(B * T2 * F2, C, min_tm=128), st)
    _lib.check(rc, "pafc_conv3x3s2_nhwc_split_ph")
    return out


def causal_conv_silu_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], reverse: bool = False
                        ) -> torch.Tensor:
    """SiLU(causal depthwise conv1d) in channels-last layout: x (B, L, C) -- may be a column slice of a wider tensor --
    weight (C, 1, K) -> (B, L, C) contiguous (include/pafc_encoder_ops.h: pafc_dwconv1d_cl_ex, act 2).  reverse: the
    convolution that is causal in reversed time (what flip -> conv -> flip computes), i.e. the taps reversed and looking
    right: same kernel, left_pad 0."""
    _lib.require_gpu(weight, bias)
    if not x.is_cuda or x.dim() != 3 or x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        raise _lib.PafcError("causal_conv_silu_cl: (B, L, C) GPU tensor, unit stride in C, batch stride L * row stride")
    B, Lq, C = x.shape
    K = weight.shape[-1]
    y = torch.empty((B, Lq, C), dtype=x.dtype, device=x.device)
    if reverse:
        weight = weight.flip(-1).contiguous()
    rc = _lib.lib().pafc_dwconv1d_cl_ex(_lib.dtype_code(x.dtype), B, Lq, C, K, 0 if reverse else K - 1, Lq, _lib.ptr(x),
                                        x.stride(1), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), 2, None,
                                        _lib.stream_of(x))
    _lib.check(rc, "pafc_dwconv1d_cl_ex")
    return y


def causal_conv_silu_cl_prefix(xp: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """SiLU(causal depthwise conv1d) of a chunk whose left context is laid out in front of it: xp (B, K - 1 + T, C)
    contiguous = [the K - 1 rows before the chunk | the chunk], weight (C, 1, K) -> (B, T, C).  Three zero rows in front are the
    module's own causal zero padding (the start of a stream).  pafc_dwconv1d_cl_ex with left_pad 0, T_out = T_in - (K - 1)."""
    _lib.require_gpu(xp, weight, bias)
    K = weight.shape[-1]
    if xp.dim() != 3 or not xp.is_contiguous() or xp.shape[1] < K:
        raise _lib.PafcError("causal_conv_silu_cl_prefix: contiguous (B, K - 1 + T, C) with T >= 1")
    B, Tin, C = xp.shape
    T = Tin - (K - 1)
    y = torch.empty((B, T, C), dtype=xp.dtype, device=xp.device)
    rc = _lib.lib().pafc_dwconv1d_cl_ex(_lib.dtype_code(xp.dtype), B, Tin, C, K, 0, T, _lib.ptr(xp), C, _lib.ptr(weight),
                                        _lib.ptr(bias), _lib.ptr(y), 2, None, _lib.stream_of(xp))
    _lib.check(rc, "pafc_dwconv1d_cl_ex")
    return y


def mamba2_prep(xbc: torch.Tensor, dt_raw: torch.Tensor, dt_bias: torch.Tensor, A_log: torch.Tensor, d_inner: int):
    """xbc (B, L, d_inner + 256) contiguous, dt_raw (B, L, H) slice -> [r0, r1, k0, k1, v, w] fp32 (B, L, d_inner)."""
    _lib.require_gpu(xbc, dt_bias, A_log)
    if xbc.dim() != 3 or not xbc.is_contiguous() or xbc.shape[2] != d_inner + 256:
        raise _lib.PafcError("mamba2_prep: contiguous xbc (B, L, d_inner + 256)")
    B, Lq, _ = xbc.shape
    planes = [torch.empty((B, Lq, d_inner), dtype=torch.float32, device=xbc.device) for _ in range(6)]
    rc = _lib.lib().pafc_mamba2_prep(_lib.dtype_code(xbc.dtype), B, Lq, d_inner, _lib.ptr(xbc), _lib.ptr(dt_raw),
                                     dt_raw.stride(1), _lib.ptr(dt_bias), _lib.ptr(A_log), *[_lib.ptr(t) for t in planes],
                                     _lib.stream_of(xbc))
    _lib.check(rc, "pafc_mamba2_prep")
    return planes


def mamba2_scan(xbc: torch.Tensor, dt: torch.Tensor, log_a: torch.Tensor, H: int, reverse: bool = False,
                D: Optional[torch.Tensor] = None, chunk_len: int = 0) -> torch.Tensor:
    """Mamba-2 selective scan on the dedicated SSD kernel: xbc (B, L, >= H*64 + 256) bf16 contiguous, dt / log_a (B, L, H)
    fp32 contiguous -> y (B, L, H*64) fp32 (include/pafc_encoder_ops.h: pafc_mamba2_scan_dir); with D (H) fp32 the scan returns
    bf16(y + D x) as mamba_ssm's does (pafc_mamba2_scan_skip_bf16).  chunk_len 0: the library's own chunk length."""
    _lib.require_gpu(xbc, dt, log_a, D)
    if xbc.dtype != torch.bfloat16 or dt.dtype != torch.float32 or log_a.dtype != torch.float32:
        raise _lib.PafcError("mamba2_scan: bf16 xbc, fp32 dt / log_a")
    if xbc.dim() != 3 or not xbc.is_contiguous() or not dt.is_contiguous() or not log_a.is_contiguous():
        raise _lib.PafcError("mamba2_scan: contiguous xbc (B, L, >= H * 64 + 256), dt / log_a (B, L, H)")
    B, Lq, ldx = xbc.shape
    if tuple(dt.shape) != (B, Lq, H) or tuple(log_a.shape) != (B, Lq, H) or ldx < H * 64 + 256:
        raise _lib.PafcError("mamba2_scan: dt / log_a must be (B, L, H), xbc rows at least H * 64 + 256 wide")
    Lb = _lib.lib()
    nws = Lb.pafc_mamba2_scan_workspace_bytes(B, Lq, H, chunk_len)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=xbc.device)
    if D is not None:
        if D.dtype != torch.float32 or D.shape != (H,):
            raise _lib.PafcError("mamba2_scan: D must be float32 (H)")
        y = torch.empty((B, Lq, H * 64), dtype=torch.bfloat16, device=xbc.device)
        rc = Lb.pafc_mamba2_scan_skip_bf16(B, Lq, H, _lib.ptr(xbc), ldx, _lib.ptr(dt), _lib.ptr(log_a), _lib.ptr(D),
                                           _lib.ptr(y), int(reverse), chunk_len, _lib.ptr(ws) if nws else None, nws,
                                           _lib.stream_of(xbc))
        _lib.check(rc, "pafc_mamba2_scan_skip_bf16")
        return y
    y = torch.empty((B, Lq, H * 64), dtype=torch.float32, device=xbc.device)
    rc = Lb.pafc_mamba2_scan_dir(B, Lq, H, _lib.ptr(xbc), ldx, _lib.ptr(dt), _lib.ptr(log_a), _lib.ptr(y), int(reverse), chunk_len,
                                 _lib.ptr(ws) if nws else None, nws, _lib.stream_of(xbc))
    _lib.check(rc, "pafc_mamba2_scan_dir")
    return y


def mamba2_scan_state(xbc: torch.Tensor, dt: torch.Tensor, log_a: torch.Tensor, H: int, s_in: Optional[torch.Tensor] = None,
                      s_out: Optional[torch.Tensor] = None, reverse: bool = False, D: Optional[torch.Tensor] = None,
                      want_state: bool = True, chunk_len: int = 0):
    """mamba2_scan from an initial state, returning the final one (include/pafc_encoder_ops.h: pafc_mamba2_scan_state).
    s_in / s_out: float32 (B, H, 128, 64) [state dim][head channel]; s_in None = zero state; s_out None = allocated here when
    want_state; s_out may BE s_in (the state is updated where it lies).  -> (y, s_out): y fp32 raw scan, or with D (H) fp32
    bf16(scan + D x)."""
    _lib.require_gpu(xbc, dt, log_a, D, s_in, s_out)
    if xbc.dtype != torch.bfloat16 or dt.dtype != torch.float32 or log_a.dtype != torch.float32:
        raise _lib.PafcError("mamba2_scan_state: bf16 xbc, fp32 dt / log_a")
    if xbc.dim() != 3 or not xbc.is_contiguous() or not dt.is_contiguous() or not log_a.is_contiguous():
        raise _lib.PafcError("mamba2_scan_state: contiguous xbc (B, L, H * 64 + 256), dt / log_a (B, L, H)")
    B, Lq, ldx = xbc.shape
    if tuple(dt.shape) != (B, Lq, H) or tuple(log_a.shape) != (B, Lq, H):
        raise _lib.PafcError("mamba2_scan_state: dt / log_a must be (B, L, H)")
    for name, s in (("s_in", s_in), ("s_out", s_out)):
        if s is not None and (s.dtype != torch.float32 or tuple(s.shape) != (B, H, 128, 64) or not s.is_contiguous()):
            raise _lib.PafcError(f"mamba2_scan_state: {name} must be contiguous float32 (B, H, 128, 64)")
    if D is not None and (D.dtype != torch.float32 or tuple(D.shape) != (H,)):
        raise _lib.PafcError("mamba2_scan_state: D must be float32 (H)")
    if s_out is None and want_state:
        s_out = torch.empty((B, H, 128, 64), dtype=torch.float32, device=xbc.device)
    Lb = _lib.lib()
    nws = Lb.pafc_mamba2_scan_workspace_bytes(B, Lq, H, chunk_len)
    ws = torch.empty(nws, dtype=torch.uint8, device=xbc.device) if nws else None
    y = torch.empty((B, Lq, H * 64), dtype=torch.bfloat16 if D is not None else torch.float32, device=xbc.device)
    rc = Lb.pafc_mamba2_scan_state(B, Lq, H, _lib.ptr(xbc), ldx, _lib.ptr(dt), _lib.ptr(log_a), _lib.ptr(D),
                                   None if D is not None else _lib.ptr(y), _lib.ptr(y) if D is not None else None,
                                   _lib.ptr(s_in), _lib.ptr(s_out), int(reverse), chunk_len, _lib.ptr(ws), nws,
                                   _lib.stream_of(xbc))
    _lib.check(rc, "pafc_mamba2_scan_state")
    return y, s_out


def mamba2_scan_backward(xbc: torch.Tensor, dt: torch.Tensor, log_a: torch.Tensor, gy: torch.Tensor, H: int,
                         reverse: bool = False, chunk_len: int = 0):
    """Backward of mamba2_scan's fp32 form (include/pafc_encoder_ops.h: pafc_mamba2_scan_backward): xbc (B, L, ldx) bf16
    contiguous, dt / log_a (B, L, H) fp32, gy (B, L, H*64) fp32 = dL/dy  ->  (g_xbc bf16 like xbc: [g_x | g_B | g_C] with g_B,
    g_C summed over the heads, g_dt, g_la fp32 (B, L, H)).  g_dt is the gradient through the argument dt alone."""
    _lib.require_gpu(xbc, dt, log_a, gy)
    if xbc.dtype != torch.bfloat16 or dt.dtype != torch.float32 or log_a.dtype != torch.float32 or gy.dtype != torch.float32:
        raise _lib.PafcError("mamba2_scan_backward: bf16 xbc, fp32 dt / log_a / gy")
    if xbc.dim() != 3 or not xbc.is_contiguous() or not dt.is_contiguous() or not log_a.is_contiguous() or not gy.is_contiguous():
        raise _lib.PafcError("mamba2_scan_backward: contiguous xbc (B, L, >= H * 64 + 256), dt / log_a (B, L, H), gy (B, L, H * 64)")
    B, Lq, ldx = xbc.shape
    if tuple(dt.shape) != (B, Lq, H) or tuple(log_a.shape) != (B, Lq, H) or tuple(gy.shape) != (B, Lq, H * 64):
        raise _lib.PafcError("mamba2_scan_backward: dt / log_a must be (B, L, H), gy (B, L, H * 64)")
    Lb = _lib.lib()
    nws = Lb.pafc_mamba2_scan_bwd_workspace_bytes(B, Lq, H, chunk_len)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=xbc.device)
    g_xbc = torch.empty_like(xbc) if ldx == H * 64 + 256 else torch.zeros_like(xbc)     # (padding columns: zero)
    g_dt = torch.empty_like(dt)
    g_la = torch.empty_like(log_a)
    rc = Lb.pafc_mamba2_scan_backward(B, Lq, H, _lib.ptr(xbc), ldx, _lib.ptr(dt), _lib.ptr(log_a), _lib.ptr(gy), _lib.ptr(g_xbc),
                                      ldx, _lib.ptr(g_dt), _lib.ptr(g_la), int(reverse), chunk_len, _lib.ptr(ws), nws,
                                      _lib.stream_of(xbc))
    _lib.check(rc, "pafc_mamba2_scan_backward")
    return g_xbc, g_dt, g_la


class _Mamba2ScanTrain(torch.autograd.Function):
    """y = mamba2_scan(xbc, dt, log_a) in fp32 with the SSD backward kernel behind it."""

    @staticmethod
    def forward(ctx, xbc, dt, log_a, H, reverse):
        xbc, dt, log_a = xbc.contiguous(), dt.contiguous(), log_a.contiguous()
        ctx.save_for_backward(xbc, dt, log_a)
        ctx.H, ctx.reverse = H, reverse
        return mamba2_scan(xbc, dt, log_a, H, reverse)

    @staticmethod
    def backward(ctx, gy):
        xbc, dt, log_a = ctx.saved_tensors
        g_xbc, g_dt, g_la = mamba2_scan_backward(xbc, dt, log_a, gy.float().contiguous(), ctx.H, ctx.reverse)
        return g_xbc, g_dt, g_la, None, None


def mamba2_scan_train(xbc: torch.Tensor, dt: torch.Tensor, log_a: torch.Tensor, H: int, reverse: bool = False) -> torch.Tensor:
    """mamba2_scan (fp32 y, no D term) as a differentiable op: gradients reach xbc (bf16, its shape), dt and log_a."""
    return _Mamba2ScanTrain.apply(xbc, dt, log_a, H, bool(reverse))


def mamba2_gate_norm(y: torch.Tensor, z: torch.Tensor, norm_weight: torch.Tensor, eps: float) -> torch.Tensor:
    """RMSNorm(y * silu(z)) * norm_weight over the last axis; z may be a column slice of a wider tensor."""
    _lib.require_gpu(y, norm_weight)
    d = y.shape[-1]
    rows = y.numel() // d
    if z.dtype != y.dtype or norm_weight.dtype != y.dtype or z.stride(-1) != 1 or z.shape != y.shape or not z.is_cuda:
        raise _lib.PafcError("mamba2_gate_norm: y, z, norm_weight in one dtype; z shaped like y with unit channel stride")
    out = torch.empty_like(y)
    rc = _lib.lib().pafc_mamba2_gate_norm(_lib.dtype_code(y.dtype), rows, d, _lib.ptr(y), _lib.ptr(z), z.stride(-2),
                                          _lib.ptr(norm_weight), float(eps), _lib.ptr(out), _lib.stream_of(y))
    _lib.check(rc, "pafc_mamba2_gate_norm")
    return out


def mamba2_finish(y0, y1, xbc, dt_raw, z, dt_bias, D, norm_weight, eps: float, d_inner: int, diag: bool = True
                  ) -> torch.Tensor:
    _lib.require_gpu(y0, y1, xbc, dt_bias, D, norm_weight)
    if xbc.dim() != 3 or not xbc.is_contiguous() or xbc.shape[2] != d_inner + 256:
        raise _lib.PafcError("mamba2_finish: contiguous xbc (B, L, d_inner + 256)")
    B, Lq, _ = xbc.shape
    out = torch.empty((B, Lq, d_inner), dtype=xbc.dtype, device=xbc.device)
    rc = _lib.lib().pafc_mamba2_finish(_lib.dtype_code(xbc.dtype), B, Lq, d_inner, _lib.ptr(y0), _lib.ptr(y1), _lib.ptr(xbc),
                                       _lib.ptr(dt_raw), dt_raw.stride(1), _lib.ptr(z), z.stride(1), _lib.ptr(dt_bias),
                                       _lib.ptr(D), _lib.ptr(norm_weight), float(eps), int(diag), _lib.ptr(out),
                                       _lib.stream_of(xbc))
    _lib.check(rc, "pafc_mamba2_finish")
    return out


class RowsTable:
    """A table of tensors whose rows move between a pool of S slots and a dense batch in ONE launch each way
    (pafc_rows_gather / pafc_rows_scatter).  entries: [(pool (S, ...), compact (>= m, ...))] with equal row shapes and dtypes,
    both contiguous; rings: [(ring (S, frames, F), window (>= m, w, F))] -- gather only: compact row j receives the w frames
    that start at frame offs[j] of its slot's ring, wrapping.  The host copy and the device copy of the table are made once,
    here: the tensors must stay where they are for the life of the table.  gather(idx, m, offs) / scatter(idx, m): idx device
    int32 (>= m), compact row j is pool slot idx[j]; idx[j] < 0 is a padding row (gather: zeros, scatter: skipped); offs
    device int32 (>= m) BYTE offsets into the rings (frame index x frame_bytes).  No wait, nothing allocated: both can be captured."""

    def __init__(self, entries, rings=()):
        rows, self.S, self.rows_max, dev = [], None, None, None
        self._frame_bytes = None
        for ring, (pool, comp) in [(False, e) for e in entries] + [(True, e) for e in rings]:
            _lib.require_gpu(pool, comp)
            if pool.device != comp.device or pool.dtype != comp.dtype or pool.dim() < 1 or comp.dim() != pool.dim():
                raise _lib.PafcError("RowsTable: a pool tensor and its compact tensor must share device, dtype and rank")
            if dev is None:
                dev, self.S = pool.device, pool.size(0)
            if pool.device != dev or pool.size(0) != self.S:
                raise _lib.PafcError("RowsTable: every pool tensor must have the same number of slots on one device")
            es = pool.element_size()
            if ring:
                if pool.dim() != 3 or pool.size(2) != comp.size(2) or comp.size(1) > pool.size(1):
                    raise _lib.PafcError("RowsTable: a ring is (S, frames, F) and its window (m, w <= frames, F)")
                fb = pool.size(2) * es
                if self._frame_bytes not in (None, fb):
                    raise _lib.PafcError("RowsTable: the rings of one table must have frames of one size")
                self._frame_bytes = fb
                rows.append([pool.data_ptr(), comp.data_ptr(), comp.size(1) * fb, pool.size(1) * fb])
            else:
                if pool.shape[1:] != comp.shape[1:]:
                    raise _lib.PafcError(f"RowsTable: row shapes differ ({tuple(pool.shape[1:])} and {tuple(comp.shape[1:])})")
                rows.append([pool.data_ptr(), comp.data_ptr(), (pool.numel() // max(self.S, 1)) * es, 0])
            self.rows_max = comp.size(0) if self.rows_max is None else min(self.rows_max, comp.size(0))
        if not rows:
            raise _lib.PafcError("RowsTable: no entries")
        self.n, self.device = len(rows), dev
        self._has_ring = any(r[3] for r in rows)
        flat = [v for r in rows for v in r]
        self._host = (ctypes.c_long * len(flat))(*flat)
        self._dev = torch.tensor(flat, dtype=torch.int64).to(dev)
        self._keep = (list(entries), list(rings))
        self._L = _lib.lib()

    def _idx(self, idx, m, what):
        if idx is None or not idx.is_cuda or idx.device != self.device or idx.dtype != torch.int32 or idx.dim() != 1 \
                or not idx.is_contiguous() or idx.numel() < m:
            raise _lib.PafcError(f"RowsTable: {what} must be a contiguous int32 tensor of >= {m} elements on {self.device}")
        return idx

    def _m(self, m):
        if not 1 <= m <= self.rows_max:
            raise _lib.PafcError(f"RowsTable: m = {m} rows, the compact tensors hold {self.rows_max}")
        return int(m)

    def gather(self, idx: torch.Tensor, m: int, offs: Optional[torch.Tensor] = None) -> None:
        m = self._m(m)
        self._idx(idx, m, "idx")
        if self._has_ring:
            self._idx(offs, m, "offs")
        rc = self._L.pafc_rows_gather(self._host, _lib.ptr(self._dev), self.n, _lib.ptr(idx),
                                      _lib.ptr(offs if self._has_ring else None), m, self.S, _lib.stream_of(idx))
        _lib.check(rc, "pafc_rows_gather")

    def scatter(self, idx: torch.Tensor, m: int) -> None:
        m = self._m(m)
        self._idx(idx, m, "idx")
        rc = self._L.pafc_rows_scatter(self._host, _lib.ptr(self._dev), self.n, _lib.ptr(idx), m, self.S, _lib.stream_of(idx))
        _lib.check(rc, "pafc_rows_scatter")

    @property
    def frame_bytes(self) -> int:
        """Bytes of one ring frame: offs[j] = (frame mod ring frames) * frame_bytes."""
        return self._frame_bytes or 0


def rows_gather(entries, idx: torch.Tensor, m: int, rings=(), offs: Optional[torch.Tensor] = None) -> None:
    """One-off RowsTable(entries, rings).gather(idx, m, offs) (the table is built and uploaded for this call)."""
    RowsTable(entries, rings).gather(idx, m, offs)


def rows_scatter(entries, idx: torch.Tensor, m: int) -> None:
    """One-off RowsTable(entries).scatter(idx, m)."""
    RowsTable(entries).scatter(idx, m)


def mha_rows(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_off: torch.Tensor, kv_off: torch.Tensor, kv_len: torch.Tensor,
             heads: int, causal: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Multi-head attention over packed row groups (include/pafc_attention.h: pafc_mha_rows), one launch for every group and
    head.  q (rows, >= H * 64), k / v (kv rows, >= H * 64): 2-D fp32 or bf16, unit stride in the last dimension (column slices
    of a stacked projection are fine; k and v share a row pitch); q_off (G + 1), kv_off / kv_len (G) int32 on the device.
    Group g: query rows [q_off[g], q_off[g + 1]) over the keys / values [kv_off[g], kv_off[g] + kv_len[g]); causal: query i of
    its group sees the keys [0, i].  Returns out (rows, H * 64)."""
    d = heads * 64
    for t in (q, k, v):
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != q.dtype or t.shape[1] < d:
            raise _lib.PafcError("mha_rows: q, k, v are 2-D GPU tensors of one dtype, unit stride along the heads")
    if k.stride(0) != v.stride(0):
        raise _lib.PafcError("mha_rows: k and v must share their row pitch")
    for t in (q_off, kv_off, kv_len):
        if not t.is_cuda or t.dtype != torch.int32 or t.stride(-1) != 1:
            raise _lib.PafcError("mha_rows: q_off, kv_off, kv_len are int32 GPU tensors")
    G = kv_len.numel()
    if q_off.numel() != G + 1 or kv_off.numel() != G:
        raise _lib.PafcError("mha_rows: q_off (G + 1), kv_off (G), kv_len (G)")
    if out is None:
        out = torch.empty(q.shape[0], d, dtype=q.dtype, device=q.device)
    elif not out.is_cuda or out.dtype != q.dtype or out.dim() != 2 or out.stride(1) != 1 or out.shape != (q.shape[0], d):
        raise _lib.PafcError("mha_rows: out is (rows, H * 64) in the operands' dtype")
    if G == 0 or q.shape[0] == 0:
        return out
    rc = _lib.lib().pafc_mha_rows(_lib.dtype_code(q.dtype), G, heads, 64, _lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v),
                                  k.stride(0), _lib.ptr(q_off), _lib.ptr(kv_off), _lib.ptr(kv_len), int(bool(causal)),
                                  _lib.ptr(out), out.stride(0), _lib.stream_of(q))
    _lib.check(rc, "pafc_mha_rows")
    return out


def mha_band(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, p: torch.Tensor, pos_bias_u: torch.Tensor,
             pos_bias_v: torch.Tensor, batch: int, heads: int, w: int, t_pad: Optional[int] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Limited-context self-attention with the positional term (include/pafc_attention.h: pafc_mha_band), one launch for every
    batch row, head and query tile.  q, k, v (batch * T, >= H * 64): 2-D fp32 or bf16 with unit stride along the heads, row
    b * T + i = frame i of batch row b (column slices of one stacked Q | K | V projection are fine; k and v share a row pitch);
    p (T, >= H * 64): the projected position rows, shared by the batch; pos_bias_u / pos_bias_v (H, 64) contiguous.  Query i
    sees the keys j with |j - i| <= w, 0 <= j < t_pad; the keys of [T, t_pad) are the reference's unmasked zero padding (score
    0, value 0) and are never read.  t_pad None: T rounded up to a multiple of 2 w, the reference's value.  Returns out
    (batch * T, H * 64)."""
    d, per16 = heads * 64, 16 // q.element_size()
    T, t_pad = _mha_band_operands("mha_band", q, k, v, p, pos_bias_u, pos_bias_v, batch, heads, w, t_pad)
    if out is None:
        out = torch.empty(q.shape[0], d, dtype=q.dtype, device=q.device)
    elif (not out.is_cuda or out.dtype != q.dtype or out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != (q.shape[0], d)
          or out.stride(0) % per16 or out.data_ptr() % 16):
        raise _lib.PafcError("mha_band: out is (batch * T, H * 64) in the operands' dtype, 16-byte aligned rows")
    from .profiling import op_timer
    # 384 flop per (query, key) pair: a 128-deep score and a 64-wide PV; the band's corners counted as full (an upper figure)
    with op_timer("mha_band_w%d" % w, sample=12, flops=384.0 * batch * heads * T * min(T, 2 * w + 1)):
        rc = _lib.lib().pafc_mha_band(_lib.dtype_code(q.dtype), batch, T, heads, 64, int(w), int(t_pad), _lib.ptr(q), q.stride(0),
                                      _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(p), p.stride(0), _lib.ptr(pos_bias_u),
                                      _lib.ptr(pos_bias_v), _lib.ptr(out), out.stride(0), _lib.stream_of(q))
    _lib.check(rc, "pafc_mha_band")
    return out


def logp_gather_rows(logits: torch.Tensor, target: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = logits[r, target[r]] - logsumexp(logits[r]) (include/pafc_attention.h: pafc_logp_gather_rows): the logits are
    read once, the (rows, V) log-softmax is never formed.  logits (rows, V) fp32 / bf16 with unit stride along V, target (rows)
    int32 on the device; out (rows) float32."""
    if not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1:
        raise _lib.PafcError("logp_gather_rows: logits are a 2-D GPU tensor with unit stride along the vocabulary")
    rows, V = logits.shape
    if not target.is_cuda or target.dtype != torch.int32 or target.numel() != rows or target.stride(-1) != 1:
        raise _lib.PafcError("logp_gather_rows: target is (rows) int32 on the GPU")
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=logits.device)
    elif not out.is_cuda or out.dtype != torch.float32 or out.numel() != rows or out.stride(-1) != 1:
        raise _lib.PafcError("logp_gather_rows: out is (rows) float32 on the GPU")
    if rows == 0:
        return out
    rc = _lib.lib().pafc_logp_gather_rows(_lib.dtype_code(logits.dtype), rows, V, _lib.ptr(logits), logits.stride(0),
                                          _lib.ptr(target), _lib.ptr(out), _lib.stream_of(logits))
    _lib.check(rc, "pafc_logp_gather_rows")
    return out


# ---- the attention decoder's loss on packed rows (include/pafc_attention.h, csrc/mha_rows_bwd.hip) ---------------------------
def _mha_rows_operands(who: str, q, k, v, q_off, kv_off, kv_len, heads: int) -> int:
    d = heads * 64
    for t in (q, k, v):
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != q.dtype or t.shape[1] < d:
            raise _lib.PafcError(f"{who}: q, k, v are 2-D GPU tensors of one dtype, unit stride along the heads")
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.PafcError(f"{who}: fp32 or bf16 operands")
    if k.stride(0) != v.stride(0) or k.shape[0] != v.shape[0]:
        raise _lib.PafcError(f"{who}: k and v must share their rows and their row pitch")
    for t in (q_off, kv_off, kv_len):
        if not t.is_cuda or t.dtype != torch.int32 or t.stride(-1) != 1:
            raise _lib.PafcError(f"{who}: q_off, kv_off, kv_len are int32 GPU tensors")
    G = kv_len.numel()
    if q_off.numel() != G + 1 or kv_off.numel() != G:
        raise _lib.PafcError(f"{who}: q_off (G + 1), kv_off (G), kv_len (G)")
    return G


def mha_rows_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_off: torch.Tensor, kv_off: torch.Tensor,
                 kv_len: torch.Tensor, heads: int, causal: bool):
    """mha_rows that also returns lse (rows, H) float32, the log of every row's softmax denominator per head
    (pafc_mha_rows_lse): -> (out (rows, H * 64) with the bits of mha_rows, lse).  Rows outside every group: out undefined,
    lse -inf."""
    G = _mha_rows_operands("mha_rows_lse", q, k, v, q_off, kv_off, kv_len, heads)
    out = torch.empty(q.shape[0], heads * 64, dtype=q.dtype, device=q.device)
    lse = torch.full((q.shape[0], heads), float("-inf"), dtype=torch.float32, device=q.device)
    if G == 0 or q.shape[0] == 0:
        return out, lse
    rc = _lib.lib().pafc_mha_rows_lse(_lib.dtype_code(q.dtype), G, heads, 64, _lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v),
                                      k.stride(0), _lib.ptr(q_off), _lib.ptr(kv_off), _lib.ptr(kv_len), int(bool(causal)),
                                      _lib.ptr(out), out.stride(0), _lib.ptr(lse), _lib.stream_of(q))
    _lib.check(rc, "pafc_mha_rows_lse")
    return out, lse


def mha_rows_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor,
                 q_off: torch.Tensor, kv_off: torch.Tensor, kv_len: torch.Tensor, heads: int, causal: bool,
                 dq: Optional[torch.Tensor] = None, dk: Optional[torch.Tensor] = None, dv: Optional[torch.Tensor] = None):
    """(dq, dk, dv) of mha_rows from its operands, the out / lse of mha_rows_lse and the upstream gradient dout
    (pafc_mha_rows_bwd; no atomics, two runs give the same bits).  PRECONDITION: the key ranges of two groups that both have
    query rows do not overlap.  dq (rows, >= H * 64), dk / dv (kv rows, >= H * 64, one row pitch) may be handed in, column
    slices of stacked buffers included; THIS wrapper zeroes them first (the kernels write owned rows only), so rows outside
    every group's range come back zero."""
    G = _mha_rows_operands("mha_rows_bwd", q, k, v, q_off, kv_off, kv_len, heads)
    d, rows = heads * 64, q.shape[0]
    for t in (out, dout):
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != q.dtype or t.shape[0] != rows or t.shape[1] < d:
            raise _lib.PafcError("mha_rows_bwd: out and dout are (rows, >= H * 64) in the operands' dtype")
    if not lse.is_cuda or lse.dtype != torch.float32 or lse.shape != (rows, heads) or not lse.is_contiguous():
        raise _lib.PafcError("mha_rows_bwd: lse is (rows, H) float32, contiguous")
    if dq is None:
        dq = torch.zeros(rows, d, dtype=q.dtype, device=q.device)
    else:
        dq.zero_()
    if dk is None or dv is None:
        dkv = torch.zeros(k.shape[0], 2 * d, dtype=q.dtype, device=q.device)
        dk, dv = dkv[:, :d], dkv[:, d:]
    else:
        dk.zero_()
        dv.zero_()
    if (not dq.is_cuda or dq.dtype != q.dtype or dq.dim() != 2 or dq.stride(1) != 1 or dq.shape[0] != rows or dq.shape[1] < d):
        raise _lib.PafcError("mha_rows_bwd: dq is (rows, >= H * 64) in the operands' dtype")
    for t in (dk, dv):
        if (not t.is_cuda or t.dtype != q.dtype or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != k.shape[0] or t.shape[1] < d
                or t.stride(0) != dk.stride(0)):
            raise _lib.PafcError("mha_rows_bwd: dk, dv are (kv rows, >= H * 64) in the operands' dtype with one row pitch")
    if G == 0 or rows == 0:
        return dq, dk, dv
    L = _lib.lib()
    nbytes = L.pafc_mha_rows_bwd_workspace_bytes(rows, heads)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    rc = L.pafc_mha_rows_bwd(_lib.dtype_code(q.dtype), G, heads, 64, rows, _lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v),
                             k.stride(0), _lib.ptr(out), out.stride(0), _lib.ptr(dout), dout.stride(0), _lib.ptr(lse),
                             _lib.ptr(q_off), _lib.ptr(kv_off), _lib.ptr(kv_len), int(bool(causal)), _lib.ptr(dq), dq.stride(0),
                             _lib.ptr(dk), _lib.ptr(dv), dk.stride(0), _lib.ptr(ws), nbytes, _lib.stream_of(q))
    _lib.check(rc, "pafc_mha_rows_bwd")
    return dq, dk, dv


class _MhaRowsTrain(torch.autograd.Function):
    """mha_rows under autograd: pafc_mha_rows_lse forward, pafc_mha_rows_bwd backward.  When q, k and v are the column thirds
    of one stacked projection (self-attention) the three gradients are the thirds of one buffer, k | v halves likewise."""

    @staticmethod
    def forward(ctx, q, k, v, q_off, kv_off, kv_len, heads, causal):
        out, lse = mha_rows_lse(q, k, v, q_off, kv_off, kv_len, heads, causal)
        ctx.save_for_backward(q, k, v, out, lse, q_off, kv_off, kv_len)
        ctx.heads, ctx.causal = heads, bool(causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, q_off, kv_off, kv_len = ctx.saved_tensors
        d = ctx.heads * 64
        if dout.dtype != q.dtype:
            dout = dout.to(q.dtype)
        if dout.stride(1) != 1 or (dout.stride(0) * dout.element_size()) % 16 or dout.data_ptr() % 16:
            dout = dout.contiguous()
        dq = dk = dv = None
        if q.shape[0] == k.shape[0]:                       # one buffer for the three: the stacked projection's gradient
            buf = torch.zeros(q.shape[0], 3 * d, dtype=q.dtype, device=q.device)
            dq, dk, dv = buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:]
        dq, dk, dv = mha_rows_bwd(q, k, v, out, dout, lse, q_off, kv_off, kv_len, ctx.heads, ctx.causal, dq, dk, dv)
        return dq, dk, dv, None, None, None, None, None


def mha_rows_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_off: torch.Tensor, kv_off: torch.Tensor,
                   kv_len: torch.Tensor, heads: int, causal: bool) -> torch.Tensor:
    """mha_rows with gradients for q, k and v (which may be slices of one stacked projection).  The key ranges of two groups
    with query rows must not overlap (mha_rows_bwd)."""
    return _MhaRowsTrain.apply(q, k, v, q_off, kv_off, kv_len, heads, causal)


# ---- training the Conformer baseline's slot (include/pafc_attention.h, csrc/mha_band_bwd.hip) --------------------------------
def _mha_band_operands(who: str, q, k, v, p, pos_bias_u, pos_bias_v, batch: int, heads: int, w: int, t_pad):
    """The argument checks of mha_band for the training pair; -> (T, t_pad)."""
    d = heads * 64
    for name, t in (("q", q), ("k", k), ("v", v), ("p", p)):
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != q.dtype or t.shape[1] < d:
            raise _lib.PafcError(f"{who}: {name} is a 2-D GPU tensor of q's dtype with at least H * 64 columns and unit stride "
                                 f"along them")
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.PafcError(f"{who}: fp32 or bf16 operands, got {q.dtype}")
    if batch < 1 or heads < 1 or q.shape[0] % batch:
        raise _lib.PafcError(f"{who}: q has {q.shape[0]} rows, not a multiple of batch = {batch}")
    T = q.shape[0] // batch
    if T < 1 or k.shape[0] != q.shape[0] or v.shape[0] != q.shape[0] or p.shape[0] != T:
        raise _lib.PafcError(f"{who}: q, k, v hold batch * T rows and p holds T = {T} rows "
                             f"(k {k.shape[0]}, v {v.shape[0]}, p {p.shape[0]})")
    if k.stride(0) != v.stride(0):
        raise _lib.PafcError(f"{who}: k and v must share their row pitch")
    if w < 0:
        raise _lib.PafcError(f"{who}: w = {w} is negative")
    if t_pad is None:
        t_pad = -(-T // (2 * w)) * 2 * w if w > 0 else T
    if t_pad < T:
        raise _lib.PafcError(f"{who}: t_pad = {t_pad} is below T = {T}")
    per16 = 16 // q.element_size()
    for name, t in (("q", q), ("k", k), ("v", v), ("p", p)):
        if t.stride(0) % per16 or t.data_ptr() % 16:
            raise _lib.PafcError(f"{who}: {name} needs a 16-byte aligned base and a row pitch that is a multiple of 16 bytes")
    for name, t in (("pos_bias_u", pos_bias_u), ("pos_bias_v", pos_bias_v)):
        if not t.is_cuda or t.dtype != q.dtype or tuple(t.shape) != (heads, 64) or not t.is_contiguous() or t.data_ptr() % 16:
            raise _lib.PafcError(f"{who}: {name} is a contiguous, 16-byte aligned (H, 64) GPU tensor of q's dtype")
    return T, int(t_pad)


def _mha_band_rows(who: str, name: str, t, like, rows: int, d: int):
    per16 = 16 // like.element_size()
    if (not t.is_cuda or t.dtype != like.dtype or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != rows or t.shape[1] < d
            or t.stride(0) % per16 or t.data_ptr() % 16):
        raise _lib.PafcError(f"{who}: {name} is ({rows}, >= H * 64) in the operands' dtype, unit stride along the heads, 16-byte "
                             f"aligned rows")


def mha_band_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, p: torch.Tensor, pos_bias_u: torch.Tensor,
                 pos_bias_v: torch.Tensor, batch: int, heads: int, w: int, t_pad: Optional[int] = None):
    """mha_band that also returns lse (batch * T, H) float32, the log of every query's softmax denominator per head with the
    padding keys' term in it (pafc_mha_band_lse): -> (out with the bits of mha_band, lse)."""
    T, t_pad = _mha_band_operands("mha_band_lse", q, k, v, p, pos_bias_u, pos_bias_v, batch, heads, w, t_pad)
    out = torch.empty(q.shape[0], heads * 64, dtype=q.dtype, device=q.device)
    lse = torch.empty(q.shape[0], heads, dtype=torch.float32, device=q.device)
    rc = _lib.lib().pafc_mha_band_lse(_lib.dtype_code(q.dtype), batch, T, heads, 64, int(w), t_pad, _lib.ptr(q), q.stride(0),
                                      _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(p), p.stride(0), _lib.ptr(pos_bias_u),
                                      _lib.ptr(pos_bias_v), _lib.ptr(out), out.stride(0), _lib.ptr(lse), _lib.stream_of(q))
    _lib.check(rc, "pafc_mha_band_lse")
    return out, lse


def mha_band_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, p: torch.Tensor, pos_bias_u: torch.Tensor,
                 pos_bias_v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, batch: int, heads: int,
                 w: int, t_pad: Optional[int] = None, dq: Optional[torch.Tensor] = None, dk: Optional[torch.Tensor] = None,
                 dv: Optional[torch.Tensor] = None, dp: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None):
    """(dq, dk, dv, dp, du, dvb) of mha_band from its operands, the out / lse of mha_band_lse and the upstream gradient dout
    (pafc_mha_band_bwd: three launches, no atomics, two runs give the same bits).  dq, dk, dv (batch * T, >= H * 64; dk and dv
    with one row pitch) and dp (T, >= H * 64) may be handed in, column slices of stacked buffers included; every row of them is
    written.  du, dvb: (H, 64) float32, the sums over every row of the batch.  workspace: a uint8 GPU tensor of at least
    pafc_mha_band_bwd_workspace_bytes bytes, allocated here when None."""
    T, t_pad = _mha_band_operands("mha_band_bwd", q, k, v, p, pos_bias_u, pos_bias_v, batch, heads, w, t_pad)
    d, rows = heads * 64, q.shape[0]
    _mha_band_rows("mha_band_bwd", "out", out, q, rows, d)
    _mha_band_rows("mha_band_bwd", "dout", dout, q, rows, d)
    if not lse.is_cuda or lse.dtype != torch.float32 or tuple(lse.shape) != (rows, heads) or not lse.is_contiguous():
        raise _lib.PafcError("mha_band_bwd: lse is (batch * T, H) float32, contiguous")
    if dq is None:
        dq = torch.empty(rows, d, dtype=q.dtype, device=q.device)
    if dk is None or dv is None:
        dkv = torch.empty(rows, 2 * d, dtype=q.dtype, device=q.device)
        dk, dv = dkv[:, :d], dkv[:, d:]
    if dp is None:
        dp = torch.empty(T, d, dtype=q.dtype, device=q.device)
    for name, t, n in (("dq", dq, rows), ("dk", dk, rows), ("dv", dv, rows), ("dp", dp, T)):
        _mha_band_rows("mha_band_bwd", name, t, q, n, d)
    if dk.stride(0) != dv.stride(0):
        raise _lib.PafcError("mha_band_bwd: dk and dv must share their row pitch")
    du = torch.empty(heads, 64, dtype=torch.float32, device=q.device)
    dvb = torch.empty(heads, 64, dtype=torch.float32, device=q.device)
    L = _lib.lib()
    nbytes = L.pafc_mha_band_bwd_workspace_bytes(batch, T, heads)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise _lib.PafcError("mha_band_bwd: workspace is a contiguous uint8 GPU tensor")
    from .profiling import op_timer
    # 896 flop per (query, key) pair and pass: a 128-deep score, a 64-deep dP and two or three 64-wide products
    with op_timer("mha_band_bwd_w%d" % w, sample=12, flops=1792.0 * batch * heads * T * min(T, 2 * w + 1)):
        rc = L.pafc_mha_band_bwd(_lib.dtype_code(q.dtype), batch, T, heads, 64, int(w), t_pad, _lib.ptr(q), q.stride(0),
                                 _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(p), p.stride(0), _lib.ptr(pos_bias_u),
                                 _lib.ptr(pos_bias_v), _lib.ptr(out), out.stride(0), _lib.ptr(dout), dout.stride(0),
                                 _lib.ptr(lse), _lib.ptr(dq), dq.stride(0), _lib.ptr(dk), _lib.ptr(dv), dk.stride(0),
                                 _lib.ptr(dp), dp.stride(0), _lib.ptr(du), _lib.ptr(dvb), _lib.ptr(workspace),
                                 workspace.numel(), _lib.stream_of(q))
    _lib.check(rc, "pafc_mha_band_bwd")
    return dq, dk, dv, dp, du, dvb


def _thirds_of_one_buffer(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d: int) -> bool:
    """Are q, k, v the column thirds [Q | K | V] of one (rows, 3 d) buffer?"""
    es = q.element_size()
    return (q.shape[1] == d and k.shape[1] == d and v.shape[1] == d and q.stride(0) == 3 * d and k.stride(0) == 3 * d
            and v.stride(0) == 3 * d and k.data_ptr() == q.data_ptr() + d * es and v.data_ptr() == q.data_ptr() + 2 * d * es)


class _MhaBandTrain(torch.autograd.Function):
    """mha_band under autograd: pafc_mha_band_lse forward, pafc_mha_band_bwd backward.  When q, k and v are the column thirds of
    one stacked projection the three gradients are the thirds of one (rows, 3 D) buffer, as _MhaRowsTrain's are (q, k, v arrive
    as three slice views, so autograd still adds three zero-padded thirds before the QKV GEMM's backward).  The biases may be fp32 parameters under a bf16 kernel (autocast): they are cast as _param_as does
    and their gradients come back in their own dtype."""

    @staticmethod
    def forward(ctx, q, k, v, p, pos_bias_u, pos_bias_v, batch, heads, w, t_pad):
        u, vb = _param_as(pos_bias_u, q.dtype).contiguous(), _param_as(pos_bias_v, q.dtype).contiguous()
        out, lse = mha_band_lse(q, k, v, p, u, vb, batch, heads, w, t_pad)
        ctx.save_for_backward(q, k, v, p, u, vb, out, lse)
        ctx.cfg = (batch, heads, w, t_pad, pos_bias_u.dtype, pos_bias_v.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, p, u, vb, out, lse = ctx.saved_tensors
        batch, heads, w, t_pad, u_dtype, vb_dtype = ctx.cfg
        d = heads * 64
        if dout.dtype != q.dtype:
            dout = dout.to(q.dtype)
        if dout.stride(1) != 1 or (dout.stride(0) * dout.element_size()) % 16 or dout.data_ptr() % 16:
            dout = dout.contiguous()
        dq = dk = dv = None
        stacked = _thirds_of_one_buffer(q, k, v, d)
        if stacked:                                        # one buffer for the three: the stacked projection's gradient
            buf = torch.empty(q.shape[0], 3 * d, dtype=q.dtype, device=q.device)
            dq, dk, dv = buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:]
        dq, dk, dv, dp, du, dvb = mha_band_bwd(q, k, v, p, u, vb, out, dout, lse, batch, heads, w, t_pad, dq, dk, dv)
        if not stacked:                                    # gradients of the inputs' shapes (wider inputs: zero beyond H * 64)
            dq, dk, dv, dp = (_grad_like(g, t, d) for g, t in ((dq, q), (dk, k), (dv, v), (dp, p)))
        else:
            dp = _grad_like(dp, p, d)
        return dq, dk, dv, dp, du.to(u_dtype), dvb.to(vb_dtype), None, None, None, None


def _grad_like(g: torch.Tensor, t: torch.Tensor, d: int) -> torch.Tensor:
    if t.shape[1] == d:
        return g
    full = torch.zeros(t.shape, dtype=g.dtype, device=g.device)
    full[:, :d] = g
    return full


def mha_band_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, p: torch.Tensor, pos_bias_u: torch.Tensor,
                   pos_bias_v: torch.Tensor, batch: int, heads: int, w: int, t_pad: Optional[int] = None) -> torch.Tensor:
    """mha_band with gradients for q, k, v, p and the two biases (q, k, v may be slices of one stacked projection; the biases
    may be fp32 parameters of a bf16 call)."""
    return _MhaBandTrain.apply(q, k, v, p, pos_bias_u, pos_bias_v, batch, heads, w, t_pad)


def _lsm_operands(who: str, logits: torch.Tensor, target: torch.Tensor):
    if not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1 or logits.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.PafcError(f"{who}: logits are a 2-D fp32 / bf16 GPU tensor with unit stride along the vocabulary")
    if not target.is_cuda or target.dtype != torch.int32 or target.numel() != logits.shape[0] or target.stride(-1) != 1:
        raise _lib.PafcError(f"{who}: target is (rows) int32 on the GPU")


def lsm_loss_rows(logits: torch.Tensor, target: torch.Tensor, smoothing: float):
    """Per row of (rows, V) logits: the label-smoothing loss against target (int32; -1 is ignored), lse = logsumexp and
    correct = (argmax == target) (pafc_lsm_loss_rows) -> (loss, lse float32 (rows), correct int32 (rows))."""
    _lsm_operands("lsm_loss_rows", logits, target)
    rows, V = logits.shape
    loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    correct = torch.empty(rows, dtype=torch.int32, device=logits.device)
    if rows:
        rc = _lib.lib().pafc_lsm_loss_rows(_lib.dtype_code(logits.dtype), rows, V, _lib.ptr(logits), logits.stride(0),
                                           _lib.ptr(target), float(smoothing), _lib.ptr(loss), _lib.ptr(lse), _lib.ptr(correct),
                                           _lib.stream_of(logits))
        _lib.check(rc, "pafc_lsm_loss_rows")
    return loss, lse, correct


def lsm_loss_rows_bwd(logits: torch.Tensor, target: torch.Tensor, smoothing: float, lse: torch.Tensor, g: torch.Tensor,
                      out: Optional[torch.Tensor] = None, pad_to: Optional[int] = None) -> torch.Tensor:
    """g * d(sum of lsm_loss_rows' losses) / dlogits in the logits' dtype (pafc_lsm_loss_rows_bwd); g one float32 on the device.
    out: where to write ((rows, V) view of rows with pitch pad_to, default a fresh buffer; may be `logits`); the columns from V
    to pad_to of every row are zeroed.  Returns the (rows, V) view."""
    _lsm_operands("lsm_loss_rows_bwd", logits, target)
    rows, V = logits.shape
    if out is None:
        width = pad_to or V
        out = torch.empty(rows, width, dtype=logits.dtype, device=logits.device)[:, :V]
    if (not out.is_cuda or out.dtype != logits.dtype or out.shape != logits.shape or out.stride(1) != 1
            or out.stride(0) < (pad_to or V)):
        raise _lib.PafcError("lsm_loss_rows_bwd: out is (rows, V) in the logits' dtype with a row pitch of at least pad_to")
    if (not lse.is_cuda or lse.dtype != torch.float32 or lse.numel() != rows or not g.is_cuda or g.dtype != torch.float32
            or g.numel() != 1):
        raise _lib.PafcError("lsm_loss_rows_bwd: lse (rows) and g (1) are float32 on the GPU")
    if rows:
        rc = _lib.lib().pafc_lsm_loss_rows_bwd(_lib.dtype_code(logits.dtype), rows, V, _lib.ptr(logits), logits.stride(0),
                                               _lib.ptr(target), float(smoothing), _lib.ptr(lse), _lib.ptr(g), _lib.ptr(out),
                                               pad_to or V, _lib.stream_of(logits))
        _lib.check(rc, "pafc_lsm_loss_rows_bwd")
    return out


class _AttHeadLoss(torch.autograd.Function):
    """output_layer + label-smoothing loss of the attention decoder on hand-written kernels only, in the manner of
    _CtcHeadLoss: logits = x W^T + b as bf16 rows padded to a multiple of 64 columns (pafc_gemm_bf16), loss / lse / correct per
    row from the logits (pafc_lsm_loss_rows), and backwards the gradient written over the logits (pafc_lsm_loss_rows_bwd),
    dX = dlogits W on pafc_gemm_bf16 against the zero-padded W^T, dW / db through gemm_tn.  The (rows, V) log-softmax never
    exists.  A vocabulary that is no multiple of 8 runs the three products over the padded width (zero weight rows)."""

    @staticmethod
    def forward(ctx, x, weight, bias, target, smoothing, denom):
        M, C = x.shape
        V = weight.shape[0]
        Vp = (V + 63) // 64 * 64
        xb = x.to(torch.bfloat16)
        if xb.stride(1) != 1 or xb.stride(0) % 8 or xb.data_ptr() % 16:
            xb = xb.contiguous()
        wb = _bf16_shadow(weight).detach()
        bb = None if bias is None else _bf16_shadow(bias).detach()
        padded = V % 8 != 0
        if padded:
            wp = torch.zeros((Vp, C), dtype=torch.bfloat16, device=x.device)
            wp[:V].copy_(wb)
            wb = wp
            if bb is not None:
                bp = torch.zeros(Vp, dtype=torch.bfloat16, device=x.device)
                bp[:V].copy_(bb)
                bb = bp
        logits = torch.empty((M, Vp), dtype=torch.bfloat16, device=x.device)
        gemm_bf16(xb, wb, bb, out=logits if padded else logits[:, :V])
        loss, lse, correct = lsm_loss_rows(logits[:, :V], target, smoothing)
        ctx.save_for_backward(xb, wb, logits, lse, target, denom)
        ctx.dims = (M, C, V, Vp, float(smoothing), padded)
        ctx.w_dtype, ctx.b_dtype, ctx.x_dtype = weight.dtype, None if bias is None else bias.dtype, x.dtype
        n_correct = correct.sum()
        ctx.mark_non_differentiable(n_correct)
        return loss.sum() / denom, n_correct

    @staticmethod
    def backward(ctx, g, _gcorrect):
        xb, wb, logits, lse, target, denom = ctx.saved_tensors
        M, C, V, Vp, smoothing, padded = ctx.dims
        if getattr(ctx, "spent", False):
            raise _lib.PafcError("att_head_loss: a second backward pass through one forward (the gradient was written over the logits)")
        ctx.spent = True
        gf = (g.detach().to(torch.float32) / denom).reshape(1).contiguous()
        lsm_loss_rows_bwd(logits[:, :V], target, smoothing, lse, gf, out=logits[:, :V], pad_to=Vp)
        dl = logits                                                                 # written in place, (M, Vp) with its zero padding
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wt = torch.zeros((C, Vp), dtype=torch.bfloat16, device=xb.device)       # W^T, zero beyond V: K = Vp is a multiple of 64
            wt[:, :V].copy_(wb[:V].t())
            dx = gemm_bf16(dl, wt).to(ctx.x_dtype)
        want_b = ctx.b_dtype is not None and ctx.needs_input_grad[2]
        dlv = dl if padded else dl[:, :V]
        if ctx.needs_input_grad[1]:
            od = ctx.w_dtype if ctx.w_dtype in (torch.float32, torch.bfloat16) else torch.float32
            if want_b:
                dw, db = gemm_tn(dlv, xb, od, want_bias=True)
                db = db[:V].to(ctx.b_dtype)
            else:
                dw = gemm_tn(dlv, xb, od)
            dw = dw[:V].to(ctx.w_dtype)
        elif want_b:
            db = dl[:, :V].sum(0, dtype=torch.float32).to(ctx.b_dtype)
        return dx, dw, db, None, None, None


def att_head_loss(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], target: torch.Tensor, smoothing: float,
                  denom: torch.Tensor):
    """(sum_r lsm_loss(x_r W^T + b, target_r) / denom, number of rows whose argmax is their target): see _AttHeadLoss.  x (rows,
    C) with C % 64 == 0, target (rows) int32 on the GPU (-1: ignored), denom a float32 scalar tensor on the GPU (the batch size
    or the number of scored tokens).  One backward pass per forward: the gradient is written over the saved logits."""
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or x.shape[1] % 64:
        raise _lib.PafcError("att_head_loss: x (rows, C) against weight (V, C), C a multiple of 64")
    if not denom.is_cuda or denom.dtype != torch.float32 or denom.numel() != 1:
        raise _lib.PafcError("att_head_loss: denom is one float32 on the GPU")
    return _AttHeadLoss.apply(x, weight, bias, target, float(smoothing), denom.reshape(()))


# ---- the attention decoder's beam search (include/pafc_attn_search.h, csrc/attn_search.hip) ----------------------------------
def _i32_gpu(who: str, **tensors) -> None:
    for name, t in tensors.items():
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
            raise _lib.PafcError(f"{who}: {name} is a contiguous int32 GPU tensor")


def mha_step(qkv: torch.Tensor, cache: torch.Tensor, anc: torch.Tensor, pos: torch.Tensor, done: torch.Tensor, beam: int,
             heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Single-query self-attention of the R new rows of a beam-search step through the ancestor table (pafc_mha_step).
    qkv (R, >= 3 * H * 64) the stacked q | k | v projection of the new rows, fp32 or bf16, unit stride along the columns;
    cache (P, R, 2 * H * 64) contiguous in qkv's dtype: the launch stores the rows' k | v at position pos[0] and attends over
    the positions [0, pos[0]]; anc (2, R, P), pos (1), done (1) int32 on the device.  With done set or pos outside [0, P)
    nothing is written.  Returns out (R, H * 64)."""
    d = heads * 64
    if not qkv.is_cuda or qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] < 3 * d:
        raise _lib.PafcError("mha_step: qkv is a 2-D GPU tensor of at least 3 * H * 64 columns with unit stride along them")
    R = qkv.shape[0]
    if not cache.is_cuda or cache.dtype != qkv.dtype or cache.dim() != 3 or not cache.is_contiguous() \
            or cache.shape[1:] != (R, 2 * d) or cache.shape[0] < 1:
        raise _lib.PafcError("mha_step: cache is (P, R, 2 * H * 64), contiguous, in qkv's dtype")
    P = cache.shape[0]
    _i32_gpu("mha_step", anc=anc, pos=pos, done=done)
    if anc.shape != (2, R, P) or pos.numel() != 1 or done.numel() != 1:
        raise _lib.PafcError("mha_step: anc is (2, R, P), pos and done hold one int32 each")
    if not 1 <= beam <= 16 or R % beam:
        raise _lib.PafcError(f"mha_step: a beam of {beam} for {R} rows (1..16, dividing the rows)")
    if out is None:
        out = torch.empty(R, d, dtype=qkv.dtype, device=qkv.device)
    elif not out.is_cuda or out.dtype != qkv.dtype or out.dim() != 2 or out.stride(1) != 1 or out.shape != (R, d):
        raise _lib.PafcError("mha_step: out is (R, H * 64) in qkv's dtype")
    rc = _lib.lib().pafc_mha_step(_lib.dtype_code(qkv.dtype), R, beam, heads, 64, P, _lib.ptr(qkv), qkv.stride(0), _lib.ptr(cache),
                                  _lib.ptr(anc), _lib.ptr(pos), _lib.ptr(done), _lib.ptr(out), out.stride(0), _lib.stream_of(qkv))
    _lib.check(rc, "pafc_mha_step")
    return out


def attn_beam_select_workspace(B: int, beam: int, device) -> torch.Tensor:
    nbytes = _lib.lib().pafc_attn_beam_select_workspace_bytes(B, beam)
    if nbytes == 0:
        raise _lib.PafcError(f"attn_beam_select: {B} utterances with a beam of {beam} (the beam is 1..16)")
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def attn_beam_select(logits: torch.Tensor, beam: int, eos: int, cap: int, score: torch.Tensor, ended: torch.Tensor,
                     token: torch.Tensor, anc: torch.Tensor, trace_parent: torch.Tensor, trace_token: torch.Tensor,
                     trace_score: torch.Tensor, pos: torch.Tensor, done: torch.Tensor,
                     workspace: Optional[torch.Tensor] = None) -> None:
    """One beam-search step's selection straight from the (R, V) logits (pafc_attn_beam_select): per row the logsumexp and
    the `beam` largest logits (an ended row: the single candidate (eos, 0)), per utterance the `beam` best of its beam * beam
    candidates by score[parent] + logp; writes score / ended / token (R), the trace row pos[0] of trace_parent / trace_token /
    trace_score (P, R), the other half of anc (2, R, P), done and pos += 1, all in place.  Frozen (nothing written) when done
    is set or pos[0] >= cap."""
    if not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1:
        raise _lib.PafcError("attn_beam_select: logits are a 2-D GPU tensor with unit stride along the vocabulary")
    R, V = logits.shape
    if not 1 <= beam <= 16 or R % beam or R == 0:
        raise _lib.PafcError(f"attn_beam_select: a beam of {beam} for {R} rows (1..16, dividing the rows)")
    if V < beam:
        raise _lib.PafcError(f"attn_beam_select: a vocabulary of {V} for a beam of {beam}")
    _i32_gpu("attn_beam_select", ended=ended, token=token, anc=anc, trace_parent=trace_parent, trace_token=trace_token, pos=pos,
             done=done)
    for name, t in (("score", score), ("trace_score", trace_score)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.PafcError(f"attn_beam_select: {name} is a contiguous float32 GPU tensor")
    P = trace_parent.shape[0] if trace_parent.dim() == 2 else 0
    if score.numel() != R or ended.numel() != R or token.numel() != R or anc.shape != (2, R, P) or pos.numel() != 1 \
            or done.numel() != 1 or any(t.shape != (P, R) for t in (trace_parent, trace_token, trace_score)):
        raise _lib.PafcError("attn_beam_select: score / ended / token (R), anc (2, R, P), the traces (P, R), pos and done (1)")
    if not 1 <= cap < P:
        raise _lib.PafcError(f"attn_beam_select: a cap of {cap} steps for tables of {P} positions (1 <= cap < P)")
    B = R // beam
    if workspace is None:
        workspace = attn_beam_select_workspace(B, beam, logits.device)
    elif not workspace.is_cuda or not workspace.is_contiguous():
        raise _lib.PafcError("attn_beam_select: the workspace is a contiguous GPU tensor")
    rc = _lib.lib().pafc_attn_beam_select(_lib.dtype_code(logits.dtype), B, beam, V, P, cap, eos, _lib.ptr(logits),
                                          logits.stride(0), _lib.ptr(score), _lib.ptr(ended), _lib.ptr(token), _lib.ptr(anc),
                                          _lib.ptr(trace_parent), _lib.ptr(trace_token), _lib.ptr(trace_score), _lib.ptr(pos),
                                          _lib.ptr(done), _lib.ptr(workspace), workspace.numel() * workspace.element_size(),
                                          _lib.stream_of(logits))
    _lib.check(rc, "pafc_attn_beam_select")


# ---- joint CTC/attention decoding (include/pafc_joint_search.h, csrc/joint_search.hip) -------------------------------------
def mha_step_paths(qkv: torch.Tensor, cache: torch.Tensor, path: torch.Tensor, length: torch.Tensor, new_row: torch.Tensor,
                   need: torch.Tensor, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Single-query self-attention of R rows at different positions through per-row tables of cache rows
    (pafc_mha_step_paths).  qkv (R, >= 3 * H * 64) the stacked q | k | v projection, fp32 or bf16, unit stride along the columns;
    cache (rows, 2 * H * 64) contiguous in qkv's dtype; path (R, W) int32: row r of length[r] attends over the cache rows
    path[r, 0 .. length[r] - 2] and its own k, v, and stores its k | v into cache row new_row[r] iff need[r].  A row with
    need == 0 writes nothing to the cache; its out row is computed all the same and is meant to be discarded.  Table entries
    outside the cache are clamped into it.  Returns out (R, H * 64)."""
    d = heads * 64
    if not qkv.is_cuda or qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] < 3 * d:
        raise _lib.PafcError("mha_step_paths: qkv is a 2-D GPU tensor of at least 3 * H * 64 columns with unit stride along them")
    R = qkv.shape[0]
    if not cache.is_cuda or cache.dtype != qkv.dtype or cache.dim() != 2 or not cache.is_contiguous() or cache.shape[1] != 2 * d \
            or cache.shape[0] < 1:
        raise _lib.PafcError("mha_step_paths: cache is (rows, 2 * H * 64), contiguous, in qkv's dtype")
    _i32_gpu("mha_step_paths", path=path, length=length, new_row=new_row, need=need)
    if path.dim() != 2 or path.shape[0] != R or path.shape[1] < 1 or length.numel() != R or new_row.numel() != R \
            or need.numel() != R:
        raise _lib.PafcError("mha_step_paths: path is (R, W), length / new_row / need hold R int32 each")
    if out is None:
        out = torch.empty(R, d, dtype=qkv.dtype, device=qkv.device)
    elif not out.is_cuda or out.dtype != qkv.dtype or out.dim() != 2 or out.stride(1) != 1 or out.shape != (R, d):
        raise _lib.PafcError("mha_step_paths: out is (R, H * 64) in qkv's dtype")
    rc = _lib.lib().pafc_mha_step_paths(_lib.dtype_code(qkv.dtype), R, heads, 64, cache.shape[0], path.shape[1], _lib.ptr(qkv),
                                        qkv.stride(0), _lib.ptr(cache), _lib.ptr(path), path.stride(0), _lib.ptr(length),
                                        _lib.ptr(new_row), _lib.ptr(need), _lib.ptr(out), out.stride(0), _lib.stream_of(qkv))
    _lib.check(rc, "pafc_mha_step_paths")
    return out


class _JointStateStruct(ctypes.Structure):
    """pafc_joint_state of include/pafc_joint_search.h, field for field."""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "N", "C", "T", "M", "HS")] + [(n, ctypes.c_void_p) for n in (
        "parent", "token", "length", "start", "end", "snap_end", "ctc_conf", "snap_ctc_conf", "att_conf", "att_sum", "lse", "row",
        "p_nb", "p_b", "stamp", "hash_key", "hash_node", "n_nodes", "executed", "nlive", "evals", "node", "need", "in_token",
        "in_pos", "in_len", "new_row", "row_of_slot", "store_row", "score", "path", "cand_tok", "cand_p", "p_blank", "skip",
        "trace_node", "trace_score", "trace_exec")]


class JointSearchState:
    """The device state of one joint_decoding call (pafc_joint_state): the tensors by name, in their initial values, and the
    struct that the kernels take.  B utterances, beam N, C candidates per frame, T frames; decode: whether the decoder runs
    (dec_w > 0: slot 0 of every utterance then asks for round 0's decode of [sos])."""

    def __init__(self, B: int, N: int, C: int, T: int, sos: int, device, decode: bool = True):
        if not (1 <= N <= 16 and 1 <= C <= 24 and B >= 1 and T >= 1):
            raise _lib.PafcError(f"joint search: {B} utterances, a beam of {N} (1..16), {C} candidates per frame (1..24), {T} frames")
        M = 1 + T * N * C
        HS = 1 << (2 * M - 1).bit_length()
        R = B * N
        if (T + 2) * R > 0x7fffffff:
            raise _lib.PafcError(f"joint search: {(T + 2) * R} cache rows do not fit an int32")
        self.B, self.N, self.C, self.T, self.M, self.HS, self.R = B, N, C, T, M, HS, R
        i32 = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=device)                 # noqa: E731
        f64 = lambda *shape, fill=0.0: torch.full(shape, fill, dtype=torch.float64, device=device)             # noqa: E731
        f32 = lambda *shape, fill=0.0: torch.full(shape, fill, dtype=torch.float32, device=device)             # noqa: E731
        inf = float("inf")
        t = self.t = dict(
            parent=i32(B, M, fill=-1), token=i32(B, M), length=i32(B, M), start=i32(B, M), end=i32(B, M), snap_end=i32(B, M),
            ctc_conf=f32(B, M, fill=-inf), snap_ctc_conf=f32(B, M, fill=-inf), att_conf=f64(B, M, fill=-inf), att_sum=f64(B, M),
            lse=f64(B, M, fill=float("nan")), row=i32(B, M, fill=-1), p_nb=f64(2, B, M, fill=-inf), p_b=f64(2, B, M, fill=-inf),
            stamp=i32(2, B, M, fill=-1), hash_key=torch.full((B, HS), -1, dtype=torch.int64, device=device), hash_node=i32(B, HS),
            n_nodes=i32(B, fill=1), executed=i32(B), nlive=i32(B, fill=1), evals=i32(B, fill=1 if decode else 0),
            node=i32(R, fill=-1), need=i32(R), in_token=i32(R), in_pos=i32(R), in_len=i32(R, fill=1), new_row=i32(R),
            row_of_slot=i32(R), store_row=i32(R, fill=(T + 1) * R), score=f64(R), path=i32(R, T + 1),
            cand_tok=i32(B, T, C, fill=-1), cand_p=f32(B, T, C, fill=-inf), p_blank=f32(B, T, fill=-inf), skip=i32(B, T),
            trace_node=i32(T, R, fill=-1), trace_score=f64(T, R), trace_exec=i32(T, B, fill=-1))
        # node 0 of every utterance is [sos], in the table of "frame 0" at (p_nb, p_b) = (-inf, 0); it sits in slot 0
        t["token"][:, 0].fill_(sos)
        t["length"][:, 0].fill_(1)
        t["p_b"][0, :, 0].fill_(0.0)
        t["stamp"][0, :, 0].fill_(0)
        first = lambda name: t[name].view(B, N)[:, 0]              # slot 0 of every utterance               # noqa: E731
        first("node").fill_(0)
        first("in_token").fill_(sos)
        if decode:
            rows = torch.arange(0, R, N, dtype=torch.int32, device=device)
            first("need").fill_(1)
            for name in ("new_row", "store_row", "row_of_slot"):
                first(name).copy_(rows)
            t["row"][:, 0].copy_(rows)
        self.struct = _JointStateStruct(B, N, C, T, M, HS, **{k: v.data_ptr() for k, v in t.items()})

    def __getattr__(self, name):
        try:
            return self.__dict__["t"][name]
        except KeyError:
            raise AttributeError(name) from None


def joint_candidates(state: JointSearchState, ctc: torch.Tensor, lens: torch.Tensor, blank: int, log_threshold: float) -> None:
    """The candidates of every frame into state.cand_tok / cand_p / p_blank / skip (pafc_joint_candidates): ctc (B, T, V) fp32
    or bf16 contiguous on the GPU, lens (B) int32 on the GPU."""
    _lib.require_gpu(ctc)
    _i32_gpu("joint_candidates", lens=lens)
    if ctc.dim() != 3 or ctc.shape[:2] != (state.B, state.T) or lens.numel() != state.B:
        raise _lib.PafcError(f"joint_candidates: ctc {tuple(ctc.shape)} / lens for a state of {state.B} x {state.T} frames")
    rc = _lib.lib().pafc_joint_candidates(_lib.dtype_code(ctc.dtype), state.B, state.T, ctc.shape[2], state.C, blank,
                                          log_threshold, _lib.ptr(ctc), _lib.ptr(lens), _lib.ptr(state.cand_tok),
                                          _lib.ptr(state.cand_p), _lib.ptr(state.p_blank), _lib.ptr(state.skip),
                                          _lib.stream_of(ctc))
    _lib.check(rc, "pafc_joint_candidates")


def joint_frame(state: JointSearchState, t: int, logits: Optional[torch.Tensor], V: int, lens: torch.Tensor, ctc_w: float,
                dec_w: float, bonus: float, blank: int) -> None:
    """Frame t of the search for every utterance (pafc_joint_frame): logits (R, >= V) fp32 or bf16 with unit stride along the
    vocabulary, row r the output_layer row of slot r's prefix (None with dec_w == 0); everything else is in `state`."""
    _i32_gpu("joint_frame", lens=lens)
    if logits is not None and (not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] != state.R
                               or logits.shape[1] < V):
        raise _lib.PafcError("joint_frame: logits are (R, >= V) on the GPU with unit stride along the vocabulary")
    if logits is None and dec_w > 0:
        raise _lib.PafcError("joint_frame: dec_w > 0 needs the logits")
    weights = (ctypes.c_double * 3)(ctc_w, dec_w, bonus)
    rc = _lib.lib().pafc_joint_frame(ctypes.byref(state.struct), t, _lib.dtype_code(logits.dtype) if logits is not None else 0, V,
                                     _lib.ptr(logits), logits.stride(0) if logits is not None else 0, _lib.ptr(lens), weights,
                                     blank, _lib.stream_of(lens))
    _lib.check(rc, "pafc_joint_frame")


def joint_collect(state: JointSearchState) -> dict:
    """The beams' hypotheses in compact form (pafc_joint_collect): dict(len (R), tok / start / end (R, T + 1) int32, ctc_conf
    (R, T + 1) float32, att_conf (R, T + 1) float64), on the device."""
    dev, R, W = state.node.device, state.R, state.T + 1
    out = dict(len=torch.zeros(R, dtype=torch.int32, device=dev), tok=torch.zeros(R, W, dtype=torch.int32, device=dev),
               start=torch.zeros(R, W, dtype=torch.int32, device=dev), end=torch.zeros(R, W, dtype=torch.int32, device=dev),
               ctc_conf=torch.zeros(R, W, dtype=torch.float32, device=dev),
               att_conf=torch.zeros(R, W, dtype=torch.float64, device=dev))
    rc = _lib.lib().pafc_joint_collect(ctypes.byref(state.struct), _lib.ptr(out["len"]), _lib.ptr(out["tok"]),
                                       _lib.ptr(out["start"]), _lib.ptr(out["end"]), _lib.ptr(out["ctc_conf"]),
                                       _lib.ptr(out["att_conf"]), _lib.stream_of(state.node))
    _lib.check(rc, "pafc_joint_collect")
    return out
