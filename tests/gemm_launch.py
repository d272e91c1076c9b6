"""The buffer layout the GEMM battery tests share (tests/test_gemm_ph_forms_gpu.py, tests/test_gemm_small_tiles_gpu.py,
tests/test_gemm_f32_f64_gpu.py, tests/test_gemm_tn_f64_gpu.py):
operands inside rows wider than the row with NaN in the padding, the output inside a sentinel-filled buffer with 64 guard rows
per batch entry, the lo plane of a planes output `lo_gap` columns behind the hi plane -- and the read-back that tells whether
anything outside the output was written.  The launches themselves go through the bound library (paper_accurate_fast_cheap_amd
._lib), one function per entry point."""
from types import SimpleNamespace

import torch

from tests import gemm_ref

SENTINEL = 7.0
ACT = {"none": 0, "silu": 1, "tanh": 2, "relu": 3, "glu": 4}
OUT = {"bf16": 0, "f32": 1, "planes": 2}
RES = {None: 0, "bf16": 1, "f32": 2}
ERR_BAD_DIMS, ERR_UNSUPPORTED, ERR_ALIGNMENT = -2, -7, -8


def padded(t, pad, fill=float("nan")):
    """t (..., rows, cols) inside rows `pad` elements wider; the padding holds NaN: a read of it shows in the result."""
    if not pad:
        return t.contiguous()
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + pad,), fill, dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf


def lay_out(form, ops, pad=0, lo_gap=0, inplace=False, min_ldo=0):
    """The buffers of one call: A, W (padded), bias, the residual (padded, or the output buffer itself when `inplace`), the
    sentinel-filled output (Z, M + 64, ldo), and the strides that describe them."""
    A, W, bias, res = ops["A"], ops["W"], ops.get("bias"), ops.get("residual")
    lay = SimpleNamespace()
    lay.batched = A.dim() == 3
    lay.Z = A.shape[0] if lay.batched else 1
    lay.M, lay.N = A.shape[-2], W.shape[-2]
    lay.K = W.shape[-1] // 3 if form.a_split else W.shape[-1]
    lay.No = lay.N // 2 if form.act == "glu" else lay.N
    lay.planes = form.out == "planes"
    lay.lo_off = lay.No + lo_gap if lay.planes else 0
    lay.ldo = max((lay.lo_off + lay.No if lay.planes else lay.No) + pad, min_ldo)
    lay.A, lay.W = padded(A, pad), padded(W, pad)
    lay.out = torch.full((lay.Z, lay.M + 64, lay.ldo), SENTINEL, dtype=torch.float32 if form.out == "f32" else torch.bfloat16,
                         device=A.device)
    if res is not None and inplace:
        lay.out[:, :lay.M, :lay.No] = res
        lay.R, lay.ldr, lay.sR = lay.out, lay.ldo, lay.out.stride(0)
    elif res is not None:
        lay.R = padded(res, pad)
        lay.ldr, lay.sR = lay.R.stride(-2), (lay.R.stride(0) if lay.batched else 0)
    else:
        lay.R, lay.ldr, lay.sR = None, 0, 0
    lay.bias = bias.contiguous() if bias is not None else None
    lay.sBias = lay.bias.stride(0) if (lay.bias is not None and lay.bias.dim() == 2) else 0
    lay.sA, lay.sW = (lay.A.stride(0), lay.W.stride(0)) if lay.batched else (0, 0)
    lay.res_kind = RES[form.res] if res is not None else 0
    return lay


def read_back(lay):
    """-> (result as float64 (..., M, No), True if every element outside the output kept the sentinel)"""
    out, M, No = lay.out, lay.M, lay.No
    body = out[:, :M]
    got = gemm_ref.planes_value(body, No, lay.lo_off) if lay.planes else body[..., :No].double()
    keep = torch.ones_like(out, dtype=torch.bool)
    keep[:, :M, :No] = False
    if lay.planes:
        keep[:, :M, lay.lo_off:lay.lo_off + No] = False
    clean = bool((out[keep] == SENTINEL).all())
    return (got if lay.batched else got[0]), clean


def launch_ph(L, form, ops, tile_m, pad=0, lo_gap=0, inplace=False, overrides=None, min_ldo=0):
    """pafc_gemm_ph_ex2 on the layout above -> (rc, result as float64, sentinels intact, the output buffer)."""
    from paper_accurate_fast_cheap_amd import _lib
    lay = lay_out(form, ops, pad, lo_gap, inplace, min_ldo)
    args = dict(M=lay.M, N=lay.N, K=lay.K, batch=lay.Z, A=_lib.ptr(lay.A), lda=lay.A.stride(-2), strideA=lay.sA,
                a_split=int(form.a_split), a_plane_block=int(ops.get("plane_block", 0)), W=_lib.ptr(lay.W), ldw=lay.W.stride(-2),
                strideW=lay.sW, bias=_lib.ptr(lay.bias), strideBias=lay.sBias, residual=_lib.ptr(lay.R), res_kind=lay.res_kind,
                ldr=lay.ldr, strideR=lay.sR, out=_lib.ptr(lay.out), out_kind=OUT[form.out], ldo=lay.ldo, lo_off=lay.lo_off,
                strideO=lay.out.stride(0), alpha=float(ops.get("alpha", 1.0)), act=ACT[form.act], tile_m=tile_m,
                stream=_lib.stream_of(lay.A))
    args.update(overrides or {})
    rc = L.pafc_gemm_ph_ex2(*args.values())
    got, clean = read_back(lay)
    return rc, got, clean, lay.out


def launch_f32out(L, form, ops, pad=0, lo_gap=0, inplace=False, overrides=None, min_ldo=0, workspace=True):
    """pafc_gemm_bf16_f32out_pb (csrc/gemm_bf16.hip: fp32 or planes out, one problem per call).  The workspace is what
    pafc_gemm_bf16_f32out_workspace_bytes asks for -- inside a sentinel-filled buffer 64 floats longer -- or NULL
    (`workspace=False`).  -> (rc, result as float64, sentinels intact (workspace guard included), the output buffer, S)."""
    from paper_accurate_fast_cheap_amd import _lib
    lay = lay_out(form, ops, pad, lo_gap, inplace, min_ldo)
    assert not lay.batched and form.out != "bf16"
    ws_bytes = int(L.pafc_gemm_bf16_f32out_workspace_bytes(lay.M, lay.N, lay.K, int(form.a_split)))
    assert ws_bytes % (4 * lay.M * lay.N) == 0, ws_bytes
    S = ws_bytes // (4 * lay.M * lay.N) or 1
    ws = torch.full((ws_bytes // 4 + 64,), SENTINEL, dtype=torch.float32, device=lay.A.device) if (ws_bytes and workspace) else None
    args = dict(M=lay.M, N=lay.N, K=lay.K, A=_lib.ptr(lay.A), lda=lay.A.stride(-2), a_split=int(form.a_split),
                a_plane_block=int(ops.get("plane_block", 0)), W=_lib.ptr(lay.W), ldw=lay.W.stride(-2), bias=_lib.ptr(lay.bias),
                residual=_lib.ptr(lay.R), ldr=lay.ldr, out=_lib.ptr(lay.out), out_kind=OUT[form.out], ldo=lay.ldo,
                lo_off=lay.lo_off, alpha=float(ops.get("alpha", 1.0)), act=ACT[form.act], workspace=_lib.ptr(ws),
                workspace_bytes=ws_bytes if ws is not None else 0, stream=_lib.stream_of(lay.A))
    args.update(overrides or {})
    rc = L.pafc_gemm_bf16_f32out_pb(*args.values())
    got, clean = read_back(lay)
    if ws is not None:
        clean = clean and bool((ws[ws_bytes // 4:] == SENTINEL).all())
    return rc, got, clean, lay.out, (S if ws is not None or not ws_bytes else 1)


def launch_bf16(L, form, ops, pad=0, inplace=False, overrides=None, min_ldo=0):
    """pafc_gemm_bf16 (csrc/gemm_bf16.hip: bf16 out, bf16 bias and residual, batch over grid.y)
    -> (rc, result as float64, sentinels intact, the output buffer)."""
    from paper_accurate_fast_cheap_amd import _lib
    lay = lay_out(form, ops, pad, 0, inplace, min_ldo)
    assert form.out == "bf16" and not form.a_split
    args = dict(M=lay.M, N=lay.N, K=lay.K, batch=lay.Z, A=_lib.ptr(lay.A), lda=lay.A.stride(-2), strideA=lay.sA, W=_lib.ptr(lay.W),
                ldw=lay.W.stride(-2), strideW=lay.sW, bias=_lib.ptr(lay.bias), strideBias=lay.sBias, residual=_lib.ptr(lay.R),
                ldr=lay.ldr, strideR=lay.sR, out=_lib.ptr(lay.out), ldo=lay.ldo, strideO=lay.out.stride(0),
                alpha=float(ops.get("alpha", 1.0)), act=ACT[form.act], stream=_lib.stream_of(lay.A))
    args.update(overrides or {})
    rc = L.pafc_gemm_bf16(*args.values())
    got, clean = read_back(lay)
    return rc, got, clean, lay.out


def _inside(t, rows, cols, fill=float("nan")):
    """t (Z, r, c) in the corner of a (Z, rows, cols) buffer of `fill`."""
    buf = torch.full((t.shape[0], rows, cols), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1], :t.shape[2]] = t
    return buf


def launch_f32(L, form, ops, pad=0, inplace=False, overrides=None):
    """pafc_gemm_f32 (csrc/gemm_f32.hip: fp32 operands, bias, residual and output, batch over grid.z).  Operand rows `pad`
    floats wider with NaN in the padding (pad % 4 == 0: rows stay 16-byte aligned); the output inside a sentinel-filled buffer
    with 64 guard rows per batch entry and ldo = N + pad + 3 > N; the residual in a buffer of its own with ldr = N + pad + 5
    != ldo, or the output buffer itself (`inplace`); a batch's entries of A, W and the residual two NaN rows further apart
    than one entry; the bias per entry or shared (strideBias = 0).
    -> (rc, result as float64, sentinels intact, the output buffer)"""
    from paper_accurate_fast_cheap_amd import _lib
    assert form.out == "f32" and not form.a_split and form.act != "glu" and pad % 4 == 0
    A, W, bias, res = ops["A"], ops["W"], ops.get("bias"), ops.get("residual")
    assert A.dtype == torch.float32 and W.dtype == torch.float32
    lay = SimpleNamespace(batched=A.dim() == 3, planes=False, lo_off=0)
    u3 = lambda t: t if lay.batched else t.unsqueeze(0)
    lay.Z, lay.M, lay.N, lay.K = u3(A).shape[0], A.shape[-2], W.shape[-2], W.shape[-1]
    lay.No, spare = lay.N, 2 if lay.batched else 0
    lay.A = _inside(u3(A), lay.M + spare, lay.K + pad)
    lay.W = _inside(u3(W), lay.N + spare, lay.K + pad)
    lay.ldo = lay.N + pad + 3
    lay.out = torch.full((lay.Z, lay.M + 64, lay.ldo), SENTINEL, dtype=torch.float32, device=A.device)
    if res is not None and inplace:
        lay.out[:, :lay.M, :lay.N] = u3(res)
        R, ldr, sR = lay.out, lay.ldo, lay.out.stride(0)
    elif res is not None:
        R = _inside(u3(res), lay.M + spare, lay.N + pad + 5)
        ldr, sR = R.stride(1), R.stride(0)
    else:
        R, ldr, sR = None, 0, 0
    bias = bias.contiguous() if bias is not None else None
    sBias = bias.stride(0) if (bias is not None and bias.dim() == 2) else 0
    args = dict(M=lay.M, N=lay.N, K=lay.K, batch=lay.Z, A=_lib.ptr(lay.A), lda=lay.A.stride(1), strideA=lay.A.stride(0),
                W=_lib.ptr(lay.W), ldw=lay.W.stride(1), strideW=lay.W.stride(0), bias=_lib.ptr(bias), strideBias=sBias,
                residual=_lib.ptr(R), ldr=ldr, strideR=sR, out=_lib.ptr(lay.out), ldo=lay.ldo, strideO=lay.out.stride(0),
                alpha=float(ops.get("alpha", 1.0)), act=ACT[form.act], stream=_lib.stream_of(lay.A))
    args.update(overrides or {})
    rc = L.pafc_gemm_f32(*args.values())
    got, clean = read_back(lay)
    return rc, got, clean, lay.out


ERR_WORKSPACE = -4
TN_COL0 = 8          # the column at which dy and x start inside their wider buffers (16 bytes: the slices stay aligned)


def launch_tn(L, dy, x, out_dtype, want_bias=True, overrides=None, batched=None):
    """pafc_gemm_tn_bf16 / pafc_gemm_tn_bf16_batched (csrc/gemm_tn.hip).  dy (.., R, M) and x (.., R, N) bf16 are laid out as
    column slices [8, 8 + M) of NaN-filled buffers 24 columns wider (a batch's entries one NaN row further apart than R rows);
    dw, dbias and the workspace each lie at the front of a sentinel-filled buffer 64 elements longer than the library asks
    for.  -> (rc, dw (.., M, N), dbias (.., M) or None, sentinels intact, S, (dw, dbias, workspace buffers)) with
    S = workspace_bytes / (4 batch M (N + 1)), the only part of the plan the library reports."""
    from paper_accurate_fast_cheap_amd import _lib
    is_b = dy.dim() == 3
    batched = is_b if batched is None else batched
    u3 = lambda t: t if is_b else t.unsqueeze(0)
    Z, R, M = u3(dy).shape
    N = x.shape[-1]
    spare = 1 if is_b else 0
    nan = float("nan")
    dyb = torch.full((Z, R + spare, M + 24), nan, dtype=torch.bfloat16, device=dy.device)
    xb = torch.full((Z, R + spare, N + 24), nan, dtype=torch.bfloat16, device=dy.device)
    dyb[:, :R, TN_COL0:TN_COL0 + M] = u3(dy)
    xb[:, :R, TN_COL0:TN_COL0 + N] = u3(x)
    dys, xs = dyb[:, :R, TN_COL0:TN_COL0 + M], xb[:, :R, TN_COL0:TN_COL0 + N]
    ws_bytes = int(L.pafc_gemm_tn_batched_workspace_bytes(R, M, N, Z) if batched else L.pafc_gemm_tn_workspace_bytes(R, M, N))
    assert ws_bytes > 0 and ws_bytes % (4 * Z * M * (N + 1)) == 0, ws_bytes
    S = ws_bytes // (4 * Z * M * (N + 1))
    dw = torch.full((Z * M * N + 64,), SENTINEL, dtype=out_dtype, device=dy.device)
    db = torch.full((Z * M + 64,), SENTINEL, dtype=out_dtype, device=dy.device) if want_bias else None
    ws = torch.full((ws_bytes // 4 + 64,), SENTINEL, dtype=torch.float32, device=dy.device)
    args = dict(R=R, M=M, N=N, batch=Z, dy=_lib.ptr(dys), lda=dys.stride(1), stride_dy=dys.stride(0), x=_lib.ptr(xs),
                ldb=xs.stride(1), stride_x=xs.stride(0), dw=_lib.ptr(dw), dbias=_lib.ptr(db),
                dw_dtype=_lib.PAFC_F32 if out_dtype == torch.float32 else _lib.PAFC_BF16, workspace=_lib.ptr(ws),
                workspace_bytes=ws_bytes, stream=_lib.stream_of(dyb))
    args.update(overrides or {})
    if batched:
        rc = L.pafc_gemm_tn_bf16_batched(*args.values())
    else:
        for k in ("batch", "stride_dy", "stride_x"):
            del args[k]
        rc = L.pafc_gemm_tn_bf16(*args.values())
    clean = bool((dw[Z * M * N:] == SENTINEL).all()) and bool((ws[ws_bytes // 4:] == SENTINEL).all())
    if db is not None:
        clean = clean and bool((db[Z * M:] == SENTINEL).all())
    shape = (lambda *s: (Z,) + s if is_b else s)
    got_w = dw[:Z * M * N].reshape(shape(M, N))
    got_b = db[:Z * M].reshape(shape(M)) if db is not None else None
    return rc, got_w, got_b, clean, S, (dw, db, ws)


def judge(form, ops, rc, got, clean):
    """Random operands: -> (problem or None, worst err / bound, activation term)"""
    if rc != 0:
        return "rc %d" % rc, float("inf"), 0.0
    want = gemm_ref.ideal(form, ops)
    act_t = gemm_ref.activation_term(form, ops)
    ratio = float(((got - want).abs() / gemm_ref.bound(form, ops, act_t)).max())
    if not bool(torch.isfinite(got).all()):
        return "not finite", float("inf"), act_t
    if not clean:
        return "wrote outside the output", ratio, act_t
    return (None if ratio <= 1.0 else "err / bound = %.3g" % ratio), ratio, act_t


def judge_exact(form, ops, rc, got, clean):
    """Grid operands (gemm_ref.make_grid_operands), no activation: the result is the float64 value rounded once to the
    output type, bit for bit.  -> problem or None"""
    assert form.act == "none"
    if rc != 0:
        return "rc %d" % rc
    if not bool(torch.isfinite(got).all()):
        return "not finite"
    if not clean:
        return "wrote outside the output"
    want = gemm_ref.round_to(form, gemm_ref.ideal(form, ops))
    wrong = int((got != want).sum())
    return None if wrong == 0 else "%d of %d elements differ from the exact result" % (wrong, want.numel())
