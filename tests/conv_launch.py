"""The buffer layout and the launches of the subsampling-convolution battery (tests/test_conv_sub_f64_gpu.py), in the way of
tests/gemm_launch.py: the image with NaN in the input row T1 - 1 of an even T1 and in the column F1 - 1 of an even F1 (no
window reads them), the output inside a SENTINEL-filled buffer with GUARD rows behind the last pixel (and, for the planes of
conv1 with a pixel stride wider than both planes, guard columns between the pixels), and the read-back that tells whether
anything outside the output was written.  The launches go through the bound library (paper_accurate_fast_cheap_amd._lib), one
function per entry point, so that relu, bias = NULL, tile_m and pixel_stride are reachable.  Every launch returns
(rc, the result as float64 (M, Co), sentinels intact, the output buffer)."""
import torch

from tests import conv_ref
from tests.gemm_launch import ERR_ALIGNMENT, ERR_BAD_DIMS, ERR_UNSUPPORTED, SENTINEL, judge, judge_exact  # noqa: F401

GUARD = 64


def poisoned(x: torch.Tensor) -> torch.Tensor:
    """A copy of the image (B, T1, F1, ...) with NaN where no window reads: the last row of an even T1, the last column of an
    even F1."""
    x = x.clone()
    if x.shape[1] % 2 == 0:
        x[:, -1] = float("nan")
    if x.shape[2] % 2 == 0:
        x[:, :, -1] = float("nan")
    return x.contiguous()


def guarded(rows: int, ld: int, dtype, device, planes: int = 1) -> torch.Tensor:
    return torch.full((planes, rows + GUARD, ld), SENTINEL, dtype=dtype, device=device)


def read_back(buf, M, n, lo=None):
    """The (M, n) result at the head of plane 0 of `buf` (+ the lo plane at lo = (plane, column offset)) as float64, and
    whether every other element of the buffer kept the sentinel."""
    got = buf[0, :M, :n].double()
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[0, :M, :n] = False
    if lo is not None:
        got = got + buf[lo[0], :M, lo[1]:lo[1] + n].double()
        keep[lo[0], :M, lo[1]:lo[1] + n] = False
    return got, bool((buf[keep] == SENTINEL).all())


def _dims(ops, overrides):
    d = ops["case"]._asdict()
    d.update({k: v for k, v in (overrides or {}).items() if k in d})
    return d["B"], d["T1"], d["F1"], d["Ci"], d["Co"]


def _relu(form):
    return int(form.act == "relu")


def launch_bf16(L, form, ops, tile_m=None, overrides=None):
    """pafc_conv3x3s2_nhwc_bf16, or with tile_m pafc_conv3x3s2_nhwc_bf16_ph.  `overrides` replaces dimensions in the CALL (the
    buffers stay those of the case: a refused call describes operands inside them)."""
    from paper_accurate_fast_cheap_amd import _lib
    x, w, b = poisoned(ops["x"]), ops["taps"].contiguous(), ops.get("bias")
    M, Co = conv_ref.rows_of(ops["case"]), ops["case"].Co
    buf = guarded(M, Co, torch.bfloat16, x.device)
    dims = _dims(ops, overrides)
    tile_m = (overrides or {}).get("tile_m", tile_m)
    if tile_m is None:
        rc = L.pafc_conv3x3s2_nhwc_bf16(*dims, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(buf), _relu(form), _lib.stream_of(x))
    else:
        rc = L.pafc_conv3x3s2_nhwc_bf16_ph(*dims, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(buf), _relu(form), tile_m,
                                           _lib.stream_of(x))
    return (rc,) + read_back(buf, M, Co) + (buf,)


def launch_f32split(L, form, ops, overrides=None):
    """pafc_conv3x3s2_nhwc_f32split: the planes of the image and of the weight as tensors of their own, fp32 bias and output."""
    from paper_accurate_fast_cheap_amd import _lib
    xh, xl = poisoned(ops["x_hi"]), poisoned(ops["x_lo"])
    wh, wl, b = ops["taps_hi"].contiguous(), ops["taps_lo"].contiguous(), ops.get("bias")
    M, Co = conv_ref.rows_of(ops["case"]), ops["case"].Co
    buf = guarded(M, Co, torch.float32, xh.device)
    rc = L.pafc_conv3x3s2_nhwc_f32split(*_dims(ops, overrides), _lib.ptr(xh), _lib.ptr(xl), _lib.ptr(wh), _lib.ptr(wl), _lib.ptr(b),
                                        _lib.ptr(buf), _relu(form), _lib.stream_of(xh))
    return (rc,) + read_back(buf, M, Co) + (buf,)


def launch_split_ph(L, form, ops, tile_m, overrides=None):
    """pafc_conv3x3s2_nhwc_split_ph: the image as planes per pixel [hi Ci | lo Ci], the weight [hi | hi | lo] per tap and row,
    fp32 bias, the output as planes per position [hi Co | lo Co]."""
    from paper_accurate_fast_cheap_amd import _lib
    x = poisoned(torch.cat([ops["x_hi"], ops["x_lo"]], dim=-1))
    w = torch.cat([ops["taps_hi"], ops["taps_hi"], ops["taps_lo"]], dim=-1).contiguous()
    b = ops.get("bias")
    M, Co = conv_ref.rows_of(ops["case"]), ops["case"].Co
    buf = guarded(M, 2 * Co, torch.bfloat16, x.device)
    tile_m = (overrides or {}).get("tile_m", tile_m)
    rc = L.pafc_conv3x3s2_nhwc_split_ph(*_dims(ops, overrides), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(buf), _relu(form),
                                        tile_m, _lib.stream_of(x))
    return (rc,) + read_back(buf, M, Co, lo=(0, Co)) + (buf,)


def _c1_dims(ops, overrides):
    B, T, Fd, _, C = _dims(ops, overrides)
    return B, T, Fd, C


def launch_c1_bf16(L, form, ops, overrides=None):
    """pafc_conv3x3s2_c1_nhwc_bf16: x (B, T, F), w (C, 9), bf16."""
    from paper_accurate_fast_cheap_amd import _lib
    x, w, b = poisoned(ops["x"].unsqueeze(-1)), ops["w"].contiguous(), ops.get("bias")
    M, C = conv_ref.rows_of(ops["case"]), ops["case"].Co
    buf = guarded(M, C, torch.bfloat16, x.device)
    rc = L.pafc_conv3x3s2_c1_nhwc_bf16(*_c1_dims(ops, overrides), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(buf), _relu(form),
                                       _lib.stream_of(x))
    return (rc,) + read_back(buf, M, C) + (buf,)


C1_LAYOUTS = ["two-tensors", "ps=C", "ps=2C", "ps=2C+8"]


def launch_c1_f32split(L, form, ops, layout, overrides=None):
    """The fp32 conv1 writing planes.  "two-tensors": pafc_conv3x3s2_c1_nhwc_f32split, a guarded tensor per plane; the others
    pafc_conv3x3s2_c1_nhwc_f32split_ps: "ps=C" the same two tensors, "ps=2C" one tensor [hi C | lo C] per pixel
    (out_lo = out_hi + C), "ps=2C+8" the same with eight guard columns behind every pixel."""
    from paper_accurate_fast_cheap_amd import _lib
    x, w, b = poisoned(ops["x"].unsqueeze(-1)), ops["w"].contiguous(), ops.get("bias")
    M, C = conv_ref.rows_of(ops["case"]), ops["case"].Co
    ps = {"two-tensors": C, "ps=C": C, "ps=2C": 2 * C, "ps=2C+8": 2 * C + 8}[layout]
    buf = guarded(M, ps, torch.bfloat16, x.device, planes=2 if ps == C else 1)
    lo = (1, 0) if ps == C else (0, C)
    hi_ptr = _lib.ptr(buf)
    lo_ptr = type(hi_ptr)(buf.data_ptr() + 2 * (lo[0] * buf.stride(0) + lo[1]))
    ps = (overrides or {}).get("pixel_stride", ps)
    if layout == "two-tensors":
        rc = L.pafc_conv3x3s2_c1_nhwc_f32split(*_c1_dims(ops, overrides), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), hi_ptr, lo_ptr,
                                               _relu(form), _lib.stream_of(x))
    else:
        rc = L.pafc_conv3x3s2_c1_nhwc_f32split_ps(*_c1_dims(ops, overrides), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), hi_ptr, lo_ptr,
                                                  ps, _relu(form), _lib.stream_of(x))
    return (rc,) + read_back(buf, M, C, lo=lo) + (buf,)
