"""pafc_gemm_ph_ktail (csrc/gemm_ph.hip): the split-operand fp32 projections with the row tiles from `split_row` on run once per
half of K into fp32 slabs of a workspace and summed by a fix-up pass.  Every element against the float64 `ideal` of
tests/gemm_ref.py within its `bound`, UNMODIFIED: the bound allows fp32 accumulation of the K columns in any order plus eight
fp32 roundings, and the K split adds one (slab 0 + slab 1) to the three of the epilogue.

The plan is forced through the explicit arguments at the smallest shapes where it can go wrong:
  M = 582 (two full tiles + 70 rows) with split_row 0 / 256 / 512; M = 272 and 257 with split_row 256 (a tail of one 16-row
  group, of one row); N = 512 and 264 (a partial second column tile); K = 128 (two K-steps per slice, the least the tile loop
  takes) and 512; K = 1536 in plane blocks of 512 (the second slice starts in the middle of a block, as at K = 9728); rows of
  out / residual / A / W wider than the matrix with guard columns and rows; the workspace between two guards.
Forms: split-f32, split-f32-res, split-f32-res-inplace, each with alpha = 0.7 and with and without a bias."""
import functools

import pytest
import torch

from tests import gemm_ref, parity_log
from tests.gemm_ref import SHARED_FRAGMENT_FORMS

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GUARD = 64                    # floats either side of the workspace (256 bytes: the workspace stays 16-byte aligned)
ALPHA = 0.7
MMAX = 582
ERR_BAD_DIMS, ERR_UNSUPPORTED = -2, -7
KTAIL_FORMS = ["split-f32", "split-f32-res", "split-f32-res-inplace"]


@functools.lru_cache(maxsize=None)
def _base(N, K, plane_block=0):
    """The MMAX-row problem at (N, K) with bias and residual and its float64 products, formed once: every form, M and
    split_row below is a view of it."""
    form = SHARED_FRAGMENT_FORMS["split-f32-res"]
    ops = gemm_ref.make_operands(form, MMAX, N, K, seed=31 * K + N, alpha=ALPHA, plane_block=plane_block, device="cuda")
    gemm_ref.products(form, ops)
    return ops


def _case(name, N, K, M, bias, plane_block=0):
    form = SHARED_FRAGMENT_FORMS[name]
    ops = gemm_ref.rows(_base(N, K, plane_block), M)
    if form.res is None:
        ops["residual"] = None
    if not bias:
        ops["bias"] = None
    return form, ops


def _padded(t, pad, fill=float("nan")):
    if not pad:
        return t.contiguous()
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + pad,), fill, dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf


def _launch(L, ops, split_row, pad=0, inplace=False, overrides=None):
    """Operands in rows `pad` elements wider than the matrix (NaN in the padding of the inputs), the output inside a sentinel
    buffer with `pad` guard columns and 64 guard rows, the workspace between two sentinel guards.
    -> (rc, out buffer, result (M, N) float64, True if nothing outside output and workspace was written, workspace buffer)"""
    from paper_accurate_fast_cheap_amd import _lib
    A, W, bias, res = ops["A"], ops["W"], ops.get("bias"), ops.get("residual")
    M, N, K = A.shape[0], W.shape[0], W.shape[1] // 3
    Ab, Wb = _padded(A, pad), _padded(W, pad)
    ldo = N + pad
    out = torch.full((M + 64, ldo), SENTINEL, dtype=torch.float32, device=A.device)
    if res is not None and inplace:
        out[:M, :N] = res
        Rb, ldr = out, ldo
    elif res is not None:
        Rb = _padded(res, pad)
        ldr = Rb.stride(0)
    else:
        Rb, ldr = None, 0
    nws = 2 * max(M - split_row, 0) * N
    wsbuf = torch.full((GUARD + nws + GUARD,), SENTINEL, dtype=torch.float32, device=A.device)
    ws = wsbuf[GUARD:GUARD + nws]
    args = dict(M=M, N=N, K=K, batch=1, A=_lib.ptr(Ab), lda=Ab.stride(0), strideA=0, a_split=1,
                a_plane_block=int(ops.get("plane_block", 0)), W=_lib.ptr(Wb), ldw=Wb.stride(0), strideW=0,
                bias=_lib.ptr(bias.contiguous() if bias is not None else None), strideBias=0, residual=_lib.ptr(Rb),
                res_kind=2 if res is not None else 0, ldr=ldr, strideR=0, out=_lib.ptr(out), out_kind=1, ldo=ldo, lo_off=0,
                strideO=0, alpha=float(ops.get("alpha", 1.0)), act=0, tile_m=256, workspace=_lib.ptr(ws),
                workspace_bytes=nws * 4, split_row=split_row, kslices=2, stream=_lib.stream_of(A))
    args.update(overrides or {})
    rc = L.pafc_gemm_ph_ktail(*args.values())
    torch.cuda.synchronize()
    keep = torch.ones_like(out, dtype=torch.bool)
    keep[:M, :N] = False
    clean = bool((out[keep] == SENTINEL).all()) and bool((wsbuf[:GUARD] == SENTINEL).all()) and bool((wsbuf[GUARD + nws:] == SENTINEL).all())
    return rc, out, out[:M, :N].double(), clean, wsbuf


def _judge(form, ops, rc, got, clean):
    if rc != 0:
        return "rc %d" % rc, float("inf")
    want = gemm_ref.ideal(form, ops)
    ratio = float(((got - want).abs() / gemm_ref.bound(form, ops, 0.0)).max())
    if not bool(torch.isfinite(got).all()):
        return "not finite", float("inf")
    if not clean:
        return "wrote outside the output or the workspace", ratio
    return (None if ratio <= 1.0 else "err / bound = %.3g" % ratio), ratio


# (M, split_row, N, K)
SHAPES = ([(582, s, 512, 128) for s in (0, 256, 512)] + [(272, 256, 512, 128), (257, 256, 512, 128)]
          + [(582, 256, 264, 128), (582, 256, 512, 512), (582, 512, 264, 512), (257, 256, 264, 512)])


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("name", KTAIL_FORMS)
def test_ktail_forms(hip, name, bias):
    worst, bad = 0.0, []
    for M, split_row, N, K in SHAPES:
        form, ops = _case(name, N, K, M, bias)
        rc, _, got, clean, _ = _launch(hip, ops, split_row, inplace=name.endswith("inplace"))
        problem, ratio = _judge(form, ops, rc, got, clean)
        print(f"{name} bias={bias} M={M} split_row={split_row} N={N} K={K}: err/bound {ratio:.4g}")
        worst = max(worst, ratio)
        if problem:
            bad.append((M, split_row, N, K, problem))
    parity_log.record("gemm_ph ktail/forms", **{f"{name}/{'bias' if bias else 'nobias'} worst_err_over_bound": worst})
    assert not bad, (name, bias, bad)


@pytest.mark.parametrize("name", KTAIL_FORMS)
def test_plane_blocks_with_a_slice_starting_inside_a_block(hip, name):
    """K = 1536 in blocks [hi 512 | lo 512]: slice 1 starts at column 768, the middle of the second block."""
    worst, bad = 0.0, []
    for M, split_row, N in [(582, 256, 264), (582, 0, 512), (257, 256, 512)]:
        form, ops = _case(name, N, 1536, M, True, plane_block=512)
        rc, _, got, clean, _ = _launch(hip, ops, split_row, inplace=name.endswith("inplace"))
        problem, ratio = _judge(form, ops, rc, got, clean)
        print(f"{name} PB=512 M={M} split_row={split_row} N={N} K=1536: err/bound {ratio:.4g}")
        worst = max(worst, ratio)
        if problem:
            bad.append((M, split_row, N, problem))
    parity_log.record("gemm_ph ktail/plane blocks", **{f"{name}/PB=512 worst_err_over_bound": worst})
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", KTAIL_FORMS)
def test_row_strides_and_guards(hip, name):
    """lda, ldw, ldo, ldr 64 elements wider than the rows: the inputs' padding (NaN) is never read; the guard columns and the 64
    guard rows behind `out` and the guards either side of the workspace keep their sentinel."""
    worst, bad = 0.0, []
    for M, split_row, N, K in [(582, 256, 264, 128), (582, 512, 512, 512), (272, 0, 264, 512)]:
        form, ops = _case(name, N, K, M, True)
        rc, _, got, clean, _ = _launch(hip, ops, split_row, pad=64, inplace=name.endswith("inplace"))
        problem, ratio = _judge(form, ops, rc, got, clean)
        print(f"{name} strided M={M} split_row={split_row} N={N} K={K}: err/bound {ratio:.4g}")
        worst = max(worst, ratio)
        if problem:
            bad.append((M, split_row, N, K, problem))
    parity_log.record("gemm_ph ktail/row strides", **{f"{name} worst_err_over_bound": worst})
    assert not bad, (name, bad)


def test_two_calls_give_the_same_bits(hip):
    for name in KTAIL_FORMS:
        _, ops = _case(name, 512, 512, 582, True)
        a = _launch(hip, ops, 256, inplace=name.endswith("inplace"))
        b = _launch(hip, ops, 256, inplace=name.endswith("inplace"))
        assert a[0] == 0 and b[0] == 0
        assert torch.equal(a[1], b[1]), name
        assert torch.equal(a[4], b[4]), name            # the slabs too


def test_wrapper_forced_on_and_forced_off(hip):
    """hip_ops.gemm_ph_ex(tail_split=(split_row, 2)) is the direct pafc_gemm_ph_ktail call, bit for bit, also over a strided
    in-place residual stream; tail_split=None / False is pafc_gemm_ph_ex2 as it was, bit for bit."""
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.hip_ops import gemm_ph_ex
    M, N, K = 582, 264, 512
    form, ops = _case("split-f32-res", N, K, M, True)
    A, W, bias, res = ops["A"].contiguous(), ops["W"], ops["bias"], ops["residual"].contiguous()
    rc, direct, _, _, _ = _launch(hip, ops, 256)
    assert rc == 0
    on = gemm_ph_ex(A, W, bias, alpha=ALPHA, residual=res, a_split=True, out_kind="f32", tail_split=(256, 2))
    assert torch.equal(on, direct[:M, :N])
    # in place over a residual stream whose rows are wider than N
    wide = torch.full((M, N + 64), SENTINEL, device="cuda")
    wide[:, :N] = res
    gemm_ph_ex(A, W, bias, alpha=ALPHA, residual=wide[:, :N], out=wide[:, :N], a_split=True, out_kind="f32", tail_split=(256, 2))
    assert torch.equal(wide[:, :N], direct[:M, :N]) and bool((wide[:, N:] == SENTINEL).all())
    # forced off: today's single launch
    ref = torch.full((M, N), SENTINEL, device="cuda")
    rc = hip.pafc_gemm_ph_ex2(M, N, K, 1, _lib.ptr(A), A.stride(0), 0, 1, 0, _lib.ptr(W), W.stride(0), 0, _lib.ptr(bias), 0,
                              _lib.ptr(res), 2, res.stride(0), 0, _lib.ptr(ref), 1, N, 0, 0, ALPHA, 0, 256, _lib.stream_of(A))
    assert rc == 0
    for off in (None, False):
        got = gemm_ph_ex(A, W, bias, alpha=ALPHA, residual=res, a_split=True, out_kind="f32", tile_m=256, tail_split=off)
        assert torch.equal(got, ref)
    got, want = on.double(), gemm_ref.ideal(form, ops)
    assert bool(((got - want).abs() <= gemm_ref.bound(form, ops, 0.0)).all())


def test_the_library_plans_as_python_does_on_this_device(hip):
    import ctypes
    from paper_accurate_fast_cheap_amd.hip_ops import DISPATCH, _ph_ktail_plan
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row = ctypes.c_long(-1)
    for M, N, K in [(44998, 512, 2048), (44998, 512, 9728), (44998, 2048, 512), (16000, 512, 2048), (cus * 128 + 300, 512, 2048)]:
        ks = hip.pafc_gemm_ph_ktail_plan(M, N, K, 1, 0, DISPATCH["ktail_min_k"], ctypes.byref(row))       # cus 0: the device's
        assert ((row.value, ks) if ks else None) == _ph_ktail_plan(M, N, K, cus), (M, N, K)


REFUSALS = [
    ("workspace one byte short", dict(workspace_bytes=-1), ERR_BAD_DIMS),
    ("split_row not a multiple of 256", dict(split_row=128), ERR_BAD_DIMS),
    ("split_row beyond M", dict(split_row=768), ERR_BAD_DIMS),
    ("K / 32 not a multiple of 4", dict(K=64), ERR_BAD_DIMS),
    ("GLU", dict(act=4), ERR_UNSUPPORTED),
    ("an activation", dict(act=1), ERR_UNSUPPORTED),
    ("planes output", dict(out_kind=2, lo_off=512, ldo=1024), ERR_UNSUPPORTED),
    ("bf16 output", dict(out_kind=0), ERR_UNSUPPORTED),
    ("three slices", dict(kslices=3), ERR_UNSUPPORTED),
    ("a batch", dict(batch=2), ERR_UNSUPPORTED),
    ("192-row tiles", dict(tile_m=192), ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("what,overrides,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(hip, what, overrides, code):
    """Refused calls return the stated code and leave `out` and the workspace as they were.  (Every refused call describes
    operands that lie inside the buffers it is given: `out` is allocated 1024 floats wide.)"""
    form, ops = _case("split-f32", 512, 128, 582, True)
    overrides = dict(overrides)
    if overrides.get("workspace_bytes") == -1:
        overrides["workspace_bytes"] = 2 * (582 - 256) * 512 * 4 - 1
    rc, out, _, _, wsbuf = _launch(hip, ops, 256, pad=512, overrides=overrides)
    assert rc == code, what
    assert bool((out == SENTINEL).all()), what
    assert bool((wsbuf == SENTINEL).all()), what
