"""Every operand form and tile height of the phase-pipelined GEMM (csrc/gemm_ph.hip) at small shapes, each result against
the float64 `ideal` of tests/gemm_ref.py within its derived `bound` (one rounding to the output type; see that module).
The kernel is called through the bound library (pafc_gemm_ph_ex2), so that batch, row strides and lo_off are reachable.

(form, tile_m) -> case id.  Every form below runs at tile_m 64, 128, 192 and 256; the id is <test>[<form>-<tile_m>]:

  launch_ph<GLU, ACT, RES, OUT, SPL>            form                    test
  shared-fragment split (a_split, out_kind 1 / 2)
    <0, 0, 0, 1, SPL>                           split-f32               test_shared_fragment_split_forms
    <0, 0, 2, 1, SPL>                           split-f32-res           test_shared_fragment_split_forms  (alpha 0.5, bias)
    <0, 0, 2, 1, SPL>  out == residual          split-f32-res-inplace   test_shared_fragment_split_forms
    <1, 0, 0, 1, SPL>                           split-f32-glu           test_shared_fragment_split_forms
    <0, 0, 0, 2, SPL>                           split-planes            test_shared_fragment_split_forms
    <0, 1, 0, 2, SPL>                           split-planes-silu       test_shared_fragment_split_forms
  the hi, lo, hi walk (a_split, out_kind 0)
    <0, 0, 0, 0>                                split-bf16              test_hi_lo_hi_walk_forms
    <0, 1, 0, 0>                                split-bf16-silu         test_hi_lo_hi_walk_forms
    <0, 0, 1, 0>                                split-bf16-res          test_hi_lo_hi_walk_forms
    <1, 0, 0, 0>                                split-bf16-glu          test_hi_lo_hi_walk_forms
  plain bf16 A
    <0, 0 / 1 / 2 / 3, 0, 0>                    bf16, bf16-silu, bf16-tanh, bf16-relu     test_plain_bf16_forms
    <1, 0, 0, 0>, <0, 0, 1, 0>                  bf16-glu, bf16-res                        test_plain_bf16_forms
    <0, 0, 0, 1>, <1, 0, 0, 1>, <0, 0, 2, 1>    f32, f32-glu, f32-res                     test_plain_bf16_forms
    <0, 0, 0, 2>, <0, 1, 0, 2>                  planes, planes-silu                       test_plain_bf16_forms
  CONV = true (conv_ph_launch: the second subsampling convolution)
    <0, 0 / 3, 0, 0, CONV>                      bf16, bf16-relu         tests/test_conv_sub_f64_gpu.py: test_conv2_bf16_ph
    <0, 0 / 3, 0, 2, CONV, 0, SPL>              split-planes (+ ReLU)   tests/test_conv_sub_f64_gpu.py: test_conv2_split_ph

Each such case walks M in {1, tile_m - 1, tile_m, tile_m + 1, 2 tile_m + 7} at one (N, K) and every (N, K) of
{8, 264, 512, 1000} x {128, 384, 1024} (GLU: {256, 768}) at M = 2 tile_m + 7.  Row strides, lo_off and sentinels:
test_row_strides_lo_off_and_sentinels; batches: test_batched_with_distinct_strides, test_blocks_walk_tiles_across_batch_entries;
plane blocks: test_plane_blocks; the wrapper's argument passing: test_wrapper_passes_tile_m_and_plane_block; refusals:
test_refused_combinations_leave_the_output_alone.  Worst err / bound per case and the measured activation term go to the
parity log (tests/parity_log.py)."""
import functools

import pytest
import torch

from tests import gemm_launch, gemm_ref, parity_log
from tests.gemm_ref import FORMS, HI_LO_HI_FORMS, PLAIN_FORMS, SHARED_FRAGMENT_FORMS

pytestmark = pytest.mark.gpu

TILES = [64, 128, 192, 256]
MMAX = 2 * 256 + 7
ERR_BAD_DIMS, ERR_UNSUPPORTED = gemm_launch.ERR_BAD_DIMS, gemm_launch.ERR_UNSUPPORTED
# the buffer layout (NaN-padded rows, sentinel-guarded output, lo_off gap), the launch and the verdict: tests/gemm_launch.py,
# shared with the battery of the small tiles (tests/test_gemm_small_tiles_gpu.py)
SENTINEL, _padded, _launch, _judge = gemm_launch.SENTINEL, gemm_launch.padded, gemm_launch.launch_ph, gemm_launch.judge


@functools.lru_cache(maxsize=None)
def _operands(name, N, K, alpha):
    """The MMAX-row problem of a form at (N, K) on the GPU with its float64 products: every M of every tile height is a row
    slice of it, and the forms that multiply the same planes share the products."""
    form = FORMS[name]
    ops = gemm_ref.make_operands(form, MMAX, N, K, seed=1000 * K + N, alpha=alpha, device="cuda")
    ops["_prod"] = _products(form.a_split, N, K)(form, ops)
    return ops


@functools.lru_cache(maxsize=None)
def _products(a_split, N, K):
    memo = {}

    def get(form, ops):
        if "p" not in memo:
            memo["p"] = gemm_ref.products(form, {"A": ops["A"], "W": ops["W"]})
        return memo["p"]
    return get


def _alpha(form):
    return 0.5 if form.res else 1.0


def _shapes(form, tile_m):
    glu = form.act == "glu"
    n0, k0, mr = (768 if glu else 264), 384, 2 * tile_m + 7
    shapes = [(m, n0, k0) for m in (1, tile_m - 1, tile_m, tile_m + 1, mr)]
    shapes += [(mr, n, k) for n in ((256, 768) if glu else (8, 264, 512, 1000)) for k in (128, 384, 1024) if (n, k) != (n0, k0)]
    return shapes


def _run_form(hip, family, name, tile_m):
    form = FORMS[name]
    worst, act_worst, bad = 0.0, 0.0, []
    for M, N, K in _shapes(form, tile_m):
        ops = gemm_ref.rows(_operands(name, N, K, _alpha(form)), M)
        rc, got, clean, _ = _launch(hip, form, ops, tile_m, inplace=name.endswith("inplace"))
        problem, ratio, act_t = _judge(form, ops, rc, got, clean)
        print(f"{name} tile_m={tile_m} M={M} N={N} K={K}: err/bound {ratio:.4g} act_term {act_t:.3g}")
        worst, act_worst = max(worst, ratio), max(act_worst, act_t)
        if problem:
            bad.append((M, N, K, problem))
    parity_log.record(f"gemm_ph forms/{family}", **{f"{name}/tile_m={tile_m} worst_err_over_bound": worst})
    if act_worst:
        parity_log.record("gemm_ph forms/activation term", **{f"{name}/tile_m={tile_m}": act_worst})
    assert not bad, (name, tile_m, bad)


@pytest.mark.parametrize("tile_m", TILES)
@pytest.mark.parametrize("name", list(SHARED_FRAGMENT_FORMS))
def test_shared_fragment_split_forms(hip, name, tile_m):
    """launch_ph<..., SPL = true>: what the headline's fp32 layers launch -- fp32 out, fp32 residual (out of place and over the
    residual, alpha 0.5 with a bias), GLU, planes, planes + SiLU."""
    _run_form(hip, "shared-fragment split", name, tile_m)


@pytest.mark.parametrize("tile_m", TILES)
@pytest.mark.parametrize("name", list(HI_LO_HI_FORMS))
def test_hi_lo_hi_walk_forms(hip, name, tile_m):
    """a_split = 1 with out_kind = 0: the K loop walks hi, lo, hi of A against [hi_w | hi_w | lo_w] (PhParams::nk1), bf16 out."""
    _run_form(hip, "hi, lo, hi walk", name, tile_m)


@pytest.mark.parametrize("tile_m", TILES)
@pytest.mark.parametrize("name", list(PLAIN_FORMS))
def test_plain_bf16_forms(hip, name, tile_m):
    """A plain bf16 A with every output kind: bf16 x {none, SiLU, tanh, ReLU, GLU, bf16 residual}, fp32 x {none, GLU, fp32
    residual}, planes x {none, SiLU}."""
    _run_form(hip, "plain bf16 A", name, tile_m)


LAYOUT_FORMS = ["split-f32-res", "split-planes-silu", "bf16-res", "split-bf16-res"]


@pytest.mark.parametrize("tile_m", TILES)
@pytest.mark.parametrize("name", LAYOUT_FORMS)
def test_row_strides_lo_off_and_sentinels(hip, name, tile_m):
    """lda, ldw, ldo, ldr 64 elements wider than the row, lo_off = N + 64: the padding of the inputs holds NaN and is never
    read, the columns outside the output, the gap between the planes and 64 guard rows behind M keep their sentinel."""
    form, worst, bad = FORMS[name], 0.0, []
    for M, N, K in [(2 * tile_m + 7, 264, 384), (tile_m + 1, 1000, 128)]:
        ops = gemm_ref.rows(_operands(name, N, K, _alpha(form)), M)
        rc, got, clean, _ = _launch(hip, form, ops, tile_m, pad=64, lo_gap=64)
        problem, ratio, _ = _judge(form, ops, rc, got, clean)
        print(f"{name} tile_m={tile_m} M={M} N={N} K={K} strided: err/bound {ratio:.4g}")
        worst = max(worst, ratio)
        if problem:
            bad.append((M, N, K, problem))
    parity_log.record("gemm_ph forms/row strides", **{f"{name}/tile_m={tile_m} worst_err_over_bound": worst})
    assert not bad, (name, tile_m, bad)


@functools.lru_cache(maxsize=None)
def _batched(name, M, N, K, batch, shared_bias):
    form = FORMS[name]
    return gemm_ref.make_operands(form, M, N, K, seed=77 + batch, batch=batch, alpha=_alpha(form), shared_bias=shared_bias,
                                  device="cuda")


@pytest.mark.parametrize("shared_bias", [False, True], ids=["bias-per-entry", "bias-shared"])
@pytest.mark.parametrize("tile_m", TILES)
@pytest.mark.parametrize("name", LAYOUT_FORMS)
def test_batched_with_distinct_strides(hip, name, tile_m, shared_bias):
    """batch = 3: every tensor with a batch stride of its own (A, W, residual and the guarded, padded output all differ), the
    bias per entry or shared (strideBias = 0)."""
    form = FORMS[name]
    ops = _batched(name, tile_m + 1, 264, 384, 3, shared_bias)
    rc, got, clean, _ = _launch(hip, form, ops, tile_m, pad=64, lo_gap=64)
    problem, ratio, _ = _judge(form, ops, rc, got, clean)
    parity_log.record("gemm_ph forms/batch 3", **{f"{name}/tile_m={tile_m}/{'shared' if shared_bias else 'per-entry'} bias": ratio})
    assert problem is None, (name, tile_m, problem)


@pytest.mark.parametrize("name", ["split-f32-res-inplace", "split-planes-silu", "bf16-res"])
def test_blocks_walk_tiles_across_batch_entries(hip, name):
    """More tiles than CUs: a block walks several tiles, across a ragged N tail (1000 = 3 x 256 + 232), a ragged M tail
    (581 = 9 x 64 + 5) and a batch boundary, with the next tile's operands prefetched under the current one."""
    form = FORMS[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tile_m, M, N, K = 64, 581, 1000, 256
    per_entry = -(-M // tile_m) * -(-N // 256)
    batch = max(7, cus // per_entry + 1)
    assert per_entry * batch > cus
    ops = _batched(name, M, N, K, batch, False)
    rc, got, clean, _ = _launch(hip, form, ops, tile_m, inplace=name.endswith("inplace"))
    problem, ratio, _ = _judge(form, ops, rc, got, clean)
    parity_log.record("gemm_ph forms/tiles > CUs", **{f"{name} worst_err_over_bound": ratio, "tiles": per_entry * batch, "cus": cus})
    assert problem is None, (name, problem)


@pytest.mark.parametrize("tile_m", TILES)
@pytest.mark.parametrize("plane_block", [64, 128, 512])
@pytest.mark.parametrize("name", ["split-f32", "split-bf16"])
def test_plane_blocks(hip, name, plane_block, tile_m):
    """a_plane_block: the planes of A alternate in blocks [hi PB | lo PB], for the shared-fragment form and the hi, lo, hi walk."""
    form = FORMS[name]
    M, N, K = 2 * tile_m + 7, 264, 1024
    ops = gemm_ref.make_operands(form, M, N, K, seed=5 + plane_block, plane_block=plane_block, device="cuda")
    rc, got, clean, _ = _launch(hip, form, ops, tile_m)
    problem, ratio, _ = _judge(form, ops, rc, got, clean)
    parity_log.record("gemm_ph forms/plane blocks", **{f"{name}/PB={plane_block}/tile_m={tile_m} worst_err_over_bound": ratio})
    assert problem is None, (name, plane_block, tile_m, problem)


@pytest.mark.parametrize("tile_m", TILES)
def test_wrapper_passes_tile_m_and_plane_block(hip, tile_m):
    """hip_ops.gemm_ph_ex(..., tile_m=...) reaches csrc/gemm_ph.hip at few rows (without tile_m those go to the small tiles
    of csrc/gemm_bf16.hip) and gives, bit for bit, what the direct call gives."""
    from paper_accurate_fast_cheap_amd.hip_ops import gemm_ph_ex
    M, N, K = 2 * tile_m + 7, 264, 384
    for name, kind in [("split-f32-res", "f32"), ("split-planes-silu", "planes"), ("split-bf16-res", "bf16"), ("f32-glu", "f32")]:
        form = FORMS[name]
        ops = gemm_ref.rows(_operands(name, 768 if form.act == "glu" else N, K, _alpha(form)), M)
        rc, _, _, direct = _launch(hip, form, ops, tile_m)
        assert rc == 0
        got = gemm_ph_ex(ops["A"].contiguous(), ops["W"], ops["bias"], form.act, alpha=ops["alpha"],
                         residual=None if ops["residual"] is None else ops["residual"].contiguous(), a_split=form.a_split,
                         out_kind=kind, tile_m=tile_m)
        assert torch.equal(got, direct[0, :M]), name
    form = FORMS["split-f32"]
    ops = gemm_ref.make_operands(form, M, N, 1024, seed=9, plane_block=128, device="cuda")
    rc, _, _, direct = _launch(hip, form, ops, tile_m)
    got = gemm_ph_ex(ops["A"], ops["W"], ops["bias"], a_split=True, out_kind="f32", tile_m=tile_m, a_plane_block=128)
    assert rc == 0 and torch.equal(got, direct[0, :M])


REFUSALS = [
    ("residual with an activation", "bf16-res", dict(act=1), ERR_UNSUPPORTED),
    ("fp32 residual with an activation, split", "split-f32-res", dict(act=1), ERR_UNSUPPORTED),
    ("bf16 residual with an fp32 output", "f32-res", dict(res_kind=1), ERR_UNSUPPORTED),
    ("planes with a bf16 residual", "bf16-res", dict(out_kind=2, lo_off=264, ldo=528), ERR_UNSUPPORTED),
    ("planes with an fp32 residual, split", "split-f32-res", dict(out_kind=2, lo_off=264, ldo=528), ERR_UNSUPPORTED),
    ("K % 128", "bf16", dict(K=320), ERR_UNSUPPORTED),
    ("K % 128, split", "split-f32", dict(K=64), ERR_UNSUPPORTED),
    ("GLU with N % 256", "bf16", dict(act=4), ERR_UNSUPPORTED),
    ("GLU with N % 256, split", "split-f32", dict(act=4), ERR_UNSUPPORTED),
    ("lo_off < N", "split-planes", dict(lo_off=256), ERR_BAD_DIMS),
    ("lo_off < N, plain", "planes-silu", dict(lo_off=0), ERR_BAD_DIMS),
]


@pytest.mark.parametrize("what,name,overrides,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_combinations_leave_the_output_alone(hip, what, name, overrides, code):
    """What pafc_gemm_ph_ex2 refuses returns its error code and launches nothing: the sentinel-filled output is untouched.
    (Every refused call describes operands that lie inside the buffers it is given.)"""
    form = FORMS[name]
    ops = gemm_ref.rows(_operands(name, 264, 384, _alpha(form)), 135)
    rc, _, _, out = _launch(hip, form, ops, 128, overrides=overrides, min_ldo=528)
    torch.cuda.synchronize()
    assert rc == code, what
    assert bool((out == SENTINEL).all()), what
