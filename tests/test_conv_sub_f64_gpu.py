"""The forward subsampling convolutions -- the forward kernels of csrc/conv_sub.hip and the CONV = true instantiations of
csrc/gemm_ph.hip (conv_ph_launch), every entry point of them -- at their edge shapes, each result against the float64
`ideal` of its im2col GEMM within the derived `bound` of tests/gemm_ref.py (one rounding to the output type; no tolerance is
chosen here).  Reference and case tables: tests/conv_ref.py (checked on the CPU by tests/test_conv_ref.py); buffers, sentinels
and launches through the bound library: tests/conv_launch.py.

  entry point                              test                                    tiles / layouts            cases
  pafc_conv3x3s2_nhwc_bf16                 test_conv2_bf16_default_tile            128 x 128 (default)        CONV2_CASES["bf16"][128]
  pafc_conv3x3s2_nhwc_bf16                 test_conv2_bf16_conv_tile[1..4]         PAFC_CONV_TILE 1 | 2, 3, 4 ...["bf16"][128] | [256]
  pafc_conv3x3s2_nhwc_bf16_ph              test_conv2_bf16_ph[128 | 192 | 256]     tile_m                     ...["bf16_ph"][tile_m]
  pafc_conv3x3s2_nhwc_split_ph             test_conv2_split_ph[128 | 192 | 256]    tile_m                     ...["split_ph"][tile_m]
  pafc_conv3x3s2_nhwc_f32split             test_conv2_f32split                     128 x 128                  ...["f32split"][128]
  pafc_conv3x3s2_c1_nhwc_bf16              test_conv1_bf16                                                    C1_CASES
  pafc_conv3x3s2_c1_nhwc_f32split          test_conv1_f32split[two-tensors]        a tensor per plane         C1_CASES
  pafc_conv3x3s2_c1_nhwc_f32split_ps       test_conv1_f32split[ps=C | 2C | 2C+8]   pixel_stride               C1_CASES

Every case runs with relu = 1 and 0, with a bias and with bias = NULL.  Every conv2 table holds the one-pixel image
(1, 3, 3), an image with T1 and F1 even, one with only T1 even (F1 = 39, three batch entries, tiles that start mid-frame),
one with only F1 even, M = B T2 F2 in {1, tile - 1, tile, tile + 1, 2 tile + 7} for its tile height, and Ci != Co: Ci in
{64, 128, 192, 384, 512} x Co in {128, 256, 384} (csrc/conv_sub.hip), Ci in {128, 384, 512} x Co in {8, 264, 384, 512} (the
phase-pipelined forms), walked at M = 2 tile + 7.  conv1: C in {8, 16, 64, 512, 1024, 2048} with F in {3, 4, 23, 80, 83}, T in
{3, 4, 7, 8, 11}, B in {1, 3} (row groups of four that span batch entries).  The image carries NaN in the row of an even T1 and
the column of an even F1 that no window reads; the output lies in a sentinel-filled buffer with guard rows (and, pixel stride
2 C + 8, guard columns).  Bit-exact cases on grid operands: test_exact_on_grid_operands; refusals:
test_refused_calls_leave_the_output_alone; the dispatch of pafc_conv3x3s2_nhwc_bf16 to the phase-pipelined kernel:
test_dispatch_boundary.  Worst err / bound per entry point and tile go to the parity log (tests/parity_log.py); measured on
an MI355X: bf16 0.93 - 0.95 (every PAFC_CONV_TILE), bf16_ph 0.84 - 0.90, conv1 bf16 0.996 (one rounding of a 9-term sum: the
2^-8 term is all there is), conv1 planes 0.47, split_ph 0.007, f32split 0.002 -- the bound of the split forms allows
(27 Ci + 8) 2^-24 |A| |W|^T, far more than sums of random signs lose, which is why every case runs on grid operands as well.

Not here: the hi, lo, hi walk of the split convolution (PAFC_SPLIT_WALK=hilohi is latched in a process-wide static,
split_shared_fragments(), and cannot be selected inside the suite's process); the folded-LayerNorm instantiations of
csrc/gemm_ph.hip; the conv1 weight gradient (tests/test_train_loss_kernels_gpu.py)."""
import functools

import pytest
import torch

from tests import conv_launch, conv_ref, gemm_ref, parity_log
from tests.conv_ref import C1_CASES, CONV2_CASES, Case, VARIANTS

pytestmark = pytest.mark.gpu

ERR_BAD_DIMS, ERR_UNSUPPORTED, SENTINEL = conv_launch.ERR_BAD_DIMS, conv_launch.ERR_UNSUPPORTED, conv_launch.SENTINEL


def _make(kind, case, grid=False):
    ops = conv_ref.make_problem(kind, case, device="cuda", grid=grid)
    gemm_ref.products(gemm_ref.Form(kind == "split", "f32", "none", None), ops)      # the float64 products, once per problem
    return ops


@functools.lru_cache(maxsize=None)
def _problem(kind, case):
    """The operands of a case on the GPU with their float64 products: the (relu, bias) settings and the entry points that take
    the same operands share them."""
    return _make(kind, case)


def _walk(family, launch, cases, log, key):
    """Every case with every (relu, bias) setting through `launch(form, ops)`; the worst err / bound goes to the parity log."""
    worst, bad = 0.0, []
    for case in cases:
        base = _problem(conv_ref.FORMS[family][0], case)
        for relu, with_bias in VARIANTS:
            form, ops = conv_ref.variant(family, base, relu, with_bias)
            rc, got, clean, _ = launch(form, ops)
            problem, ratio, _ = conv_launch.judge(form, ops, rc, got, clean)
            print(f"{log} {key} {tuple(case)} relu={relu} bias={int(with_bias)}: err/bound {ratio:.4g}")
            worst = max(worst, ratio)
            if problem:
                bad.append((tuple(case), relu, with_bias, problem))
    parity_log.record(f"conv_sub f64/{log}", **{f"{key} worst_err_over_bound": worst, f"{key} cases": len(cases) * len(VARIANTS)})
    assert not bad, (log, key, bad)


def test_conv2_bf16_default_tile(hip, monkeypatch):
    """conv3x3s2_kernel<4, 4, 2, 2> as pafc_conv3x3s2_nhwc_bf16 launches it by default."""
    monkeypatch.delenv("PAFC_CONV_TILE", raising=False)
    _walk("bf16", lambda f, o: conv_launch.launch_bf16(hip, f, o), CONV2_CASES["bf16"][128], "pafc_conv3x3s2_nhwc_bf16", "default tile")


@pytest.mark.parametrize("tile", [1, 2, 3, 4])
def test_conv2_bf16_conv_tile(hip, monkeypatch, tile):
    """PAFC_CONV_TILE (read per call): 1 = the default's kernel, 2 = 256 x 128 blocks on a ring of three stages with its
    counted wait, 3 = 256 x 128 with two stages, 4 = 256 x 256 (Co % 256 == 0, otherwise the default's kernel)."""
    monkeypatch.setenv("PAFC_CONV_TILE", str(tile))
    _walk("bf16", lambda f, o: conv_launch.launch_bf16(hip, f, o), CONV2_CASES["bf16"][128 if tile == 1 else 256],
          "pafc_conv3x3s2_nhwc_bf16", f"PAFC_CONV_TILE={tile}")


@pytest.mark.parametrize("tile_m", [128, 192, 256])
def test_conv2_bf16_ph(hip, tile_m):
    """launch_ph<false, 0 | 3, 0, 0, CONV>: bf16 in and out, 2 / 6 / 8 K-steps per tap, ragged N tiles."""
    _walk("bf16_ph", lambda f, o: conv_launch.launch_bf16(hip, f, o, tile_m=tile_m), CONV2_CASES["bf16_ph"][tile_m],
          "pafc_conv3x3s2_nhwc_bf16_ph", f"tile_m={tile_m}")


@pytest.mark.parametrize("tile_m", [128, 192, 256])
def test_conv2_split_ph(hip, tile_m):
    """launch_ph<false, 0 | 3, 0, 2, CONV, 0, SPL>: planes per pixel in, planes per position out, fp32 bias."""
    _walk("split_ph", lambda f, o: conv_launch.launch_split_ph(hip, f, o, tile_m), CONV2_CASES["split_ph"][tile_m],
          "pafc_conv3x3s2_nhwc_split_ph", f"tile_m={tile_m}")


def test_conv2_f32split(hip):
    """conv3x3s2_split_kernel: the planes as tensors of their own, fp32 out."""
    _walk("f32split", lambda f, o: conv_launch.launch_f32split(hip, f, o), CONV2_CASES["f32split"][128],
          "pafc_conv3x3s2_nhwc_f32split", "tile 128")


def test_conv1_bf16(hip):
    _walk("c1_bf16", lambda f, o: conv_launch.launch_c1_bf16(hip, f, o), C1_CASES, "pafc_conv3x3s2_c1_nhwc_bf16", "all C")


@pytest.mark.parametrize("layout", conv_launch.C1_LAYOUTS)
def test_conv1_f32split(hip, layout):
    """The planes of conv1 as two tensors (both entry points), as [hi C | lo C] per pixel, and with guard columns behind them."""
    entry = "pafc_conv3x3s2_c1_nhwc_f32split" + ("" if layout == "two-tensors" else "_ps")
    _walk("c1_f32split", lambda f, o: conv_launch.launch_c1_f32split(hip, f, o, layout), C1_CASES, entry, layout)


# ---- grid operands: the result is the float64 value rounded once, bit for bit ------------------------------------------------
EXACT = [("bf16", "default"), ("bf16", "PAFC_CONV_TILE=1"), ("bf16", "PAFC_CONV_TILE=2"), ("bf16", "PAFC_CONV_TILE=3"),
         ("bf16", "PAFC_CONV_TILE=4"), ("bf16_ph", 128), ("bf16_ph", 192), ("bf16_ph", 256), ("split_ph", 128), ("split_ph", 192),
         ("split_ph", 256), ("f32split", None), ("c1_bf16", None)] + [("c1_f32split", lay) for lay in conv_launch.C1_LAYOUTS]


def exact_cases(family, how):
    """The whole table of the entry point and tile: the grid case of (1, 3, 3) as of 2 tile + 7 rows."""
    if family.startswith("c1"):
        return C1_CASES
    tile = how if isinstance(how, int) else 256 if how in ("PAFC_CONV_TILE=2", "PAFC_CONV_TILE=3", "PAFC_CONV_TILE=4") else 128
    return CONV2_CASES[family][tile]


@functools.lru_cache(maxsize=None)
def _grid_problem(kind, case):
    return _make(kind, case, grid=True)


@pytest.mark.parametrize("family,how", EXACT, ids=[f"{f}-{h}" for f, h in EXACT])
def test_exact_on_grid_operands(hip, monkeypatch, family, how):
    """Every case of the tables again with operands on the grid of gemm_ref.make_grid_operands (conv_ref.make_problem(grid=
    True)): fp32 accumulation is exact in any order, so without an activation the result equals round_to(form, ideal) bit for
    bit -- a tap, channel or plane taken from the wrong place, or a plane product left out (which the bound of the split forms
    is too wide to show beyond Ci = 64), changes nearly every element (tests/test_conv_ref.py)."""
    monkeypatch.delenv("PAFC_CONV_TILE", raising=False)
    if isinstance(how, str) and how.startswith("PAFC_CONV_TILE"):
        monkeypatch.setenv("PAFC_CONV_TILE", how[-1])
    form = conv_ref.form_of(family, 0)
    launch = {"bf16": lambda f, o: conv_launch.launch_bf16(hip, f, o),
              "bf16_ph": lambda f, o: conv_launch.launch_bf16(hip, f, o, tile_m=how),
              "split_ph": lambda f, o: conv_launch.launch_split_ph(hip, f, o, how),
              "f32split": lambda f, o: conv_launch.launch_f32split(hip, f, o),
              "c1_bf16": lambda f, o: conv_launch.launch_c1_bf16(hip, f, o),
              "c1_f32split": lambda f, o: conv_launch.launch_c1_f32split(hip, f, o, how)}[family]
    bad = []
    for case in exact_cases(family, how):
        base = _grid_problem(conv_ref.FORMS[family][0], case)
        assert conv_ref.grid_bits(form, base) < 24.0, case
        for with_bias in (True, False):
            _, ops = conv_ref.variant(family, base, 0, with_bias)
            rc, got, clean, _ = launch(form, ops)
            problem = conv_launch.judge_exact(form, ops, rc, got, clean)
            if problem:
                bad.append((tuple(case), with_bias, problem))
    assert not bad, (family, how, bad)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refusals(L):
    bf, ph = conv_launch.launch_bf16, conv_launch.launch_split_ph
    c1b, c1s, f32 = conv_launch.launch_c1_bf16, conv_launch.launch_c1_f32split, conv_launch.launch_f32split
    small, odd_c = (2, 7, 12), (1, 3, 3, 1)
    return [
        ("bf16_ph Ci = 64", "bf16_ph", Case(*small, 64, 128), lambda f, o: bf(L, f, o, tile_m=256), ERR_UNSUPPORTED),
        ("bf16_ph Ci = 192", "bf16_ph", Case(*small, 192, 128), lambda f, o: bf(L, f, o, tile_m=256), ERR_UNSUPPORTED),
        ("split_ph Ci = 64", "split_ph", Case(*small, 64, 128), lambda f, o: ph(L, f, o, 256), ERR_UNSUPPORTED),
        ("split_ph Ci = 192", "split_ph", Case(*small, 192, 128), lambda f, o: ph(L, f, o, 256), ERR_UNSUPPORTED),
        ("bf16_ph tile_m = 64", "bf16_ph", Case(*small, 128, 128), lambda f, o: bf(L, f, o, tile_m=64), ERR_UNSUPPORTED),
        ("split_ph tile_m = 64", "split_ph", Case(*small, 128, 128), lambda f, o: ph(L, f, o, 64), ERR_UNSUPPORTED),
        ("bf16 Co % 128", "bf16", Case(*small, 64, 192), lambda f, o: bf(L, f, o), ERR_BAD_DIMS),
        ("f32split Co % 128", "f32split", Case(*small, 64, 192), lambda f, o: f32(L, f, o), ERR_BAD_DIMS),
        ("c1_bf16 C = 24", "c1_bf16", Case(*odd_c, 24), lambda f, o: c1b(L, f, o), ERR_BAD_DIMS),
        ("c1_bf16 C = 4096", "c1_bf16", Case(*odd_c, 4096), lambda f, o: c1b(L, f, o), ERR_BAD_DIMS),
        ("c1_f32split C = 24", "c1_f32split", Case(*odd_c, 24), lambda f, o: c1s(L, f, o, "ps=2C"), ERR_BAD_DIMS),
        ("c1_f32split C = 4096", "c1_f32split", Case(*odd_c, 4096), lambda f, o: c1s(L, f, o, "two-tensors"), ERR_BAD_DIMS),
        ("pixel_stride < C", "c1_f32split", Case(2, 7, 12, 1, 64),
         lambda f, o: c1s(L, f, o, "ps=2C+8", overrides=dict(pixel_stride=56)), ERR_BAD_DIMS),
        ("pixel_stride % 8", "c1_f32split", Case(2, 7, 12, 1, 64),
         lambda f, o: c1s(L, f, o, "ps=2C+8", overrides=dict(pixel_stride=132)), ERR_BAD_DIMS),
        ("bf16 T1 = 2", "bf16", Case(*small, 64, 128), lambda f, o: bf(L, f, o, overrides=dict(T1=2)), ERR_BAD_DIMS),
        ("bf16_ph T1 = 2", "bf16_ph", Case(*small, 128, 128), lambda f, o: bf(L, f, o, tile_m=256, overrides=dict(T1=2)), ERR_BAD_DIMS),
        ("split_ph T1 = 2", "split_ph", Case(*small, 128, 128), lambda f, o: ph(L, f, o, 256, overrides=dict(T1=2)), ERR_BAD_DIMS),
        ("f32split T1 = 2", "f32split", Case(*small, 64, 128), lambda f, o: f32(L, f, o, overrides=dict(T1=2)), ERR_BAD_DIMS),
        ("c1_bf16 T = 2", "c1_bf16", Case(2, 7, 12, 1, 64), lambda f, o: c1b(L, f, o, overrides=dict(T1=2)), ERR_BAD_DIMS),
        ("c1_f32split T = 2", "c1_f32split", Case(2, 7, 12, 1, 64), lambda f, o: c1s(L, f, o, "ps=C", overrides=dict(T1=2)), ERR_BAD_DIMS),
    ]


def test_refused_calls_leave_the_output_alone(hip, monkeypatch):
    """What the entry points refuse returns its error code and launches nothing: the sentinel-filled output is untouched.
    (Every refused call describes operands that lie inside the buffers it is given.)"""
    monkeypatch.delenv("PAFC_CONV_TILE", raising=False)
    bad = []
    for what, family, case, launch, code in _refusals(hip):
        form, ops = conv_ref.variant(family, conv_ref.make_problem(conv_ref.FORMS[family][0], case, device="cuda"), 1, True)
        rc, _, _, buf = launch(form, ops)
        torch.cuda.synchronize()
        if rc != code or not bool((buf == SENTINEL).all()):
            bad.append((what, rc, code))
    assert not bad, bad


# ---- the dispatch boundary of pafc_conv3x3s2_nhwc_bf16 -----------------------------------------------------------------------
def test_dispatch_boundary(hip, monkeypatch):
    """Co % 256 == 0 and ceil(M / 256) (Co / 256) >= 512 hands the problem to the phase-pipelined kernel: 510 tiles stay with
    conv3x3s2_kernel, 512 go -- both within the bound, the upper one bit-identical to pafc_conv3x3s2_nhwc_bf16_ph(tile_m = 256)."""
    monkeypatch.delenv("PAFC_CONV_TILE", raising=False)
    form = conv_ref.form_of("bf16", 1)
    for name, case in (("below", conv_ref.DISPATCH_BELOW), ("above", conv_ref.DISPATCH_ABOVE)):
        ops = _make("bf16", case)
        rc, got, clean, buf = conv_launch.launch_bf16(hip, form, ops)
        problem, ratio, _ = conv_launch.judge(form, ops, rc, got, clean)
        parity_log.record("conv_sub f64/dispatch boundary", **{f"{name} worst_err_over_bound": ratio, f"{name} rows": conv_ref.rows_of(case)})
        assert problem is None, (name, problem)
        if name == "above":
            rc, _, clean, direct = conv_launch.launch_bf16(hip, form, ops, tile_m=256)
            assert rc == 0 and clean and torch.equal(buf, direct)
        del ops, got, buf
