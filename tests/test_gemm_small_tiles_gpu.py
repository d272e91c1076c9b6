"""Every tile, ring and K split of the small-tile GEMMs (csrc/gemm_bf16.hip) at small shapes, against float64.

pafc_gemm_bf16_f32out_pb (fp32 / planes out; 16 instantiations gemm_bf16_kernel<EPI 3 | 4, tile and ring, SPL>, the K split
over blockIdx.y and gemm_ksplit_reduce_kernel) and pafc_gemm_bf16 (bf16 out; EPI 0 / 1 on three tiles, GLU) are called
through the bound library, with the buffer layout of tests/gemm_launch.py: operand rows 64 elements wider than the row with
NaN in the padding, the output inside a sentinel-filled buffer with 64 guard rows, the lo plane `lo_gap` columns behind hi,
the K-split workspace with a sentinel-filled tail.  Tiles and K shares are forced with PAFC_F32OUT_TILE, PAFC_F32OUT_KSPLIT
and PAFC_GEMM_TILE, which the library reads on every call.

Two yardsticks, no tolerance of this file's own:
  * grid operands (gemm_ref.make_grid_operands; act "none"): fp32 accumulation is exact in any order and in any number of
    shares, so the result equals gemm_ref.round_to(form, ideal) BIT FOR BIT.  Everything that tests the K walk uses it -- ring
    fills, K shares, the hi / lo / hi segment borders, plane blocks, tile renumbering -- because gemm_ref.bound cannot see a
    lost plane or a lost share once K is long (its accumulation term (Kw + 8) u S swamps a 2^-9 plane from K ~ 1000 on);
  * random operands (gemm_ref.make_operands) at K <= 384, err / bound <= 1: activations, the alpha / bias order, the residual
    behind the activation, the single rounding.
Every case: rc == 0, a finite result, every sentinel outside the output intact.

Which instantiation a case takes is NOT observed: `f32out_instantiation` / `bf16_instantiation` restate the documented
dispatch rule (the tile from the environment or from the plan; the deep 6-stage ring iff a 64-row tile and tiles x S <= CUs;
EPI 3 for the raw partials of a split product).  That mirror is a statement of the contract; S = workspace_bytes / (4 M N) is
the only part the library reports.  test_every_instantiation_is_covered walks the case lists of this file with that rule
and asserts that, on the card at hand, they reach all 16 f32out instantiations, the reducing pass behind each tile and all 7
pafc_gemm_bf16 instantiations.  Per family the parity log (tests/parity_log.py) gets instantiation, S and "exact" or the
worst err / bound."""
import functools
import itertools
from collections import namedtuple

import pytest
import torch

from tests import gemm_launch, gemm_ref, parity_log
from tests.gemm_launch import ERR_ALIGNMENT, ERR_BAD_DIMS, ERR_UNSUPPORTED, SENTINEL

pytestmark = pytest.mark.gpu

ALL_FORMS = {**gemm_ref.FORMS, **gemm_ref.SMALL_TILE_FORMS}
TILES = [(128, 128), (128, 64), (64, 64)]
_tid = lambda t: "auto" if t is None else "%dx%d" % t
MCAP = 2 * 128 + 7
K_PLAIN_LONG, K1_LONG = 3136, 1088           # 49 K-steps; 3 x 17 = 51 K-steps, the segment borders at 17 and 34
SPLIT_OUTPUTS = ["f32-res-inplace", "planes"]

# name: the form; tile / ksplit: forced through the environment (None: the library's plan); pad: wider rows with NaN, and the
# lo plane 64 columns behind hi; ws: bring the workspace the library asks for; grid: grid operands, judged bit for bit
Case = namedtuple("Case", "name M N K pb tile ksplit pad ws grid batch shared_bias", defaults=(0, None, None, 0, True, False, 0, False))


def form_of(name):
    return ALL_FORMS[name]


def _alpha(name):
    return 0.5 if form_of(name).res else 1.0


def _cdiv(a, b):
    return -(-a // b)


# ---- the documented dispatch rule, restated ---------------------------------------------------------------------------
def f32out_instantiation(case, S, cus):
    """The kernel pafc_gemm_bf16_f32out_pb launches for `case` when the library reports S K shares."""
    form = form_of(case.name)
    tiles = lambda bm, bn: _cdiv(case.M, bm) * _cdiv(case.N, bn)
    if case.tile:
        bm, bn = case.tile
    elif S > 1:                                   # the automatic split: 64 x 64 at few rows, else 128 x 128
        assert case.ksplit is None
        bm, bn = (64, 64) if 2 * tiles(64, 64) <= cus else (128, 128)
    elif tiles(128, 128) >= 2 * cus:
        bm, bn = 128, 128
    else:
        bm, bn = (128, 64) if tiles(128, 64) >= 2 * cus else (64, 64)
    deep = bm == 64 and tiles(bm, bn) * S <= cus
    nst = 2 if (bm, bn) == (128, 128) else 6 if deep else 3
    epi = 3 if (form.out == "f32" or S > 1) else 4
    return "f32out<EPI=%d, %dx%d, NST=%d, SPL=%d>%s" % (epi, bm, bn, nst, form.a_split, " + reduce" if S > 1 else "")


def bf16_instantiation(case, cus):
    form = form_of(case.name)
    if form.act == "glu":
        return "bf16<EPI=2, 128x128, NST=2>"
    tiles = lambda bm, bn: _cdiv(case.M, bm) * _cdiv(case.N, bn) * max(case.batch, 1)
    bm, bn = 128, 128
    if case.tile:
        bm, bn = case.tile
    elif tiles(128, 128) * 5 < 7 * cus:
        bm, bn = (128, 64) if tiles(128, 64) >= 2 * cus else (64, 64)
    return "bf16<EPI=%d, %dx%d, NST=%d>" % (1 if form.res else 0, bm, bn, 2 if (bm, bn) == (128, 128) else 3)


def _ksteps(case):
    return (3 if form_of(case.name).a_split else 1) * case.K // 64


def _shares(forced, ksteps):
    """The K shares a forced PAFC_F32OUT_KSPLIT gives: the most, up to `forced`, of ceil(ksteps / S) steps each with none empty."""
    return max(s for s in range(1, forced + 1) if (s - 1) * _cdiv(ksteps, s) < ksteps)


def _reported_S(L, case):
    """(with the case's environment set)"""
    nbytes = int(L.pafc_gemm_bf16_f32out_workspace_bytes(case.M, case.N, case.K, int(form_of(case.name).a_split)))
    return (nbytes // (4 * case.M * case.N) or 1) if case.ws else 1


def _set_env(monkeypatch, case, tile_var="PAFC_F32OUT_TILE"):
    for var, val in ((tile_var, None if case.tile is None else _tid(case.tile)), ("PAFC_F32OUT_KSPLIT", case.ksplit)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))


# ---- the case lists -------------------------------------------------------------------------------------------------------
TILE_FORMS = ["f32", "f32-res", "f32-res-inplace", "planes", "planes-silu", "f32-tanh", "f32-relu", "f32-silu-res"]


def _walk(bm, n0, k0, ns, ks=None):
    """M in {1, bm - 1, bm, bm + 1, 2 bm + 7} at (n0, k0), every other (N, K) at M = 2 bm + 7."""
    mr = 2 * bm + 7
    shapes = [(m, n0, k0) for m in (1, bm - 1, bm, bm + 1, mr)]
    return shapes + [(mr, n, k) for n in ns for k in (ks or [k0]) if (n, k) != (n0, k0)]


def cases_tiles_forms(tile, name, a_split):
    name = ("split-" if a_split else "") + name
    return [Case(name, M, N, K, tile=tile, pad=pad) for M, N, K in _walk(tile[0], 264, 192, (8, 264, 1000)) for pad in (0, 64)]


def cases_ring_fills(tile):
    M = tile[0] + 1
    return ([Case("f32", M, 264, 64 * i, tile=tile, grid=True) for i in range(1, 8)]
            + [Case("planes", M, 264, 64 * i, tile=tile, grid=True, pad=64) for i in (1, 2, 3)]
            + [Case(name, M, 264, K1, tile=tile, grid=True, pad=pad)
               for K1 in (64, 128, 192) for name, pad in (("split-f32", 0), ("split-planes", 64))])


def cases_outside_deep_ring(cus):
    """64 x 64 forced at N = 1000 (16 column tiles): M with more tiles than CUs (the 3-stage ring, also with a single K-step),
    and 65 rows (32 tiles: the deep one)."""
    M = 64 * (cus // 16) + 1
    assert _cdiv(M, 64) * 16 > cus
    return [Case(name, m, 1000, K, tile=(64, 64), grid=True, pad=64)
            for name in ("f32-res", "planes", "split-f32", "split-planes") for m, K in ((M, 192), (M, 64), (65, 192))]


def cases_auto_split(cus):
    """Shapes whose plan splits K by itself: a few dozen rows on 64 x 64 tiles, and enough rows that the 64 x 64 tiles cover
    more than half of the CUs (128 x 128 tiles with K shares)."""
    M128 = 64 * (cus // 32 + 1) - 3
    return [Case(pre + out, M, N, K, grid=True, pad=64)
            for pre, M, N, K in (("", 40, 264, K_PLAIN_LONG), ("split-", 70, 264, K1_LONG), ("split-", M128, 1000, K1_LONG))
            for out in SPLIT_OUTPUTS]


def cases_forced_split(ksplit, tile):
    return [Case(pre + out, M, N, K, tile=tile, ksplit=ksplit, grid=True, pad=64)
            for pre, K in (("", K_PLAIN_LONG), ("split-", K1_LONG)) for out in SPLIT_OUTPUTS
            for M in (1, 70, 135) for N in (8, 264)]


def cases_empty_share(ksplit, tile):
    """9 K-steps: 4 shares of ceil(9 / 4) = 3 would leave the fourth empty, 8 of 2 the sixth to eighth."""
    return [Case(out, M, N, 576, tile=tile, ksplit=ksplit, grid=True, pad=64) for out in SPLIT_OUTPUTS for M in (1, 70, 135)
            for N in (8, 264)]


def cases_no_workspace():
    return [Case(name, 70, 264, K1_LONG, grid=True, pad=64, ws=False) for name in ("split-f32-res-inplace", "split-planes")]


def cases_plane_blocks(pb, tile):
    M = (tile[0] if tile else 64) + 6
    return [Case(name, M, 264, 1024, pb=pb, tile=tile, grid=True, pad=64) for name in ("split-f32", "split-planes")]


RENUMBERED_TILES = [7, 8, 9, 17]


def cases_renumbering(n, bf16):
    names = ("bf16", "bf16-res") if bf16 else ("f32-res", "split-planes")
    return [Case(name, 64 * n - 1, N, 128, tile=(64, 64), grid=True, pad=64) for name in names for N in (8, 64)]


BF16_FORMS = ["bf16", "bf16-silu", "bf16-tanh", "bf16-relu", "bf16-res", "bf16-silu-res", "bf16-tanh-res", "bf16-relu-res"]


def cases_bf16(tile, name):
    return [Case(name, M, N, K, tile=tile, pad=pad)
            for M, N, K in _walk(tile[0], 264, 192, (8, 264, 1000), (64, 192, 384)) for pad in (0, 64)]


def cases_bf16_glu():
    return [Case("bf16-glu64", M, N, K, pad=pad) for M, N, K in _walk(128, 768, 192, (256, 768), (64, 192, 384)) for pad in (0, 64)]


def cases_bf16_batched(tile, shared_bias):
    return [Case(name, tile[0] + 1, 264, 192, tile=tile, pad=64, batch=3, shared_bias=shared_bias)
            for name in ("bf16-res", "bf16-silu-res", "bf16-silu")]


def all_f32out_cases(cus):
    tf = [cases_tiles_forms(t, n, s) for t in TILES for n in TILE_FORMS for s in (0, 1)]
    return itertools.chain(*tf, *[cases_ring_fills(t) for t in TILES], cases_outside_deep_ring(cus), cases_auto_split(cus),
                           *[cases_forced_split(s, t) for s in KSPLITS for t in TILES],
                           *[cases_empty_share(s, t) for s in (4, 8) for t in TILES], cases_no_workspace(),
                           *[cases_plane_blocks(pb, t) for pb in PLANE_BLOCKS for t in TILES + [None]],
                           *[cases_renumbering(n, False) for n in RENUMBERED_TILES])


def all_bf16_cases():
    return itertools.chain(*[cases_bf16(t, n) for t in TILES for n in BF16_FORMS], cases_bf16_glu(),
                           *[cases_bf16_batched(t, sb) for t in TILES for sb in (False, True)],
                           *[cases_renumbering(n, True) for n in RENUMBERED_TILES])


KSPLITS = [2, 3, 5, 7, 8]
PLANE_BLOCKS = [64, 128, 512]


def grid_problems(cus):
    """(name, M, N, K, plane_block, alpha) of every case judged bit for bit (tests/test_gemm_ref.py checks that fp32 holds them)."""
    for c in itertools.chain(all_f32out_cases(cus), all_bf16_cases()):
        if c.grid:
            yield c.name, c.M, c.N, c.K, c.pb, _alpha(c.name)


# ---- operands, shared among the cases that slice them -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operands(name, rows, N, K, pb, grid, batch, shared_bias):
    form = form_of(name)
    if grid:
        ops = gemm_ref.make_grid_operands(form, rows, N, K, seed=1000 * K + N + pb, plane_block=pb, alpha=_alpha(name), device="cuda")
    else:
        ops = gemm_ref.make_operands(form, rows, N, K, seed=1000 * K + N + batch, batch=batch, alpha=_alpha(name),
                                     shared_bias=shared_bias, device="cuda")
    if form.act == "glu":
        ops["glu_half"] = gemm_ref.GLU64_HALF
    gemm_ref.products(form, ops)
    return ops


def _ops_of(case):
    """The case's problem: the first M rows of the MCAP-row problem of its (form, N, K), or a problem of its own."""
    if case.batch or case.M > MCAP:
        return _operands(case.name, case.M, case.N, case.K, case.pb, case.grid, case.batch, case.shared_bias)
    return gemm_ref.rows(_operands(case.name, MCAP, case.N, case.K, case.pb, case.grid, 0, False), case.M)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(hip, monkeypatch, family, ident, cases, bf16=False, expect_S=None):
    """Launch every case, judge it, log instantiations, S and the verdict; fail with the list of what went wrong."""
    cus, insts, worst, bad = _cus(), set(), 0.0, []
    for case in cases:
        form, ops = form_of(case.name), _ops_of(case)
        _set_env(monkeypatch, case, "PAFC_GEMM_TILE" if bf16 else "PAFC_F32OUT_TILE")
        inplace = case.name.endswith("inplace")
        if bf16:
            rc, got, clean, _ = gemm_launch.launch_bf16(hip, form, ops, pad=case.pad, inplace=inplace)
            S, inst = 1, bf16_instantiation(case, cus)
        else:
            rc, got, clean, _, S = gemm_launch.launch_f32out(hip, form, ops, pad=case.pad, lo_gap=case.pad, inplace=inplace,
                                                             workspace=case.ws)
            assert S == _reported_S(hip, case)
            inst = f32out_instantiation(case, S, cus)
        if case.grid:
            problem, ratio = gemm_launch.judge_exact(form, ops, rc, got, clean), 0.0
        else:
            problem, ratio, _ = gemm_launch.judge(form, ops, rc, got, clean)
        if expect_S is not None and problem is None:
            problem = expect_S(case, S)
        print(f"{case}: {inst} S={S} " + (problem or ("exact" if case.grid else "err/bound %.4g" % ratio)))
        insts.add(f"{inst} S={S}")
        worst = max(worst, ratio)
        if problem:
            bad.append((case, inst, S, problem))
    verdict = "exact" if all(c.grid for c in cases) else "worst err / bound %.4g" % worst
    parity_log.record(f"gemm small tiles/{family}", **{ident: "; ".join(sorted(insts)) + ": " + ("FAILED" if bad else verdict)})
    assert not bad, bad


# ---- pafc_gemm_bf16_f32out_pb ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_split", [0, 1], ids=["plain", "split"])
@pytest.mark.parametrize("name", TILE_FORMS)
@pytest.mark.parametrize("tile", TILES, ids=_tid)
def test_f32out_tiles_and_forms(hip, monkeypatch, tile, name, a_split):
    """Every forced tile x output form x plain / split A: fp32, fp32 + bias + alpha 0.5 + residual (also over the residual),
    planes, planes + SiLU, tanh, ReLU, SiLU then the residual -- M around the tile height, N tails of 8 and 1000, contiguous
    and inside wider NaN-padded rows with the lo plane behind a gap.  Random operands, K = 192: err / bound <= 1."""
    _run(hip, monkeypatch, "f32out tiles x forms", f"{_tid(tile)}/{'split-' if a_split else ''}{name}",
         cases_tiles_forms(tile, name, a_split))


@pytest.mark.parametrize("tile", TILES, ids=_tid)
def test_f32out_ring_fills(hip, monkeypatch, tile):
    """1 .. 7 K-steps (plain) and 3, 6, 9 (split: one to three per segment) against rings of 2, 3 and 6 stages: a ring shorter
    than its depth, exactly full, and wrapped.  Grid operands: bit for bit."""
    _run(hip, monkeypatch, "f32out ring fills", _tid(tile), cases_ring_fills(tile))


def test_f32out_64x64_outside_the_deep_ring(hip, monkeypatch):
    """More 64 x 64 tiles than CUs (the 3-stage ring; the XCD-aware renumbering over 16 column tiles with a tail), with three
    K-steps and with one; and the same columns at 65 rows on the deep ring."""
    _run(hip, monkeypatch, "f32out 64x64 tiles > CUs", "N=1000", cases_outside_deep_ring(_cus()))


def test_f32out_k_split_automatic(hip, monkeypatch):
    """Shapes the plan splits by itself (workspace_bytes > 0 on this card): plain K = 3136 (49 K-steps) at 40 rows, split
    K1 = 1088 (51 K-steps in shares of 13: the hi / lo / hi borders at 17 and 34 fall inside shares) on 64 x 64 and on
    128 x 128 tiles; fp32 + bias + alpha + residual in place, and planes behind a lo_off gap."""
    _run(hip, monkeypatch, "f32out K split, automatic", "plan", cases_auto_split(_cus()),
         expect_S=lambda case, S: None if S > 1 else "the plan does not split this shape on this card")


@pytest.mark.parametrize("tile", TILES, ids=_tid)
@pytest.mark.parametrize("ksplit", KSPLITS)
def test_f32out_k_split_forced(hip, monkeypatch, ksplit, tile):
    """PAFC_F32OUT_KSPLIT x forced tile at both long K: shares of unequal length, segment borders inside shares, the reducing
    pass for fp32 (alpha, bias, residual in place) and planes (lo_off gap) at M = 1, 70, 135 and N = 8, 264.  (8 shares of
    the 49 plain K-steps would be 7 x 7 and an empty one: the library reports 7.)"""
    assert _shares(ksplit, K_PLAIN_LONG // 64) == (7 if ksplit == 8 else ksplit) and _shares(ksplit, 3 * K1_LONG // 64) == ksplit
    _run(hip, monkeypatch, "f32out K split, forced", f"S={ksplit}/{_tid(tile)}", cases_forced_split(ksplit, tile),
         expect_S=lambda case, S: None if S == _shares(ksplit, _ksteps(case)) else "S = %d" % S)


@pytest.mark.parametrize("tile", TILES, ids=_tid)
@pytest.mark.parametrize("ksplit,S_want", [(4, 3), (8, 5)])
def test_f32out_forced_split_leaves_no_share_empty(hip, monkeypatch, ksplit, S_want, tile):
    """9 K-steps with 4 or 8 shares forced: the plan reduces S until (S - 1) ceil(9 / S) < 9 -- 3 shares of 3, 5 of 2, 2, 2,
    2, 1 -- workspace_bytes reports that S, and the result is exact."""
    assert S_want == _shares(ksplit, 9)
    _run(hip, monkeypatch, "f32out K split, forced, 9 K-steps", f"S={ksplit}/{_tid(tile)}", cases_empty_share(ksplit, tile),
         expect_S=lambda case, S: None if S == S_want else "S = %d, expected %d" % (S, S_want))


def test_f32out_without_a_workspace(hip, monkeypatch):
    """A shape whose plan splits, called with workspace = NULL and with a workspace four bytes short: the unsplit product
    on the unsplit plan's tile, rc == 0, exact."""
    cases = cases_no_workspace()
    for case in cases:
        _set_env(monkeypatch, case)
        assert int(hip.pafc_gemm_bf16_f32out_workspace_bytes(case.M, case.N, case.K, 1)) > 0
    _run(hip, monkeypatch, "f32out no workspace", "NULL", cases)
    for case in cases:
        form, ops = form_of(case.name), _ops_of(case)
        nbytes = int(hip.pafc_gemm_bf16_f32out_workspace_bytes(case.M, case.N, case.K, 1))
        rc, got, clean, _, _ = gemm_launch.launch_f32out(hip, form, ops, pad=64, lo_gap=64, inplace=case.name.endswith("inplace"),
                                                         overrides=dict(workspace_bytes=nbytes - 4))
        assert gemm_launch.judge_exact(form, ops, rc, got, clean) is None, case


@pytest.mark.parametrize("tile", TILES + [None], ids=_tid)
@pytest.mark.parametrize("pb", PLANE_BLOCKS)
def test_f32out_plane_blocks(hip, monkeypatch, pb, tile):
    """a_plane_block 64, 128, 512: A's planes alternate in blocks [hi PB | lo PB]; K1 = 1024 is 48 K-steps, so every one of
    these also takes the automatic K split (forced tiles keep the plan's S)."""
    _run(hip, monkeypatch, "f32out plane blocks", f"PB={pb}/{_tid(tile)}", cases_plane_blocks(pb, tile))


@pytest.mark.parametrize("n", RENUMBERED_TILES)
def test_f32out_tile_renumbering(hip, monkeypatch, n):
    """7, 8, 9 and 17 tiles of 64 x 64 (one column tile, M = 64 n - 1): no renumbered tile, all, all but a tail of one.  Every
    tile holds other values, so each is written exactly once iff the result is exact."""
    _run(hip, monkeypatch, "f32out tile renumbering", f"{n} tiles", cases_renumbering(n, False))


# ---- pafc_gemm_bf16 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BF16_FORMS)
@pytest.mark.parametrize("tile", TILES, ids=_tid)
def test_bf16_tiles_and_forms(hip, monkeypatch, tile, name):
    """pafc_gemm_bf16 on every forced tile: bf16, + SiLU / tanh / ReLU, a bf16 residual (alpha 0.5), the activation then the
    residual -- M around the tile height, N in {8, 264, 1000} x K in {64, 192, 384}, contiguous and NaN-padded."""
    _run(hip, monkeypatch, "bf16 tiles x forms", f"{_tid(tile)}/{name}", cases_bf16(tile, name), bf16=True)


def test_bf16_glu_in_blocks_of_64(hip, monkeypatch):
    """GLU on the 128 x 128 tile: the weight rows in blocks of 64 values | 64 gates, which is what pafc_gemm_bf16_glu_half
    announces at these shapes."""
    cases = cases_bf16_glu()
    for case in cases:
        assert hip.pafc_gemm_bf16_glu_half(case.M, case.N, case.K, 1) == gemm_ref.GLU64_HALF, case
    _run(hip, monkeypatch, "bf16 GLU", "128x128", cases, bf16=True)


@pytest.mark.parametrize("shared_bias", [False, True], ids=["bias-per-entry", "bias-shared"])
@pytest.mark.parametrize("tile", TILES, ids=_tid)
def test_bf16_batched_with_distinct_strides(hip, monkeypatch, tile, shared_bias):
    """batch = 3 over grid.y: A, W, the residual and the guarded, padded output each with a batch stride of its own, the bias
    per entry or shared (strideBias = 0)."""
    _run(hip, monkeypatch, "bf16 batch 3", f"{_tid(tile)}/{'shared' if shared_bias else 'per-entry'} bias",
         cases_bf16_batched(tile, shared_bias), bf16=True)


@pytest.mark.parametrize("n", RENUMBERED_TILES)
def test_bf16_tile_renumbering(hip, monkeypatch, n):
    _run(hip, monkeypatch, "bf16 tile renumbering", f"{n} tiles", cases_renumbering(n, True), bf16=True)


# ---- refusals -------------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("planes with a residual", "f32-res", dict(out_kind=2, lo_off=264, ldo=528), ERR_UNSUPPORTED),
    ("planes with a residual, split", "split-f32-res", dict(out_kind=2, lo_off=264, ldo=528), ERR_UNSUPPORTED),
    ("a_plane_block without a_split", "f32", dict(a_plane_block=64), ERR_UNSUPPORTED),
    ("a_plane_block not a power of two", "split-f32", dict(a_plane_block=96), ERR_UNSUPPORTED),
    ("a_plane_block not dividing K", "split-f32", dict(a_plane_block=128), ERR_UNSUPPORTED),
    ("K % 64", "f32", dict(K=96), ERR_UNSUPPORTED),
    ("K % 64, split", "split-planes", dict(K=160), ERR_UNSUPPORTED),
    ("N % 8", "f32", dict(N=260), ERR_UNSUPPORTED),
    ("act = 4", "f32", dict(act=4), ERR_UNSUPPORTED),
    ("act = 4, split", "split-f32", dict(act=4), ERR_UNSUPPORTED),
    ("lo_off < N", "split-planes", dict(lo_off=256), ERR_BAD_DIMS),
    ("lo_off < N, plain", "planes-silu", dict(lo_off=0), ERR_BAD_DIMS),
    ("ldo % 4, fp32 out", "f32", dict(ldo=266), ERR_ALIGNMENT),
    ("ldo % 8, planes", "split-planes", dict(ldo=532), ERR_ALIGNMENT),
]


@pytest.mark.parametrize("what,name,overrides,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_f32out_refused_combinations_leave_the_output_alone(hip, monkeypatch, what, name, overrides, code):
    """What pafc_gemm_bf16_f32out_pb refuses returns its error code and launches nothing: the sentinel-filled output is
    untouched.  (Every refused call describes operands that lie inside the buffers it is given: M = 135, N = 264, K = 192,
    output rows of 536 elements.)"""
    case = Case(name, 135, 264, 192)
    _set_env(monkeypatch, case)
    form, ops = form_of(name), _ops_of(case)
    assert 135 % 128 and 192 % 128 and 192 % 96 == 0
    rc, _, _, out, _ = gemm_launch.launch_f32out(hip, form, ops, overrides=overrides, min_ldo=536)
    torch.cuda.synchronize()
    assert rc == code, what
    assert bool((out == SENTINEL).all()), what


# ---- coverage -------------------------------------------------------------------------------------------------------------
def test_every_instantiation_is_covered(hip, monkeypatch):
    """The case lists above, walked with the mirrored dispatch rule and the S the library reports for each: on this card
    they reach every f32out instantiation (EPI 3 | 4 x SPL x {128x128 / 2, 128x64 / 3, 64x64 / 3, 64x64 / 6 stages}), the
    reducing pass behind 64 x 64, 128 x 64 and 128 x 128 tiles, and every pafc_gemm_bf16 instantiation."""
    cus, seen = _cus(), set()
    for case in all_f32out_cases(cus):
        _set_env(monkeypatch, case)
        seen.add(f32out_instantiation(case, _reported_S(hip, case), cus))
    for case in all_bf16_cases():
        seen.add(bf16_instantiation(case, cus))
    rings = [(128, 128, 2), (128, 64, 3), (64, 64, 3), (64, 64, 6)]
    want = {"f32out<EPI=%d, %dx%d, NST=%d, SPL=%d>" % (e, bm, bn, nst, spl) for e in (3, 4) for spl in (0, 1) for bm, bn, nst in rings}
    want |= {"bf16<EPI=%d, %dx%d, NST=%d>" % (e, bm, bn, nst) for e in (0, 1) for bm, bn, nst in rings[:3]} | {"bf16<EPI=2, 128x128, NST=2>"}
    reduced = {s.split(",")[1].strip() for s in seen if s.endswith("+ reduce")}
    parity_log.record("gemm small tiles/coverage", cus=cus, instantiations=sorted(seen))
    assert not want - seen, sorted(want - seen)
    assert reduced >= {"64x64", "128x64", "128x128"}, reduced
