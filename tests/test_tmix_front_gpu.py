"""The time-mix front-end kernels of csrc/glue.hip against the float64 chain of tests/tmix_ref.py: every output element of
every kernel within the derived `bound` of `chain_rounded` of the same inputs (most elements: bit-identical), and the three
kernels chained from x alone against `chain_exact` with the bf16 torch op chain as the yardstick.

Instantiations the library can launch (pafc_tmix_lora_down_bf16_prev, pafc_tmix_lora_mix4_bf16_prev, pafc_decay_lora_bf16)
and where they run here:

  tmix_lora_down_kernel<8>            PAFC_LORA_DOWN_WAVES unset / 8     test_lora_down_small, test_lora_down_walks_past_its_first_trip
  tmix_lora_down_kernel<16>           PAFC_LORA_DOWN_WAVES=16            the same two
  tmix_lora_mix4_kernel<false>        PAFC_LORA_LDSW=0, or unset below 256 row tiles   test_lora_mix4_small (C 64, 128, 512), chained
  tmix_lora_mix4_kernel<true>         PAFC_LORA_LDSW=1                   test_lora_mix4_small (C 64, 128, 512)
  tmix_lora_mix4_ws_kernel<4, 1>      from 256 row tiles, PAFC_LORA_WS_WCOLS unset / 1   test_lora_mix4_ws_walk, ..._default_grid
  tmix_lora_mix4_ws_kernel<4, 4>      PAFC_LORA_WS_WCOLS=4               test_lora_mix4_ws_walk
  tmix_lora_mix4_ws_kernel<8, 8>      PAFC_LORA_WS_WCOLS=8               test_lora_mix4_ws_walk
  decay_lora_kernel                   with and without the bias          test_decay_lora_small, test_decay_lora_walks_past_its_first_trip
  FULLROW                             a template parameter of tmix_lora_mix4_kernel that no launch sets: nothing to run

Small shapes (tmix_ref.SMALL_SHAPES): 1, 15, 16 and 17 rows, (B, T) = (3, 21) with both sequence ends inside 16-row tiles,
(5, 1) where every row is first and last; ndir 1 with reverse0 either way and ndir 2; prev None and random, where the
forward-looking direction has to give the same bits either way.

Walks past the first trip (a wave takes tile i, then i + stride):
  mix4 weight-stationary, PAFC_LORA_WS_BLOCKS=3, (B, T) = (1, 4099) and (2, 2053): 257 tiles (the last one partial, (2, 2053): a
      sequence end in tile 128), stride 12 tiles for <4, 1> (22 trips a wave), 3 for <4, 4> and <8, 8> (86 trips)
  mix4 weight-stationary, default grid G = 2048 / (8 * 2) = 128 at C 512, ndir 2, (2, 4107): 514 tiles against 512 waves
  tmix_lora_down / decay_lora: grid = CUs / 2 blocks of NW waves, rows just beyond 16 * NW * grid in three sequences, the
      last tile partial; the case asserts ntiles > grid * NW"""
import functools

import pytest
import torch

from tests import parity_log
from tests import tmix_ref as R

pytestmark = pytest.mark.gpu

DIRS = [(1, False), (1, True), (2, False)]          # (ndir, reverse0)
_ENV = ("PAFC_LORA_LDSW", "PAFC_LORA_WS_BLOCKS", "PAFC_LORA_WS_WCOLS", "PAFC_LORA_DOWN_WAVES")


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    """Only what a test sets itself selects a kernel; the LDS-resident kernels at every size (product: from 8192 rows)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(hip_ops, "_LDS_RESIDENT_MIN_ROWS", 1)


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _small.cache_clear()
    _large.cache_clear()
    torch.cuda.empty_cache()


def _case(B, T, C, nd, rev0, prev, stages):
    ops = R.make_operands(B, T, C, nd, seed=1000 * B + T + C, reverse0=rev0, prev=prev, device="cuda")
    return ops, R.chain_rounded(ops, stages=stages)


@functools.lru_cache(maxsize=None)
def _small(B, T, C, nd, rev0, prev):
    return _case(B, T, C, nd, rev0, prev, ("down", "up", "decay"))


@functools.lru_cache(maxsize=2)
def _large(B, T, C, nd, rev0, prev, stages):
    return _case(B, T, C, nd, rev0, prev, stages)


def _off(got, ops, ref, stage, what):
    """-> a description if an element of `got` is outside its bound of ref[stage], else None."""
    want = ref[stage]
    if got.shape != want.shape or got.dtype != torch.bfloat16:
        return f"{what}: {tuple(got.shape)} {got.dtype}"
    err = (got.double() - want).abs()
    over = err - R.bound(stage, ops, ref)
    n_bad, n_off = int((over > 0).sum()), int((err > 0).sum())
    print(f"{what}: {n_off} of {err.numel()} off the reference, max |err| {float(err.max()):.4g}, outside the bound {n_bad}")
    if not bool(torch.isfinite(got.float()).all()):
        return f"{what}: not finite"
    if n_bad:
        i = int(over.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        return f"{what}: {n_bad} elements outside the bound, worst at {idx}: |err| {float(err.flatten()[i]):.4g} over by {float(over.max()):.4g}"
    return None


def _down(ops):
    from paper_accurate_fast_cheap_amd import hip_ops
    return hip_ops.tmix_lora_down(ops["x"], ops["maa_x"], ops["w1n"], reverse0=ops["reverse0"], prev=ops["prev"], one_pass=True)


def _mix4(ops, t):
    from paper_accurate_fast_cheap_amd import hip_ops
    return hip_ops.tmix_lora_mix4(ops["x"], t, ops["w2t"], ops["maa"], reverse0=ops["reverse0"], prev=ops["prev"])


def _decay(ops, zw):
    from paper_accurate_fast_cheap_amd import hip_ops
    return hip_ops.decay_lora(zw, ops["d1n"], ops["d2n"], ops["time_decay"], one_pass=True)


def _forward_dirs(nd, rev0):
    return [d for d in range(nd) if R.looks_forward(d, rev0)]


def _with_and_without_prev(run, shape_args, dir_axis, what):
    """run(ops, ref) -> output; both prev settings against their reference, and the forward-looking directions bit-identical."""
    bad, outs = [], {}
    nd, rev0 = shape_args[3], shape_args[4]
    for prev in (False, True):
        ops, ref = _small(*shape_args, prev)
        outs[prev], stage = run(ops, ref)
        bad.append(_off(outs[prev], ops, ref, stage, f"{what} prev={prev}"))
    for d in _forward_dirs(nd, rev0):
        if not torch.equal(outs[False].select(dir_axis, d), outs[True].select(dir_axis, d)):
            bad.append(f"{what}: forward-looking direction {d} changes with prev")
    for d in set(range(nd)) - set(_forward_dirs(nd, rev0)):
        if torch.equal(outs[False].select(dir_axis, d), outs[True].select(dir_axis, d)):
            bad.append(f"{what}: backward-looking direction {d} ignores prev")
    return [b for b in bad if b]


@pytest.mark.parametrize("nd,rev0", DIRS)
@pytest.mark.parametrize("waves", [None, "8", "16"])
def test_lora_down_small(hip, monkeypatch, waves, nd, rev0):
    """tmix_lora_down_kernel<8> / <16>: t from x, at every small shape."""
    if waves:
        monkeypatch.setenv("PAFC_LORA_DOWN_WAVES", waves)
    bad = []
    for B, T in R.SMALL_SHAPES:
        bad += _with_and_without_prev(lambda ops, ref: (_down(ops), "t"), (B, T, 512, nd, rev0), 0, f"down B={B} T={T}")
    assert not bad, bad


@pytest.mark.parametrize("nd,rev0", DIRS)
@pytest.mark.parametrize("ldsw", [None, "0", "1"])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_lora_mix4_small(hip, monkeypatch, C, ldsw, nd, rev0):
    """tmix_lora_mix4_kernel<false> / <true>: the four lerps from x and the reference's t, blockIdx.y up to C / 64 - 1."""
    if ldsw:
        monkeypatch.setenv("PAFC_LORA_LDSW", ldsw)
    bad = []
    for B, T in R.SMALL_SHAPES:
        bad += _with_and_without_prev(lambda ops, ref: (_mix4(ops, ref["t"].bfloat16()), "z"), (B, T, C, nd, rev0), 1,
                                      f"mix4 C={C} B={B} T={T}")
    assert not bad, bad


@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("with_bias", [False, True])
def test_decay_lora_small(hip, with_bias, nd):
    """decay_lora_kernel from the reference's z_w, with and without time_decay."""
    bad = []
    for B, T in R.SMALL_SHAPES:
        ops, ref = _small(B, T, 512, nd, False, False)
        zw = ref["z"][3].bfloat16().contiguous()
        if not with_bias:
            ops = dict(ops, time_decay=None)
            ref = R.chain_rounded(ops, zw=zw, stages=("decay",))
        bad.append(_off(_decay(ops, zw), ops, ref, "w", f"decay rows={B * T} bias={with_bias}"))
    assert not any(bad), [b for b in bad if b]


@pytest.mark.parametrize("wcols", ["1", "4", "8"])
@pytest.mark.parametrize("B,T", [(1, 4099), (2, 2053)])
def test_lora_mix4_ws_walk(hip, monkeypatch, B, T, wcols):
    """tmix_lora_mix4_ws_kernel<4, 1> / <4, 4> / <8, 8> on three blocks per column slice and direction: every wave reuses its
    LDS tile for 22 (86) row tiles, across a sequence end and into a partial last tile; C = 512, both directions, with prev."""
    monkeypatch.setenv("PAFC_LORA_WS_BLOCKS", "3")
    monkeypatch.setenv("PAFC_LORA_WS_WCOLS", wcols)
    ops, ref = _large(B, T, 512, 2, False, True, ("down", "up"))
    ntiles, wrows = (B * T + 15) // 16, (4 if wcols == "1" else 1)
    assert ntiles >= 256 and ntiles > 3 * wrows and (B * T) % 16
    z = _mix4(ops, ref["t"].bfloat16())
    problem = _off(z, ops, ref, "z", f"mix4 ws WCOLS={wcols} B={B} T={T}")
    assert problem is None, problem
    no_prev = dict(ops, prev=None)
    assert torch.equal(_mix4(no_prev, ref["t"].bfloat16())[:, 1], z[:, 1])


@pytest.mark.parametrize("nd,rev0", [(1, False), (1, True)])
def test_lora_mix4_ws_walk_one_direction(hip, monkeypatch, nd, rev0):
    """The weight-stationary walk with ndir = 1, reverse0 either way, (B, T) = (2, 2053)."""
    monkeypatch.setenv("PAFC_LORA_WS_BLOCKS", "3")
    ops, ref = _large(2, 2053, 512, nd, rev0, True, ("down", "up"))
    problem = _off(_mix4(ops, ref["t"].bfloat16()), ops, ref, "z", f"mix4 ws ndir=1 reverse0={rev0}")
    assert problem is None, problem


def test_lora_mix4_ws_default_grid_second_trip(hip):
    """The product's own grid, G = 2048 / ((C / 64) ndir) = 128 blocks of 4 row waves at C = 512, ndir = 2: (2, 4107) = 8214 rows
    are 514 tiles, so two waves take a second, the last of them a partial, tile."""
    B, T, C, nd = 2, 4107, 512, 2
    G = 2048 // ((C // 64) * nd)
    ntiles = (B * T + 15) // 16
    assert ntiles > G * 4 and (B * T) % 16
    ops, ref = _case(B, T, C, nd, False, True, ("down", "up"))
    problem = _off(_mix4(ops, ref["t"].bfloat16()), ops, ref, "z", f"mix4 ws default grid, {ntiles} tiles on {G * 4} waves")
    assert problem is None, problem


def _rows_beyond_one_trip(nw, nd):
    """(B, T, grid): three sequences of just more rows than grid * nw waves take in one trip, the last tile partial."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus // nd
    T = (16 * nw * grid + 40) // 3 + 1
    while (3 * T) % 16 == 0:
        T += 1
    ntiles = (3 * T + 15) // 16
    assert ntiles > grid * nw, (ntiles, grid, nw)           # or the case would not test the walk
    return 3, T, grid


@pytest.mark.parametrize("waves", ["8", "16"])
def test_lora_down_walks_past_its_first_trip(hip, monkeypatch, waves):
    """tmix_lora_down_kernel<NW>: grid = CUs / 2 blocks; rows just beyond 16 NW grid, so some waves take a second tile."""
    monkeypatch.setenv("PAFC_LORA_DOWN_WAVES", waves)
    B, T, grid = _rows_beyond_one_trip(int(waves), 2)
    ops, ref = _case(B, T, 512, 2, False, True, ("down",))
    problem = _off(_down(ops), ops, ref, "t", f"down NW={waves} rows={B * T} grid={grid}")
    assert problem is None, problem


@pytest.mark.parametrize("with_bias", [False, True])
def test_decay_lora_walks_past_its_first_trip(hip, with_bias):
    """decay_lora_kernel: grid = CUs / 2 blocks of 8 waves; rows just beyond 16 * 8 * grid."""
    B, T, grid = _rows_beyond_one_trip(8, 2)
    ops = R.make_operands(1, B * T, 512, 2, seed=7, bias=with_bias, device="cuda")
    zw = torch.randn((2, B * T, 512), generator=torch.Generator().manual_seed(8)).bfloat16().cuda()
    ref = R.chain_rounded(ops, zw=zw, stages=("decay",))
    problem = _off(_decay(ops, zw), ops, ref, "w", f"decay rows={B * T} grid={grid} bias={with_bias}")
    assert problem is None, problem


def _torch_bf16_chain(ops):
    """The module path's arithmetic (rwkv_v6/tmix.py: mix_project / forward_state) as bf16 torch ops -> z (4, ndir, rows, C), w."""
    x = ops["x"]
    B, T, C = x.shape
    zs, ws = [], []
    for d in range(ops["maa_x"].shape[0]):
        xx = R.neighbour(x, R.looks_forward(d, ops["reverse0"]), ops["prev"]) - x
        xxx = x + xx * ops["maa_x"][d]
        t = torch.tanh(xxx @ ops["w1n"][d].T.contiguous()).view(B * T, 4, -1).transpose(0, 1)
        m = torch.bmm(t, ops["w2t"][d].transpose(1, 2).contiguous()).view(4, B, T, C)
        z = torch.stack([x + xx * (ops["maa"][d, q] + m[q]) for q in range(4)])
        ws.append(ops["time_decay"][d] + torch.tanh(z[3] @ ops["d1n"][d].T.contiguous()) @ ops["d2n"][d].T.contiguous())
        zs.append(z.view(4, B * T, C))
    return torch.stack(zs, dim=1), torch.stack(ws).view(-1, B * T, C)


@pytest.mark.parametrize("prev", [False, True])
@pytest.mark.parametrize("nd", [1, 2])
def test_chained_from_x_against_the_exact_chain(hip, nd, prev):
    """tmix_lora_down -> tmix_lora_mix4 -> decay_lora from x alone at C = 512, (B, T) = (2, 37) against chain_exact.  The
    yardstick is the error of the bf16 torch op chain on the same inputs: the kernels round where it rounds (and t, td once
    instead of twice), so their max |err| may be at most 2 x its (one intermediate that rounds the other way doubles a one-step
    error) and their mean |err| at most 1.1 x its (summation order has no systematic effect on the mean).  Both pairs go to
    the parity log, per output."""
    ops = R.make_operands(2, 37, 512, nd, seed=37 + nd, prev=prev, device="cuda")
    exact = R.chain_exact(ops)
    t = _down(ops)
    z = _mix4(ops, t)
    w = _decay(ops, z[3])
    yz, yw = _torch_bf16_chain(ops)
    assert yz.dtype == torch.bfloat16 and yw.dtype == torch.bfloat16
    pairs = {"z_r": (z[0], yz[0], exact["z"][0]), "z_k": (z[1], yz[1], exact["z"][1]), "z_v": (z[2], yz[2], exact["z"][2]),
             "w": (w, yw, exact["w"])}
    bad = []
    for name, (got, yard, want) in pairs.items():
        assert got.shape == want.shape == yard.shape
        e, y = (got.double() - want).abs(), (yard.double() - want).abs()
        vals = {"kernel_max": float(e.max()), "yardstick_max": float(y.max()), "kernel_mean": float(e.mean()),
                "yardstick_mean": float(y.mean())}
        print(f"chained ndir={nd} prev={prev} {name}: {vals}")
        parity_log.record(f"tmix front end chained/ndir={nd} prev={prev}", **{f"{name} {k}": v for k, v in vals.items()})
        if not (vals["kernel_max"] <= 2.0 * vals["yardstick_max"] and vals["kernel_mean"] <= 1.1 * vals["yardstick_mean"]):
            bad.append((name, vals))
    assert not bad, bad
