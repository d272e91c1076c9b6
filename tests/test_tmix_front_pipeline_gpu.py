"""The time-mix front-end kernels of csrc/glue.hip with the next row tile's loads in flight (the default) against their
plain loops (PAFC_TMIX_PIPE=0): in every case the two outputs are `torch.equal`, and the default form is within
`tmix_ref.bound` of `tmix_ref.chain_rounded` of the same inputs, the yardstick of tests/test_tmix_front_gpu.py.

Environment variables read per call by the launchers (pafc_tmix_lora_down_bf16_prev, pafc_tmix_lora_mix4_bf16_prev,
pafc_decay_lora_bf16), beyond those listed in tests/test_tmix_front_gpu.py:

  PAFC_TMIX_PIPE=0            tmix_lora_down_kernel<NW, false>, tmix_lora_mix4_ws_kernel<NW, WCOLS, false>, decay_lora_kernel<false>:
                              load a tile, wait, compute, store, and only then load the next one
  PAFC_LORA_DOWN_BLOCKS=n     tmix_lora_down: n blocks per direction in place of one per CU (tests and A/B runs only)
  PAFC_DECAY_LORA_BLOCKS=n    decay_lora: likewise

What a prefetch could get wrong is the tile it is formed for: a wave with no next tile must issue none, the last tile's rows
are clamped, and the neighbour row of a prefetched row may lie in another sequence or in `prev`.  So with 1 and 2 blocks of 8
(16) waves per direction:

  rows 1, 15, 16, 17          one or two tiles: every wave but one or two has no tile at all
  rows 40                     three tiles, most waves have none
  (B, T) = (1, 133)           9 tiles: with one block of 8 waves one wave walks two tiles, the rest one
  (1, 261), (7, 37)           17 tiles: two and three trips, sequence ends inside tiles ((7, 37): the neighbour of a prefetched
                              row is in another sequence, or is prev)
  ndir 1 with reverse0 either way, ndir 2; prev None and random

tmix_lora_mix4_ws (from 256 row tiles): (1, 4099) and (2, 2053), 257 tiles with a partial last one, on PAFC_LORA_WS_BLOCKS 1
and 3 with PAFC_LORA_WS_WCOLS unset, 4 and 8 (65 / 22 trips a wave for <4, 1>, 257 / 86 for <4, 4> and <8, 8>), and (2, 4107)
on the default grid, where two waves take a second tile.  One chained case from x alone at (2, 2053): tmix_lora_down ->
tmix_lora_mix4 -> decay_lora, both forms equal on t, z and w."""
import functools

import pytest
import torch

from tests import tmix_ref as R

pytestmark = pytest.mark.gpu

DIRS = [(1, False), (1, True), (2, False)]          # (ndir, reverse0)
SHAPES = [(1, 1), (1, 15), (1, 16), (1, 17), (1, 40), (1, 133), (1, 261), (7, 37)]
_ENV = ("PAFC_LORA_LDSW", "PAFC_LORA_WS_BLOCKS", "PAFC_LORA_WS_WCOLS", "PAFC_LORA_DOWN_WAVES", "PAFC_TMIX_PIPE",
        "PAFC_LORA_DOWN_BLOCKS", "PAFC_DECAY_LORA_BLOCKS")


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


@functools.lru_cache(maxsize=None)
def _small(B, T, nd, rev0, prev):
    ops = R.make_operands(B, T, 512, nd, seed=1000 * B + T, reverse0=rev0, prev=prev, device="cuda")
    return ops, R.chain_rounded(ops)


@functools.lru_cache(maxsize=2)
def _large(B, T):
    ops = R.make_operands(B, T, 512, 2, seed=1000 * B + T, prev=True, device="cuda")
    return ops, R.chain_rounded(ops, stages=("down", "up"))


def _both_forms(monkeypatch, run):
    """run() under the default form and under PAFC_TMIX_PIPE=0 -> (default, plain)."""
    monkeypatch.delenv("PAFC_TMIX_PIPE", raising=False)
    new = run()
    monkeypatch.setenv("PAFC_TMIX_PIPE", "0")
    old = run()
    monkeypatch.delenv("PAFC_TMIX_PIPE", raising=False)
    torch.cuda.synchronize()
    return new, old


def _check(new, old, ops, ref, stage, what):
    """-> a description of what is wrong with the pair, or None."""
    if new.shape != old.shape or not torch.equal(new, old):
        n = int((new != old).sum()) if new.shape == old.shape else -1
        return f"{what}: the two forms differ in {n} elements"
    want = ref[stage]
    if new.shape != want.shape or new.dtype != torch.bfloat16:
        return f"{what}: {tuple(new.shape)} {new.dtype}"
    if not bool(torch.isfinite(new.float()).all()):
        return f"{what}: not finite"
    over = (new.double() - want).abs() - R.bound(stage, ops, ref)
    n_bad = int((over > 0).sum())
    if n_bad:
        return f"{what}: {n_bad} elements outside the bound, worst over by {float(over.max()):.4g}"
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


@pytest.mark.parametrize("blocks", ["1", "2"])
@pytest.mark.parametrize("waves", ["8", "16"])
def test_lora_down_both_forms(hip, monkeypatch, waves, blocks):
    """tmix_lora_down_kernel<8> / <16> on 1 and 2 blocks per direction: every shape, direction and prev setting."""
    monkeypatch.setenv("PAFC_LORA_DOWN_WAVES", waves)
    monkeypatch.setenv("PAFC_LORA_DOWN_BLOCKS", blocks)
    bad = []
    for B, T in SHAPES:
        for nd, rev0 in DIRS:
            for prev in (False, True):
                ops, ref = _small(B, T, nd, rev0, prev)
                new, old = _both_forms(monkeypatch, lambda: _down(ops))
                bad.append(_check(new, old, ops, ref, "t", f"down B={B} T={T} ndir={nd} reverse0={rev0} prev={prev}"))
    bad = [b for b in bad if b]
    assert not bad, bad


@pytest.mark.parametrize("blocks", ["1", "2"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_decay_lora_both_forms(hip, monkeypatch, with_bias, blocks):
    """decay_lora_kernel on 1 and 2 blocks per direction from the reference's z_w of every shape, direction and prev setting."""
    monkeypatch.setenv("PAFC_DECAY_LORA_BLOCKS", blocks)
    bad = []
    for B, T in SHAPES:
        for nd, rev0 in DIRS:
            for prev in (False, True):
                ops, ref = _small(B, T, nd, rev0, prev)
                zw = ref["z"][3].bfloat16().contiguous()
                if not with_bias:
                    ops = dict(ops, time_decay=None)
                    ref = R.chain_rounded(ops, zw=zw, stages=("decay",))
                new, old = _both_forms(monkeypatch, lambda: _decay(ops, zw))
                bad.append(_check(new, old, ops, ref, "w", f"decay B={B} T={T} ndir={nd} reverse0={rev0} prev={prev} bias={with_bias}"))
    bad = [b for b in bad if b]
    assert not bad, bad


@pytest.mark.parametrize("wcols", [None, "4", "8"])
@pytest.mark.parametrize("blocks", ["1", "3"])
@pytest.mark.parametrize("B,T", [(1, 4099), (2, 2053)])
def test_lora_mix4_ws_both_forms(hip, monkeypatch, B, T, blocks, wcols):
    """tmix_lora_mix4_ws_kernel<4, 1> / <4, 4> / <8, 8> on one and three blocks per column slice and direction: 257 tiles, the
    last one partial, every wave prefetches across many trips; C = 512, both directions, with prev."""
    monkeypatch.setenv("PAFC_LORA_WS_BLOCKS", blocks)
    if wcols:
        monkeypatch.setenv("PAFC_LORA_WS_WCOLS", wcols)
    ops, ref = _large(B, T)
    assert (B * T + 15) // 16 >= 256 and (B * T) % 16
    t = ref["t"].bfloat16()
    new, old = _both_forms(monkeypatch, lambda: _mix4(ops, t))
    problem = _check(new, old, ops, ref, "z", f"mix4 ws WCOLS={wcols} blocks={blocks} B={B} T={T}")
    assert problem is None, problem


def test_lora_mix4_ws_default_grid_both_forms(hip, monkeypatch):
    """The product's own grid (128 blocks of 4 row waves at C = 512, ndir = 2) at (2, 4107): 514 tiles against 512 waves, so two
    waves prefetch a second tile, the last of them a partial one, and every other wave must prefetch nothing."""
    ops, ref = _large(2, 4107)
    assert (2 * 4107 + 15) // 16 > 2048 // 16 * 4 and (2 * 4107) % 16
    t = ref["t"].bfloat16()
    new, old = _both_forms(monkeypatch, lambda: _mix4(ops, t))
    problem = _check(new, old, ops, ref, "z", "mix4 ws default grid B=2 T=4107")
    assert problem is None, problem


def test_chained_from_x_both_forms(hip, monkeypatch):
    """tmix_lora_down -> tmix_lora_mix4 (weight-stationary) -> decay_lora from x alone at (2, 2053), both directions, with prev
    and time_decay: the two forms are equal on every output."""
    ops = R.make_operands(2, 2053, 512, 2, seed=2053, prev=True, device="cuda")

    def chain():
        t = _down(ops)
        z = _mix4(ops, t)
        return t, z, _decay(ops, z[3])

    new, old = _both_forms(monkeypatch, chain)
    for name, a, b in zip(("t", "z", "w"), new, old):
        assert a.shape == b.shape and torch.equal(a, b), f"{name}: the two forms differ"
        assert bool(torch.isfinite(a.float()).all()), name
