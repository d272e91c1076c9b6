"""tests/tmix_ref.py tested on the CPU: the same chain in float32 torch on the bf16 operands, rounded at the same places and cut
into the three stretches the kernels cover (each fed with the reference's own tensor, as tests/test_tmix_front_gpu.py feeds the
kernels), stays within `bound` at every stage, at that file's smallest shapes and input scales; and each of these mistakes of
such a chain falls outside the bound on at least one element of a kernel output (t, z or w):

    neighbour taken from the other side                     prev ignored / prev applied to the forward-looking direction
    neighbour not zeroed at a batch boundary                direction 1's maa / W2 used for direction 0
    two of the four maps swapped                            one 32-column block of t fed to the wrong map
    time_decay dropped                                      tanh dropped on td

None of them is indistinguishable from a correct kernel at (B, T) = (3, 21).  (At T = 1 both neighbours are the zero pad, so
the first one cannot show there; the mutations run at (3, 21) only.)"""
import functools

import pytest
import torch

from tests import tmix_ref as R

WIDTHS = [64, 512]


def _bf(v):
    return v.bfloat16().float()


def _f32_chain(ops, ref, mut=""):
    """The three kernels' arithmetic in float32: down from x; up from x and the REFERENCE's t; decay from the REFERENCE's z_w.
    `mut` names one deliberate mistake."""
    x = ops["x"].float()
    B, T, C = x.shape
    rows, nd = B * T, ops["maa_x"].shape[0]
    xf = x.reshape(rows, C)
    prev = ops["prev"]
    out = {k: [] for k in ("xxx", "t", "m", "z", "td", "w")}
    for d in range(nd):
        fwd = R.looks_forward(d, ops["reverse0"])
        if mut == "other side":
            nb = R.neighbour(x, not fwd, None if not fwd else prev)
        elif mut == "batch boundary":
            nb = torch.zeros_like(xf)
            if fwd:
                nb[:-1] = xf[1:]
            else:
                nb[1:] = xf[:-1]
                if prev is not None:
                    nb[0] = prev[0].float()
            nb = nb.view(B, T, C)
        elif mut == "prev ignored":
            nb = R.neighbour(x, fwd, None)
        elif mut == "prev forward" and fwd:
            nb = R.neighbour(x, fwd, None)
            nb[:, -1] = prev.float()
        else:
            nb = R.neighbour(x, fwd, prev)
        dw = 1 if (mut in ("maa of direction 1", "W2 of direction 1") and d == 0) else d
        xx = _bf(nb - x).reshape(rows, C)
        xxx = _bf(xf + _bf(xx * ops["maa_x"][d].float()))
        t = _bf(torch.tanh(xxx @ ops["w1n"][d].float().T))
        tq = ref["t"][d].float().reshape(rows, 4, 32).transpose(0, 1)
        if mut == "t block":
            tq = tq[[0, 1, 3, 3]]                                   # map v reads the columns of map w
        w2 = ops["w2t"][dw if mut == "W2 of direction 1" else d].float().transpose(1, 2)
        maa = ops["maa"][dw if mut == "maa of direction 1" else d].float().view(4, 1, C)
        if mut == "maps swapped":
            w2, maa = w2[[0, 2, 1, 3]], maa[[0, 2, 1, 3]]
        m = _bf(torch.bmm(tq, w2))
        z = _bf(xf + _bf(xx * _bf(maa + m)))
        pre = ref["z"][3, d].float() @ ops["d1n"][d].float().T
        td = _bf(pre if mut == "no tanh" else torch.tanh(pre))
        w = _bf(td @ ops["d2n"][d].float().T)
        if ops["time_decay"] is not None and mut != "no time_decay":
            w = _bf(ops["time_decay"][d].float() + w)
        for k, v in zip(out, (xxx, t, m, z, td, w)):
            out[k].append(v)
    out = {k: torch.stack(v).double() for k, v in out.items()}
    out["z"] = out["z"].transpose(0, 1)
    return out


@functools.lru_cache(maxsize=None)
def _case(B, T, C, nd, rev0, prev):
    ops = R.make_operands(B, T, C, nd, seed=100 * B + T + C, reverse0=rev0, prev=prev)
    ref = R.chain_rounded(ops)
    return ops, ref, {s: R.bound(s, ops, ref) for s in ("xxx", "t", "m", "z", "td", "w")}


def test_rb_is_round_to_nearest_even_on_eight_bits():
    # ties go to the even neighbour (1 + 2^-8 down, 1 + 3 2^-8 up); a hair above a tie goes up, which a detour through
    # float32 would lose
    v = torch.tensor([1.0, 1.00390625, 1.01171875, 1.0039062500001, -0.3, 0.0, 255.5], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.015625, 1.0078125, -0.30078125, 0.0, 256.0], dtype=torch.float64)
    assert torch.equal(R.rb(v), want)
    g = torch.Generator().manual_seed(5)
    f = torch.randn(100000, generator=g) * torch.exp2(torch.randint(-20, 20, (100000,), generator=g).float())
    assert torch.equal(R.rb(f.double()), f.bfloat16().double())         # float32 -> bf16 is one rounding: torch's own


def test_exact_chain_differs_from_the_rounded_one_by_roundings_only():
    ops = R.make_operands(3, 21, 64, 2, seed=1, prev=True)
    e, r = R.chain_exact(ops), R.chain_rounded(ops)
    for k in ("xxx", "t", "m", "z", "td", "w"):
        assert e[k].shape == r[k].shape and e[k].dtype == torch.float64
        err = (e[k] - r[k]).abs()
        assert 0 < float(err.max()) < 0.1, k
        assert torch.equal(r[k], R.rb(r[k])), k                          # every stage of the rounded chain is a bf16 tensor


@pytest.mark.parametrize("nd,rev0", [(1, False), (1, True), (2, False)])
@pytest.mark.parametrize("prev", [False, True])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("B,T", R.SMALL_SHAPES)
def test_float32_chain_is_within_the_bound_at_every_stage(B, T, C, nd, rev0, prev):
    ops, ref, bnd = _case(B, T, C, nd, rev0, prev)
    got = _f32_chain(ops, ref)
    for s, b in bnd.items():
        err = (got[s] - ref[s]).abs()
        assert b.shape == ref[s].shape and bool((b >= 0).all())
        assert bool((err <= b).all()), (s, float((err - b).max()), int((err > b).sum()))
    assert not bnd["xxx"].any()


def test_bound_is_zero_given_the_intermediate_and_at_most_a_step_beyond_the_fp32_error():
    """z given m exactly: zero.  Where it is not zero it is one step of the output grid, up to the fp32 terms."""
    ops, ref, bnd = _case(3, 21, 512, 2, False, True)
    for s in ("t", "td", "m"):
        assert bool((bnd[s] <= 2.0 ** -7 * ref[s].abs() + 1e-2).all())
        assert 0.0 < float((bnd[s] == 0).double().mean()) < 1.0, s        # some elements cannot flip, some can
    assert float((bnd["z"] == 0).double().mean()) > 0.5                   # K = 32: few m_q sit near a midpoint
    # w: what the hidden values that may flip move it by, then a step of td D2's grid and one of time_decay + td D2's
    moved = bnd["td"] @ ops["d2n"].double().abs().transpose(1, 2)
    assert bool((bnd["w"] <= moved + 2.0 ** -7 * (ref["_aux"]["w_exact"].abs() + ref["w"].abs()) + 2e-3).all())


MUTATIONS = [("other side", "tz"), ("batch boundary", "tz"), ("prev ignored", "tz"), ("prev forward", "tz"),
             ("maa of direction 1", "z"), ("W2 of direction 1", "z"), ("maps swapped", "z"), ("t block", "z"),
             ("no time_decay", "w"), ("no tanh", "w")]


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("mut,where", MUTATIONS)
def test_mutation_falls_outside_the_bound(mut, where, C):
    ops, ref, bnd = _case(3, 21, C, 2, False, True)
    got = _f32_chain(ops, ref, mut)
    for s in {"t": "t", "z": "z", "w": "w", "tz": "tz"}[where]:
        err = (got[s] - ref[s]).abs()
        assert bool((err > bnd[s]).any()), (mut, s)
        if s in "tz" and where == "tz" and mut != "other side":           # only the rows at a sequence end are wrong
            bad_rows = (err > bnd[s]).reshape(-1, 63, err.shape[-1]).any(-1).any(0).nonzero().flatten().tolist()
            assert set(bad_rows) <= {0, 20, 21, 41, 42, 62}, (mut, s, bad_rows)
