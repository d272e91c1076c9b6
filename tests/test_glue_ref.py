"""tests/glue_ref.py tested on the CPU: the same chains in float32 torch, rounded at the same places, stay within `bound` at every
output element of every shape and form tests/test_glue_f64_gpu.py runs (nothing excluded), and each of a list of plausible
kernel mistakes falls outside the bound on at least one element of the case named beside it."""
import functools

import pytest
import torch

from tests import glue_ref as R

BF16, F32 = torch.bfloat16, torch.float32


def _r(dt):
    return (lambda v: v.bfloat16().float()) if dt == BF16 else (lambda v: v)


def _silu32(v):
    return v * torch.sigmoid(v)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------

def _ln32(v, g, b, eps, mut=""):
    C = v.shape[-1]
    if mut == "group dropped":                              # the lanes of the second iteration never run
        v, g, b = v[:, :C - 8], g[:C - 8], b[:C - 8]
    m = v.sum(-1, keepdim=True) / C
    c = v - m
    if mut == "one-pass":
        var = (v * v).sum(-1, keepdim=True) / C - m * m
    else:
        var = (c * c).sum(-1, keepdim=True) / (C - 1 if mut == "C - 1" else C)
    r = 1.0 / (var.sqrt() + eps) if mut == "eps outside" else torch.rsqrt(var + eps)
    out = c * r * g + b
    if mut == "group dropped":
        out = torch.cat([out, torch.zeros(out.shape[0], 8)], -1)
    return out


def _ln_chain32(c, mut=""):
    """add_layernorm in float32 torch with the specification's rounding points.  `mut` names one deliberate mistake."""
    rx, ro = _r(c["xdt"]), _r(c["odt"])
    C = c["C"]
    X = c["x"].float().reshape(-1, C)
    if c["lens"] is not None:
        i = torch.arange(X.shape[0])
        t, L = i % c["T"], c["lens"].long()[i // c["T"]]
        beyond = ((t > L) if mut == "t > len" else (t >= L)).unsqueeze(1)
    out = {}
    xn = X
    if c["y"] is not None:
        Y = c["y"].float().reshape(-1, C)
        if c["mask_y"] and mut != "mask_y ignored":
            Y = torch.where(beyond, torch.zeros(()), Y)
        a = torch.tensor(c["alpha"], dtype=F32)
        p = Y if c["alpha"] == 1.0 else rx(a * Y)
        xn = rx((a * X if mut == "alpha on x" else X) + p)
    out["x_new"] = xn
    g1, b1 = c["g1"].float(), c["b1"].float()
    if mut == "gamma beta swapped":
        g1, b1 = b1, g1
    st = lambda v: torch.stack([v.sum(-1), (v * v).sum(-1)], -1)
    out["stats_x"] = st(xn[:, :C - 8] if mut == "group dropped" else xn)
    a1 = _ln32(xn, g1, b1, 1e-5, mut)
    if c["silu"]:
        o1 = ro(_silu32(a1)) if mut == "silu before rounding" else ro(_silu32(ro(a1)))
    else:
        o1 = ro(a1)
    if c["zero_rows"]:
        o1 = torch.where(beyond, torch.zeros(()), o1)
    out["o1"] = o1
    out["stats_o1"] = st(o1)
    if c["g2"] is not None:
        out["o2"] = ro(_ln32(a1 if mut == "LN2 from unrounded o1" else o1, c["g2"].float(), c["b2"].float(), 1e-5))
    return out


def _ln_ratios(c, ref, got):
    """Worst err / bound per output; a plane output is formed from the float32 chain's value and checked as the GPU test checks it."""
    res = {}
    for k in ("x_new", "o1", "o2"):
        if k not in ref or k not in got:
            continue
        if (k == "o1" and c["split1"]) or (k == "o2" and (c["split1"] or c["split2"])):
            hi = got[k].bfloat16().float()
            lo = (got[k] - hi).bfloat16().float()
            assert bool((lo.double().abs() <= R.bf16_half_step(hi.double())).all())
            res[k] = R.worst_ratio(hi.double() + lo.double(), ref[k], R.planes_bound(ref[k], R.bound(ref, k)))
        else:
            res[k] = R.worst_ratio(got[k], ref[k], R.bound(ref, k))
    for k in ("stats_x", "stats_o1"):
        res[k] = R.worst_ratio(got[k], ref[k][:, 0], R.bound(ref, k)[:, 0])
    return res


@functools.lru_cache(maxsize=None)
def _ln_case(C, B, T, pair, form, nan=True):
    c = R.make_ln_case(C, B, T, pair, form, nan=nan)
    return c, R.ln_reference(c)


@pytest.mark.parametrize("pair", R.LN_PAIRS)
@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_float32_layernorm_chain_is_within_the_bound(C, pair):
    for B, T in R.LN_ROWS:
        for form in R.ln_forms_of(pair):
            c, ref = _ln_case(C, B, T, pair, form)
            ratios = _ln_ratios(c, ref, _ln_chain32(c))
            assert max(ratios.values()) <= 1.0, (C, B, T, form, ratios)
            for k, b in ref["_bound"].items():
                assert b.shape == ref[k].shape and not bool((b < 0).any()), k
            assert not ref["stats_x"][:, 1:].any() and not ref["stats_o1"][:, 1:].any()


def test_layernorm_bound_is_mostly_zero_in_bf16_and_about_one_step_elsewhere():
    c, ref = _ln_case(512, 3, 7, "bf16", "y ln2 silu", False)
    for k in ("o1", "o2"):
        b = R.bound(ref, k)
        assert 0.3 < float((b == 0).double().mean()) < 1.0, k                 # bit-identical wherever no midpoint is near
    # without SiLU: one step of o1's own grid, up to the fp32 terms (o2 adds what a step of o1 moves it by)
    c, ref = _ln_case(512, 3, 7, "bf16", "ln2", False)
    assert bool((R.bound(ref, "o1") <= 2.0 ** -7 * ref["o1"].abs() + 1e-3).all())
    c, ref = _ln_case(512, 3, 7, "bf16", "y alpha 1", False)
    assert not R.bound(ref, "x_new").any()                                     # bf16 + bf16 at like magnitudes fits fp32: exact
    c, ref = _ln_case(512, 3, 7, "f32", "y alpha 0.5", False)
    assert bool((R.bound(ref, "x_new") <= 2.0 ** -23 * ref["x_new"].abs()).all())
    assert bool((R.bound(ref, "o1") <= 5e-4).all())                          # (C + 2) u of a few units


# (mistake, the case that has to show it: C, (B, T), dtype pair, form, outputs at least one of which leaves its bound)
LN_MUTATIONS = [
    ("C - 1", 8, (3, 7), "f32", "plain", ("o1",)),
    ("C - 1", 512, (3, 7), "bf16", "plain", ("o1",)),
    ("eps outside", 8, (3, 7), "f32", "plain", ("o1",)),
    ("one-pass", 8, (3, 7), "f32", "mean 40", ("o1",)),
    ("LN2 from unrounded o1", 512, (3, 7), "bf16", "ln2", ("o2",)),
    ("LN2 from unrounded o1", 72, (1, 5), "f32->bf16", "ln2", ("o2",)),
    ("silu before rounding", 512, (3, 7), "bf16", "silu", ("o1",)),
    ("mask_y ignored", 72, (3, 7), "f32", "mask_y", ("x_new", "o1")),
    ("t > len", 72, (3, 7), "bf16", "zero mask silu", ("x_new", "o1")),
    ("t > len", 8, (1, 4), "f32", "zero_rows", ("o1",)),
    ("alpha on x", 72, (1, 3), "f32", "y alpha 0.5", ("x_new",)),
    ("gamma beta swapped", 8, (1, 1), "bf16", "plain", ("o1",)),
    ("group dropped", 520, (1, 5), "f32", "plain", ("o1",)),
    ("group dropped", 520, (1, 5), "bf16", "both stats", ("o1", "stats_x")),
]


@pytest.mark.parametrize("mut,C,bt,pair,form,where", LN_MUTATIONS)
def test_layernorm_mistake_falls_outside_the_bound(mut, C, bt, pair, form, where):
    c, ref = _ln_case(C, bt[0], bt[1], pair, form, False)
    assert max(_ln_ratios(c, ref, _ln_chain32(c)).values()) <= 1.0
    ratios = _ln_ratios(c, ref, _ln_chain32(c, mut))
    for k in where:
        assert ratios[k] > 1.0, (mut, k, ratios)


# ---- depthwise convolution -----------------------------------------------------------------------------------------------

def _conv32(c, mut="", gamma=None, beta=None):
    """dwconv_kernel in float32 torch: taps applied one after the other to an accumulator that starts from the bias."""
    r = _r(c["dtype"])
    C, K, T_out, T_in, pad, act = c["C"], c["K"], c["T_out"], c["T_in"], c["pad"], c["act"]
    X = c["x"].float()
    valid = torch.ones(X.shape[:2], dtype=torch.bool)
    if c["lens"] is not None and mut != "lens ignored":
        valid = torch.arange(T_in)[None, :] < c["lens"].long()[:, None]
    if mut == "lens ignored":
        X = torch.nan_to_num(X, nan=1.0)
    if act == 1:
        val, gate = (X[..., C:2 * C], X[..., :C]) if mut == "GLU halves swapped" else (X[..., :C], X[..., C:2 * C])
        inp = val * torch.sigmoid(gate)
        inp = inp if mut == "GLU product not rounded" else r(inp)
    else:
        inp = X[..., :C]
    inp = torch.where(valid.unsqueeze(-1), inp, torch.zeros(()))
    W = c["w"].float().view(C, K)
    if mut == "taps reversed":
        W = W.flip(-1)
    if mut == "taps interleaved":                          # channel pair (c, c + 1): dword j dealt out as w0[j], w1[j]
        W = W.reshape(C // 2, 2 * K).reshape(C // 2, K, 2).permute(0, 2, 1).reshape(C, K)
    if mut == "left_pad off by one":
        pad = pad + 1
    bias = c["bias"].float() if c["bias"] is not None else torch.zeros(C)
    acc = torch.zeros(X.shape[0], T_out, C) + (0.0 if mut == "bias after rounding" else bias)
    for k in range(K):
        s = torch.arange(T_out) - pad + k
        inside = (s >= 0) & (s < T_in)
        rows = inp[:, s.clamp(0, T_in - 1)]
        if mut != "halo clamped":
            rows = torch.where(inside[None, :, None], rows, torch.zeros(()))
        acc = acc + W[:, k] * rows
    if mut == "bias after rounding":
        acc = r(acc) + bias
    if act in (0, 1):
        return r(acc)
    u = r(acc)
    if act == 3:
        src = acc if mut == "statistics of the unrounded convolution" else u
        m = src.mean(-1, keepdim=True)
        var = ((src - m) ** 2).mean(-1, keepdim=True)
        u = r((u - m) * torch.rsqrt(var + 1e-5) * gamma.float() + beta.float())
    return r(_silu32(u))


@functools.lru_cache(maxsize=None)
def _conv_case(i, nan=True):
    c = R.make_conv_case(**R.conv_cases()[i], nan=nan)
    return c, R.conv_reference(c)


def test_conv_cases_cover_what_the_issue_lists():
    cases = R.conv_cases()
    for K in R.CONV_KS:
        mine = [c for c in cases if c["K"] == K]
        assert {c["T_out"] for c in mine} == set(R.CONV_TOUT) and {c["C"] for c in mine} == set(R.CONV_CS)
        assert {c["pad"] for c in mine} >= {0, (K - 1) // 2, K - 1} and {c["tin"] for c in mine} == set(R.CONV_TIN)
        assert {c["lens"] for c in mine} >= set(R.CONV_LENS) and {c["bias"] for c in mine} == {False, True}
    for C in R.CONV_CS:
        assert {(c["dtype"], c["act"]) for c in cases if c["C"] == C} == {(d, a) for d in (F32, BF16) for a in (0, 1, 2)}
    assert any(c["act"] == 1 and c["wide"] for c in cases) and any(not c["wide"] for c in cases)


@pytest.mark.parametrize("i", range(len(R.conv_cases())))
def test_float32_convolution_is_within_the_bound(i):
    c, ref = _conv_case(i)
    got = _conv32(c)
    assert torch.isfinite(ref["y"]).all() and got.shape == ref["y"].shape
    assert R.worst_ratio(got, ref["y"], R.bound(ref, "y")) <= 1.0


def _spec(**kw):
    base = dict(K=15, T_out=17, C=130, pad=7, tin="same", lens=None, bias=True, act=0, dtype=F32, wide=True)
    base.update(kw)
    return base


CONV_MUTATIONS = [
    ("taps reversed", _spec(K=4, pad=3)),
    ("taps reversed", _spec(K=31, pad=15, dtype=BF16)),
    ("left_pad off by one", _spec(K=3, pad=1, dtype=BF16)),
    ("halo clamped", _spec(K=7, pad=3, T_out=16)),
    ("halo clamped", _spec(K=31, pad=30, tin="one", T_out=15, dtype=BF16)),
    ("lens ignored", _spec(K=15, lens=16, dtype=BF16)),
    ("lens ignored", _spec(K=3, pad=0, lens=1)),
    ("taps interleaved", _spec(K=15, dtype=BF16)),
    ("GLU halves swapped", _spec(act=1, K=7, pad=3)),
    ("GLU product not rounded", _spec(act=1, K=15, dtype=BF16, C=512)),
    ("bias after rounding", _spec(K=15, dtype=BF16, C=512)),
]


@pytest.mark.parametrize("mut,spec", CONV_MUTATIONS)
def test_convolution_mistake_falls_outside_the_bound(mut, spec):
    c = R.make_conv_case(**spec)
    ref = R.conv_reference(c)
    assert R.worst_ratio(_conv32(c), ref["y"], R.bound(ref, "y")) <= 1.0
    assert R.worst_ratio(_conv32(c, mut), ref["y"], R.bound(ref, "y")) > 1.0, mut


@pytest.mark.parametrize("i", range(len(R.act3_cases())))
def test_float32_act3_chain_is_within_the_bound_and_its_mistake_is_not(i):
    c = R.make_act3_case(R.act3_cases()[i])
    ref = R.conv_reference(c, gamma=c["gamma"], beta=c["beta"])
    got = _conv32(c, gamma=c["gamma"], beta=c["beta"])
    assert R.worst_ratio(got, ref["y"], R.bound(ref, "y")) <= 1.0
    if c["T_out"] == 33:                                   # the named cases: K = 15 and 31, T = 33, bias shift 0 and 40
        bad = _conv32(c, "statistics of the unrounded convolution", gamma=c["gamma"], beta=c["beta"])
        assert R.worst_ratio(bad, ref["y"], R.bound(ref, "y")) > 1.0


def test_act3_cases_cover_what_the_issue_lists():
    cases = R.act3_cases()
    for K in (15, 31):
        mine = [c for c in cases if c["K"] == K]
        assert {c["T_out"] for c in mine} == set(R.CONV_TOUT) and {c["tin"] for c in mine} == {"same", "causal"}
        assert {c["shift"] for c in mine} == {0.0, 40.0} and {c["wide"] for c in mine} == {False, True}


# ---- weight gradient ---------------------------------------------------------------------------------------------------------

def _wgrad32(c, mut=""):
    x, dy, K, pad = c["x"].float(), c["dy"].float(), c["K"], c["pad"]
    B, T_out, C = dy.shape
    T_in = x.shape[1]
    T_walk = -(-T_out // 16) * 16 if mut == "frames past T_out" else T_out       # the whole last tile
    dw = torch.zeros(C, K)
    t = torch.arange(T_walk)
    g = dy[:, t.clamp(max=T_out - 1)]
    for k in range(K):
        s = t + k - pad + (1 if mut == "x shifted by a tap" else 0)
        rows = torch.where(((s >= 0) & (s < T_in))[None, :, None], x[:, s.clamp(0, T_in - 1)], torch.zeros(()))
        dw[:, k] = (g * rows).sum((0, 1))
    return dw.view(C, 1, K), g.sum((0, 1))


@pytest.mark.parametrize("i", range(len(R.wgrad_cases())))
def test_float32_weight_gradient_is_within_the_bound(i):
    c = R.make_wgrad_case(**R.wgrad_cases()[i])
    ref = R.dwconv_wgrad_rounded(c["x"], c["dy"], c["K"], c["pad"])
    dw, db = _wgrad32(c)
    assert R.worst_ratio(dw, ref["dw"], R.bound(ref, "dw")) <= 1.0 and R.worst_ratio(db, ref["db"], R.bound(ref, "db")) <= 1.0


WGRAD_MUTATIONS = [("x shifted by a tap", dict(K=4, B=1, T_out=127, C=2, causal=True, dtype=F32, wide=False, want_bias=True)),
                   ("x shifted by a tap", dict(K=31, B=3, T_out=257, C=130, causal=False, dtype=BF16, wide=True, want_bias=True)),
                   ("frames past T_out", dict(K=15, B=1, T_out=129, C=130, causal=False, dtype=F32, wide=True, want_bias=True)),
                   ("frames past T_out", dict(K=3, B=1, T_out=1, C=2, causal=True, dtype=BF16, wide=False, want_bias=True))]


@pytest.mark.parametrize("mut,spec", WGRAD_MUTATIONS)
def test_weight_gradient_mistake_falls_outside_the_bound(mut, spec):
    c = R.make_wgrad_case(**spec)
    ref = R.dwconv_wgrad_rounded(c["x"], c["dy"], c["K"], c["pad"])
    dw, db = _wgrad32(c, mut)
    assert R.worst_ratio(dw, ref["dw"], R.bound(ref, "dw")) > 1.0
    if mut == "frames past T_out":
        assert R.worst_ratio(db, ref["db"], R.bound(ref, "db")) > 1.0


def test_wgrad_cases_cover_what_the_issue_lists():
    cases = R.wgrad_cases()
    for K in R.CONV_KS:
        assert {(c["B"], c["T_out"]) for c in cases if c["K"] == K} == set(R.WGRAD_BT)
    for dt in (F32, BF16):
        mine = [c for c in cases if c["dtype"] == dt]
        assert {c["C"] for c in mine} == set(R.WGRAD_CS) and {c["causal"] for c in mine} == {False, True}
        assert {c["K"] for c in mine} == set(R.CONV_KS)
    assert {c["wide"] for c in cases} == {False, True} and {c["want_bias"] for c in cases} == {False, True}


# ---- roundings and planes ---------------------------------------------------------------------------------------------------

def test_r32_rounds_to_nearest_even_and_keeps_subnormals():
    one = 2.0 ** -24                                      # half a float32 step at 1
    v = torch.tensor([1.0, 1 + one, 1 + 3 * one, 1 + one + 2.0 ** -50, -(1 + one), 0.0, 2.0 ** -149, 2.0 ** -150,
                      3 * 2.0 ** -150, 2.0 ** -150 + 2.0 ** -200, 2.0 ** -126 - 2.0 ** -150], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1 + 4 * one, 1 + 2 * one, -1.0, 0.0, 2.0 ** -149, 0.0, 2.0 ** -148, 2.0 ** -149,
                         2.0 ** -126], dtype=torch.float64)
    assert torch.equal(R.r32(v), want)
    g = torch.Generator().manual_seed(3)
    f = torch.randn(10000, generator=g)
    assert torch.equal(R.r32(f.double()), f.double())


def test_planes_reproduce_the_value_to_sixteen_bits():
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(4, 1000, generator=g) * torch.exp2(torch.randint(-30, 30, (4, 1000), generator=g).float())).double()
    hi, lo = R.planes(x)
    assert torch.equal(hi, R.rb(hi)) and torch.equal(lo, R.rb(lo))
    assert bool(((hi + lo - x).abs() <= 2.0 ** -16 * x.abs()).all())
    assert bool((lo.abs() <= R.bf16_half_step(hi)).all())
    assert torch.equal(hi.float().double() - hi, torch.zeros_like(hi))
    assert torch.equal((x.float() - hi.float()).double(), x - hi)            # x - hi is exact in fp32
    tri = R.split_planes_rounded(x.float(), triple=True)
    assert torch.equal(tri[:, :1000], hi) and torch.equal(tri[:, 1000:2000], hi) and torch.equal(tri[:, 2000:], lo)
    assert float(R.planes_bound(x, torch.zeros_like(x)).max()) <= 2.0 ** -16 * float(x.abs().max())
