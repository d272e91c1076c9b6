"""tests/conv_ref.py checked by itself, on the CPU: the im2col reference is the convolution, the case tables of the GPU battery
(tests/test_conv_sub_f64_gpu.py) meet the conditions they were written for, and on the battery's own inputs a correctly formed
result -- fp32 accumulation, one rounding to the output type -- lies inside gemm_ref.bound while every planted mistake, written
here as a mutated result with no kernel involved, falls outside it."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref, gemm_ref
from tests.conv_ref import C1_CASES, CONV2_CASES, Case, VARIANTS

FAMILIES = ["bf16", "bf16_ph", "f32split", "split_ph"]


@functools.lru_cache(maxsize=None)
def _conv2_union(family):
    seen = []
    for cases in CONV2_CASES[family].values():
        seen += [c for c in cases if c not in seen]
    return seen


# ---- the reference is the operation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T1,F1,Ci,Co", [(1, 3, 3, 5, 4), (2, 8, 10, 3, 7), (3, 12, 39, 4, 6), (2, 7, 12, 6, 2), (1, 9, 5, 1, 8)])
def test_ideal_over_im2col_is_the_float64_convolution(B, T1, F1, Ci, Co):
    g = torch.Generator().manual_seed(T1 * F1)
    ints = lambda *s: torch.randint(-8, 9, s, generator=g).double()      # integers: both sums are exact, whatever their order
    x, w, b = ints(B, T1, F1, Ci), ints(9, Co, Ci), ints(Co)
    ops = {"A": conv_ref.im2col(x), "W": conv_ref.w_matrix(w), "bias": b}
    want = F.conv2d(x.permute(0, 3, 1, 2), w.reshape(3, 3, Co, Ci).permute(2, 3, 0, 1), b, stride=2).permute(0, 2, 3, 1)
    assert want.shape == (B, conv_ref.out_size(T1), conv_ref.out_size(F1), Co)
    for act in ("none", "relu"):
        got = gemm_ref.ideal(gemm_ref.Form(False, "bf16", act, None), ops).reshape(want.shape)
        assert torch.equal(got, F.relu(want) if act == "relu" else want)
    if T1 % 2 == 0:
        x[:, -1] = float("nan")
    if F1 % 2 == 0:
        x[:, :, -1] = float("nan")
    assert torch.equal(conv_ref.im2col(x), ops["A"])                      # the row / column of an even size is in no window


def test_split_construction_is_the_convolution_of_hi_plus_lo_less_the_lo_lo_product():
    case = Case(2, 8, 10, 64, 128)
    ops = conv_ref.make_problem("split", case)
    P, _, Kw = gemm_ref.products(conv_ref.form_of("f32split", 0), ops)
    assert Kw == 27 * 64
    d = lambda k: ops[k].double()
    conv = lambda x, w: F.conv2d(x.permute(0, 3, 1, 2), w.reshape(3, 3, 128, 64).permute(2, 3, 0, 1), stride=2).permute(0, 2, 3, 1)
    want = conv(d("x_hi") + d("x_lo"), d("taps_hi") + d("taps_lo")) - conv(d("x_lo"), d("taps_lo"))
    torch.testing.assert_close(P.reshape(want.shape), want, rtol=0, atol=1e-12)
    # ... and those planes are the fp32 operands to 16 bits
    assert float((conv(d("x_lo"), d("taps_lo")).abs() / conv(d("x_hi").abs(), d("taps_hi").abs())).max()) < 2.0 ** -15


# ---- the tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_conv2_tables_meet_their_conditions(family):
    ph = family.endswith("_ph")
    assert sorted(CONV2_CASES[family]) == ([128, 192, 256] if ph else [128, 256] if family == "bf16" else [128])
    for tile, cases in CONV2_CASES[family].items():
        rows = [conv_ref.rows_of(c) for c in cases]
        for m in (1, tile - 1, tile, tile + 1, 2 * tile + 7):
            assert m in rows, (family, tile, m)
        assert Case(1, 3, 3, *cases[0][3:]) in cases
        geo = {c[:3] for c in cases}
        assert any(t % 2 == 0 and f % 2 == 0 for _, t, f in geo)
        assert any(t % 2 == 0 and f % 2 == 1 for _, t, f in geo) and any(t % 2 == 1 and f % 2 == 0 for _, t, f in geo)
        assert any(f == 39 for _, _, f in geo)
        # a multi-tile case whose tiles start in the middle of a frame and run across batch entries
        assert any(c.B >= 2 and conv_ref.out_size(c.F1) > 1 and tile % conv_ref.out_size(c.F1) and conv_ref.rows_of(c) > tile
                   for c in cases)
        walked = {(c.Ci, c.Co) for c in cases if conv_ref.rows_of(c) == 2 * tile + 7}
        assert {ci for ci, _ in walked} == ({128, 384, 512} if ph else {64, 128, 192, 384, 512})
        assert {co for _, co in walked} == ({8, 264, 384, 512} if ph else {128, 256, 384})
        assert sum(ci != co for ci, co in walked) > len(walked) / 2 and cases[0].Ci != cases[0].Co
        for c in cases:
            assert c.Ci % (128 if ph else 64) == 0 and c.Co % (8 if ph else 128) == 0, c
    if family == "bf16":      # PAFC_CONV_TILE = 4 runs its own kernel only where Co % 256 == 0
        assert sum(c.Co % 256 == 0 for c in CONV2_CASES[family][256]) >= 8


def test_conv1_table_meets_its_conditions():
    assert [C for C in range(1, 4097) if conv_ref.c1_admitted(C)] == [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    assert all(conv_ref.c1_admitted(C) for C in conv_ref.C1_CS) and not conv_ref.c1_admitted(24) and not conv_ref.c1_admitted(4096)
    assert {8, 16, 64, 512, 1024, 2048} == set(conv_ref.C1_CS) == {c.Co for c in C1_CASES}
    for C in conv_ref.C1_CS:
        mine = [c for c in C1_CASES if c.Co == C]
        assert {c.F1 for c in mine} == {3, 4, 23, 80, 83} and {c.T1 for c in mine} == {3, 4, 7, 8, 11} and {c.B for c in mine} == {1, 3}
        ppi = 256 // (C // 8)
        f1s = {conv_ref.out_size(c.F1) for c in mine}
        assert min(f1s) < ppi or ppi == 1
        assert any(f > ppi for f in f1s) or ppi > 41            # (C = 8, 16: one pass covers the widest row, F = 83 -> F1 = 41)
    crossing = [c for c in C1_CASES if c.B == 3]
    assert crossing and all((c.B * conv_ref.out_size(c.T1)) % conv_ref.C1_ROWS for c in crossing)
    assert any(conv_ref.out_size(c.T1) % conv_ref.C1_ROWS for c in crossing)


def test_dispatch_cases_sit_either_side_of_the_count():
    count = lambda c: -(-conv_ref.rows_of(c) // 256) * (c.Co // 256)
    assert count(conv_ref.DISPATCH_BELOW) == 510 and count(conv_ref.DISPATCH_ABOVE) == 512
    assert conv_ref.rows_of(conv_ref.DISPATCH_ABOVE) >= 255 * 256 + 1
    c = conv_ref.DISPATCH_ABOVE
    assert c.B * c.T1 * c.F1 * c.Ci * 2 < 100e6 and c.Co % 256 == 0


def test_grid_problems_are_exact_in_float32():
    """The exact cases of the GPU file: the sums need fewer than 24 bits, fp32 accumulation of the planes in the stored order
    and in a permuted one equals the float64 product bit for bit, and a tap read from the wrong place changes the result
    nearly everywhere."""
    for family, case in conv_ref.GRID_CASES.items():
        form = conv_ref.form_of(family, 0)
        ops = conv_ref.make_problem(conv_ref.FORMS[family][0], case, grid=True)
        assert conv_ref.grid_bits(form, ops) < 23.0, family
        P, _, _ = gemm_ref.products(form, ops)
        pairs, _ = gemm_ref._planes_of(form, ops)
        perm = torch.randperm(pairs[0][0].shape[-1], generator=torch.Generator().manual_seed(3))
        for cols in (slice(None), perm):
            assert torch.equal(sum(a[:, cols].float() @ w[:, cols].float().t() for a, w in pairs).double(), P), family
        want = gemm_ref.ideal(form, ops)
        assert torch.equal((sum(a.float() @ w.float().t() for a, w in pairs) + ops["bias"].float()).double(), want)
        wrong = dict(ops, A=_mutated_a(ops, swap=True))
        wrong.pop("_prod")
        assert float((gemm_ref.round_to(form, gemm_ref.ideal(form, wrong)) != gemm_ref.round_to(form, want)).double().mean()) > 0.9
        if form.a_split:                         # the lo_a hi_w product dropped
            (_, _), (lo, w1), (_, _) = pairs
            assert float((gemm_ref.round_to(form, want - lo @ w1.t()) != gemm_ref.round_to(form, want)).double().mean()) > 0.9


@pytest.mark.parametrize("family", FAMILIES + ["c1_bf16", "c1_f32split"])
def test_every_table_case_fits_the_grid(family):
    """The GPU file runs every case of the tables on grid operands too: each needs fewer than 24 bits, with one to spare."""
    form = conv_ref.form_of(family, 0)
    for case in (C1_CASES if family.startswith("c1") else _conv2_union(family)):
        assert conv_ref.grid_bits(form, conv_ref.make_problem(conv_ref.FORMS[family][0], case, grid=True)) < 23.0, case


# ---- a correct result lies inside the bound, every planted mistake outside it, on every case of the battery ------------------
def _mutated_a(ops, **kw):
    if ops["kind"] == "split":
        return conv_ref.split_a(ops["x_hi"], ops["x_lo"], **kw)
    x = ops["x"]
    return conv_ref.im2col(x if x.dim() == 4 else x.unsqueeze(-1), **kw)


def _epilogue(form, P, bias):
    pre = P if bias is None else P + bias.double()
    return gemm_ref.round_to(form, torch.relu(pre) if form.act == "relu" else pre)


def _ratio(got, form, ops):
    return float(((got - gemm_ref.ideal(form, ops)).abs() / gemm_ref.bound(form, ops)).max())


def _fp32_product(form, ops):
    pairs, _ = gemm_ref._planes_of(form, ops)
    return sum(a.float() @ w.float().t() for a, w in pairs)


def _check_case(family, case):
    """-> the worst err / bound of the correct result over the four (relu, bias) settings, after asserting every mistake"""
    kind = conv_ref.FORMS[family][0]
    ops = conv_ref.make_problem(kind, case)
    form0 = conv_ref.form_of(family, 0)
    P, _, _ = gemm_ref.products(form0, ops)
    acc = _fp32_product(form0, ops)                                       # fp32 accumulation on the CPU
    W = ops["W"].double()
    wrong_p = {"kh and kw swapped": _mutated_a(ops, swap=True).double()}
    if case.T1 % 2 == 0:
        wrong_p["window rows one late"] = _mutated_a(ops, dt=1).double()
    if case.F1 % 2 == 0:
        wrong_p["window columns one late"] = _mutated_a(ops, df=1).double()
    if form0.a_split:
        K = W.shape[-1] // 3
        wrong_p = {k: a[:, :K] @ W[:, :K].t() + a[:, K:] @ W[:, K:2 * K].t() + a[:, :K] @ W[:, 2 * K:].t() for k, a in wrong_p.items()}
        # The bound allows (27 Ci + 8) 2^-24 of |A| |W|^T, which grows with K^2, the dropped product (2^-9 of the operands, random
        # signs) with K^0.5: 8 100 K^-1.5 of the bound per standard deviation, 0.6 at Ci = 64 -- where the largest of some
        # thousand elements is seen -- and 0.03 at Ci = 512.  Beyond Ci = 64 the exact cases see it (as in tests/test_gemm_ref
        # .py, "what the bound cannot see at long K, the grid does"): test_grid_problems_are_exact_in_float32.
        if case.Ci == 64:
            A = ops["A"].double()
            wrong_p["lo_a hi_w dropped"] = P - A[:, K:] @ W[:, K:2 * K].t()
    else:
        wrong_p = {k: a @ W.t() for k, a in wrong_p.items()}
    worst = 0.0
    for relu, with_bias in VARIANTS:
        form, v = conv_ref.variant(family, ops, relu, with_bias)
        b = v["bias"]
        pre = acc if b is None else acc + b.float()
        good = gemm_ref.round_to(form, (torch.relu(pre) if relu else pre).double())
        r = _ratio(good, form, v)
        assert r <= 1.0, (family, case, relu, with_bias, r)
        worst = max(worst, r)
        bad = {k: _epilogue(form, p, b) for k, p in wrong_p.items()}
        if b is not None:
            nb = b.double().clone()
            nb[-min(128, nb.numel()):] = 0.0
            bad["a block of 128 columns without its bias"] = _epilogue(form, P, nb)
            # the bias behind ReLU and a rounding of its own.  (Without ReLU this is the same function rounded twice, which
            # one pixel's few elements need not show: it is planted where the order matters.)
            if relu:
                bad["bias after ReLU, rounded twice"] = gemm_ref.round_to(form, gemm_ref.round_to(form, torch.relu(P)) + b.double())
        if form.out == "planes" and not form.a_split:
            bad["lo plane omitted"] = gemm_ref.ideal(form, v).float().bfloat16().double()
        for k, got in bad.items():
            assert _ratio(got, form, v) > 1.0, (family, case, relu, with_bias, k, _ratio(got, form, v))
    return worst


@pytest.mark.parametrize("family", FAMILIES)
def test_correct_result_inside_and_planted_mistakes_outside_the_bound_conv2(family):
    worst = max(_check_case(family, c) for c in _conv2_union(family))
    print(family, "correct result: worst err / bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("family", ["c1_bf16", "c1_f32split"])
def test_correct_result_inside_and_planted_mistakes_outside_the_bound_conv1(family):
    worst = max(_check_case(family, c) for c in C1_CASES)
    print(family, "correct result: worst err / bound", worst)
    assert worst <= 1.0
