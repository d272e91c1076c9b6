"""tests/gemm_ref.py checked by itself, on the CPU: the float64 reference and the derived bound the GPU tests of
csrc/gemm_ph.hip and csrc/gemm_bf16.hip hold the kernels to.  The reference must be the operation, a correct result must
lie inside the bound, and three wrong kernels -- written here as mutated results, no kernel involved -- must fall outside it."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref
from tests.gemm_ref import FORMS, Form

M, K = 71, 384


def _ops(name, seed=7, **kw):
    form = FORMS[name]
    N = 256 if form.act == "glu" else 264
    kw.setdefault("alpha", 0.5 if form.res else 1.0)
    return form, gemm_ref.make_operands(form, M, N, K, seed, **kw)


def _outside(got, form, ops):
    return float(((got - gemm_ref.ideal(form, ops)).abs() > gemm_ref.bound(form, ops)).double().mean())


@pytest.mark.parametrize("plane_block", [0, 128])
def test_split_ideal_is_the_fp32_product_to_sixteen_bits(plane_block):
    form, ops = _ops("split-f32", plane_block=plane_block)
    P, _, Kw = gemm_ref.products(form, ops)
    a, w = ops["a32"].double(), ops["w32"].double()
    assert Kw == 3 * K
    assert bool(((P - a @ w.t()).abs() <= 2.0 ** -15 * (a.abs() @ w.abs().t())).all())
    hi, lo = gemm_ref.split_hi_lo(ops["a32"])
    assert bool(((hi.double() + lo.double() - a).abs() <= 2.0 ** -16 * a.abs()).all())


def test_glu_and_epilogue_order_are_the_modules():
    """GLU over interleaved blocks of 32 = F.glu of the plain Linear; the residual is added AFTER the activation."""
    form = FORMS["bf16-glu"]
    ops = gemm_ref.make_operands(form, M, 256, K, 3)
    plain = F.glu(F.linear(ops["A"].double(), ops["W"].double(), ops["bias"].double()), dim=-1)
    inter = dict(ops, W=gemm_ref.glu_interleave(ops["W"]), bias=gemm_ref.glu_interleave(ops["bias"]))
    inter.pop("_prod", None)
    torch.testing.assert_close(gemm_ref.ideal(form, inter), plain, rtol=1e-12, atol=1e-12)
    form = Form(False, "bf16", "silu", "bf16")
    ops = gemm_ref.make_operands(form, M, 264, K, 4, alpha=0.5)
    lin = 0.5 * (ops["A"].double() @ ops["W"].double().t()) + ops["bias"].double()
    torch.testing.assert_close(gemm_ref.ideal(form, ops), F.silu(lin) + ops["residual"].double(), rtol=1e-12, atol=1e-12)


def test_rows_and_batches_are_slices_of_one_reference():
    form = FORMS["split-f32-res"]
    ops = gemm_ref.make_operands(form, M, 264, K, 5, batch=2, alpha=0.5)
    want, bnd = gemm_ref.ideal(form, ops), gemm_ref.bound(form, ops)
    part = gemm_ref.rows(ops, 33)
    assert torch.equal(gemm_ref.ideal(form, part), want[:, :33]) and torch.equal(gemm_ref.bound(form, part), bnd[:, :33])
    one = {k: (v[1] if isinstance(v, torch.Tensor) else v) for k, v in ops.items() if k != "_prod"}
    torch.testing.assert_close(gemm_ref.ideal(form, one), want[1], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_correctly_rounded_ideal_lies_inside_the_bound(name):
    """The bound cannot fail by itself: `ideal` rounded ONCE to the output type is inside it, everywhere, for every form --
    and the bound is finite and a small fraction of the values it guards."""
    form, ops = _ops(name)
    want, bnd = gemm_ref.ideal(form, ops), gemm_ref.bound(form, ops)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(bnd).all()) and bool((bnd > 0).all())
    assert _outside(gemm_ref.round_to(form, want), form, ops) == 0.0
    assert float(bnd.max()) < {"bf16": 0.05, "planes": 2e-3, "f32": 2e-3}[form.out]


def test_half_a_bf16_step_is_two_to_the_minus_eight_of_the_value():
    """Why the bf16 term is 2^-8 |x| and not 2^-9 |x|: half a step is 2^-8 of the binade's lower end.  One correct rounding
    of x = 1 + 2^-8 + 2^-20 is more than 2^-9 x off, and on the test inputs a quarter of the correctly rounded values are."""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    err = (x.float().bfloat16().double() - x).abs()
    assert 2.0 ** -9 * x < err <= 2.0 ** -8 * x
    form, ops = _ops("bf16")
    want = gemm_ref.ideal(form, ops)
    E = gemm_ref.bound(form, ops) - 2.0 ** -8 * want.abs()        # (everything but the rounding term, a little more)
    off = (gemm_ref.round_to(form, want) - want).abs() > 2.0 ** -9 * want.abs() + E
    assert float(off.double().mean()) > 0.10


def test_activation_term_is_torch_float32_against_float64():
    form, ops = _ops("split-planes-silu")
    t = gemm_ref.activation_term(form, ops)
    assert 0.0 < t < 1e-5
    assert gemm_ref.activation_term(*_ops("bf16-relu")) == 0.0 and gemm_ref.activation_term(*_ops("f32")) == 0.0
    bnd = gemm_ref.bound(form, ops)
    assert torch.equal(bnd, gemm_ref.bound(form, ops, act_term=t)) and bool((bnd >= t).all())


# ---- a deliberately wrong kernel fails: mutated results, each outside the bound on more than 1 % of the elements --------
def test_a_second_rounding_is_seen():
    """bf16 output with a bf16 residual, rounded before AND after the residual add."""
    form, ops = _ops("bf16-res")
    pre = gemm_ref.pre_activation(form, ops)
    twice = (pre.float().bfloat16().float() + ops["residual"].float()).bfloat16().double()
    assert _outside(twice, form, ops) > 0.01
    form, ops = _ops("split-bf16-res")
    pre = gemm_ref.pre_activation(form, ops)
    twice = (pre.float().bfloat16().float() + ops["residual"].float()).bfloat16().double()
    assert _outside(twice, form, ops) > 0.01


@pytest.mark.parametrize("name", ["split-f32", "split-f32-res", "split-planes-silu", "split-bf16"])
def test_a_dropped_lo_plane_product_is_seen(name):
    form, ops = _ops(name)
    Kk = K
    A, W = ops["A"].double(), ops["W"].double()
    P = A[:, :Kk] @ W[:, :Kk].t() + A[:, :Kk] @ W[:, 2 * Kk:].t()            # hi hi_w + hi lo_w: lo hi_w is missing
    mut = dict(ops, _prod=(P, ops.get("_prod", (None, None, None))[1], 3 * Kk))
    got = gemm_ref.round_to(form, gemm_ref.ideal(form, mut))
    ops.pop("_prod", None)
    assert _outside(got, form, ops) > 0.01


@pytest.mark.parametrize("name", ["split-f32-res", "bf16-res", "f32-res"])
def test_a_bias_scaled_by_alpha_is_seen(name):
    form, ops = _ops(name)
    assert ops["alpha"] == 0.5
    P, _, _ = gemm_ref.products(form, ops)
    got = gemm_ref.round_to(form, 0.5 * (P + ops["bias"].double()) + ops["residual"].double())
    assert _outside(got, form, ops) > 0.9


# ---- the forms of the small tiles (csrc/gemm_bf16.hip) and the grid operands their K walk is held to, bit for bit ---------
from tests.gemm_ref import GLU64_HALF, SMALL_TILE_FORMS  # noqa: E402


def _small_ops(name, seed=11):
    form = SMALL_TILE_FORMS[name]
    ops = gemm_ref.make_operands(form, M, 256 if form.act == "glu" else 264, K, seed, alpha=0.5 if form.res else 1.0)
    if form.act == "glu":
        ops["glu_half"] = GLU64_HALF
    return form, ops


@pytest.mark.parametrize("name", sorted(SMALL_TILE_FORMS))
def test_correctly_rounded_ideal_lies_inside_the_bound_small_tile_forms(name):
    form, ops = _small_ops(name)
    want, bnd = gemm_ref.ideal(form, ops), gemm_ref.bound(form, ops)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(bnd).all()) and bool((bnd > 0).all())
    assert _outside(gemm_ref.round_to(form, want), form, ops) == 0.0
    assert float(bnd.max()) < {"bf16": 0.05, "planes": 2e-3, "f32": 2e-3}[form.out]


def test_glu_over_blocks_of_64_and_activation_before_the_residual():
    form, ops = _small_ops("bf16-glu64")
    plain = F.glu(F.linear(ops["A"].double(), ops["W"].double(), ops["bias"].double()), dim=-1)
    inter = dict(ops, W=gemm_ref.glu_interleave(ops["W"], 64), bias=gemm_ref.glu_interleave(ops["bias"], 64))
    inter.pop("_prod", None)
    torch.testing.assert_close(gemm_ref.ideal(form, inter), plain, rtol=1e-12, atol=1e-12)
    assert not torch.allclose(gemm_ref.ideal(form, dict(inter, glu_half=32)), plain, rtol=1e-3, atol=1e-3)
    form, ops = _small_ops("split-f32-silu-res")
    P, _, _ = gemm_ref.products(form, ops)
    torch.testing.assert_close(gemm_ref.ideal(form, ops), F.silu(0.5 * P + ops["bias"].double()) + ops["residual"].double(),
                               rtol=1e-12, atol=1e-12)


GRID_K1 = [64, 1088, 3264]


def _grid(split, K1, **kw):
    form = FORMS["split-f32-res" if split else "f32-res"]
    return form, gemm_ref.make_grid_operands(form, 70, 264, K1, seed=K1 + split, alpha=0.5, **kw)


def _fp32_sum(pairs, cols=None):
    """The product accumulated in float32 (columns `cols` of every plane pair, in that order), read back as float64."""
    acc = 0
    for a, w in pairs:
        a, w = (a, w) if cols is None else (a[:, cols], w[:, cols])
        acc = acc + a.float() @ w.float().t()
    return acc.double()


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("K1", GRID_K1)
def test_grid_operands_are_exact_in_float32_in_any_order(K1, split):
    """Every partial sum of the grid operands is an fp32 number: a float32 product walked in a permuted column order, or in
    four K shares added afterwards, equals the float64 one bit for bit -- and the bits needed stay below 24."""
    form, ops = _grid(split, K1)
    P, _, Kw = gemm_ref.products(form, ops)
    pairs, _ = gemm_ref._planes_of(form, ops)
    assert Kw == (3 * K1 if split else K1)
    assert 10.0 < gemm_ref.grid_bits(form, ops) < 22.0
    perm = torch.randperm(K1, generator=torch.Generator().manual_seed(K1))
    assert torch.equal(_fp32_sum(pairs), P) and torch.equal(_fp32_sum(pairs, perm), P)
    shares = sum(_fp32_sum(pairs, perm[s::4]).float() for s in range(4)).double()
    assert torch.equal(shares, P)
    want = gemm_ref.ideal(form, ops)
    f32 = torch.addcmul(ops["bias"], _fp32_sum(pairs).float(), torch.tensor(0.5)) + ops["residual"]
    assert torch.equal(f32.double(), want) and torch.equal(gemm_ref.round_to(form, want), want)


def _changed(form, ops, P_wrong):
    mut = dict(ops, _prod=(P_wrong,) + tuple(ops["_prod"][1:]))
    return float((gemm_ref.ideal(form, mut) != gemm_ref.ideal(form, ops)).double().mean())


@pytest.mark.parametrize("plane_block", [0, 64])
@pytest.mark.parametrize("K1", GRID_K1)
def test_a_wrong_k_walk_changes_the_grid_result_nearly_everywhere(K1, plane_block):
    """What the bound cannot see at long K, the grid does: one dropped 64-column K-step (of the hi or of the lo segment), a
    dropped K share (a quarter of the walk) and a lo plane read as hi each change at least 90 % of the elements."""
    form, ops = _grid(True, K1, plane_block=plane_block)
    P, _, _ = gemm_ref.products(form, ops)
    (hi, w0), (lo, w1), (_, w2) = gemm_ref._planes_of(form, ops)[0]
    step = slice(K1 - 64, K1)
    assert _changed(form, ops, P - hi[:, step] @ w0[:, step].t()) >= 0.9
    assert _changed(form, ops, P - lo[:, step] @ w1[:, step].t()) >= 0.9
    assert _changed(form, ops, P - hi[:, step] @ w2[:, step].t()) >= 0.9
    walk = torch.cat([hi, lo, hi], dim=1), torch.cat([w0, w1, w2], dim=1)
    per = -(-(3 * K1 // 64) // 4) * 64
    for s in range(min(4, 3 * K1 // 64)):                   # (K1 = 64: three K-steps, three shares of one)
        share = slice(s * per, min((s + 1) * per, 3 * K1))
        assert _changed(form, ops, P - walk[0][:, share] @ walk[1][:, share].t()) >= 0.9
    assert _changed(form, ops, P - lo @ w1.t() + hi @ w1.t()) >= 0.9
    form, ops = _grid(False, K1)
    P, _, _ = gemm_ref.products(form, ops)
    A, W = ops["A"].double(), ops["W"].double()
    assert _changed(form, ops, P - A[:, :64] @ W[:, :64].t()) >= 0.9


def test_every_grid_shape_of_the_small_tile_tests_is_exact():
    """The GPU file's grid cases (tests/test_gemm_small_tiles_gpu.py: grid_problems), each (form, N, K, plane block) at the
    largest row count it is used with: the generator's precondition holds (make_grid_operands asserts it), with a bit to spare."""
    from tests import test_gemm_small_tiles_gpu as T
    rows = {}
    for name, M, N, K, pb, alpha in T.grid_problems(cus=256):
        rows[(name, N, K, pb, alpha)] = max(M, rows.get((name, N, K, pb, alpha), 0))
    assert len(rows) >= 20
    for (name, N, K, pb, alpha), M in rows.items():
        form = T.form_of(name)
        ops = gemm_ref.make_grid_operands(form, M, N, K, seed=1, plane_block=pb, alpha=alpha)
        assert gemm_ref.grid_bits(form, ops) < 23.0, (name, M, N, K)


# ---- fp32 operands and the activation after the residual (csrc/gemm_f32.hip; tests/test_gemm_f32_f64_gpu.py) ---------------
F32_RES = Form(False, "f32", "none", "f32")


def _f32_ops(K, act="none", n=263, seed=5):
    form = Form(False, "f32", act, "f32")
    ops = gemm_ref.make_operands(form, n, n, K, seed, alpha=0.5, f32_operands=True)
    ops["act_after_residual"] = True
    return form, ops


def _ratio(got, form, ops):
    return float(((got - gemm_ref.ideal(form, ops)).abs() / gemm_ref.bound(form, ops)).max())


@pytest.mark.parametrize("K", [4, 36, 100, 384])
def test_fp32_operand_constant_holds_float32_torch_and_sees_a_wrong_kernel(K):
    """c = (2 Kw + 8) u for fp32 operands, derived, not fitted: the same product in float32 torch stays below 0.15 of the
    bound on 263 x 263 outputs, while a dropped last quad of K and a bias placed under alpha each put more than 99 % of the
    elements outside it."""
    form, ops = _f32_ops(K)
    assert ops["A"].dtype == torch.float32 and ops["W"].dtype == torch.float32
    assert gemm_ref.accumulation_constant(ops, K) == (2 * K + 8) * gemm_ref.U32
    A, W, b, r = ops["A"], ops["W"], ops["bias"], ops["residual"]
    f32 = (0.5 * (A @ W.t()) + b + r).double()
    assert _ratio(f32, form, ops) < 0.15
    P, _, _ = gemm_ref.products(form, ops)
    Ad, Wd = A.double(), W.double()
    dropped = 0.5 * (P - Ad[:, K - 4:] @ Wd[:, K - 4:].t()) + b.double() + r.double()
    assert _outside(gemm_ref.round_to(form, dropped), form, ops) > 0.99
    under = 0.5 * (P + b.double()) + r.double()
    assert _outside(gemm_ref.round_to(form, under), form, ops) > 0.99


@pytest.mark.parametrize("act", ["silu", "tanh", "relu"])
def test_activation_after_the_residual_is_a_switch(act):
    form, ops = _f32_ops(36, act, n=71)
    P, _, _ = gemm_ref.products(form, ops)
    lin = 0.5 * P + ops["bias"].double()
    fn = {"silu": F.silu, "tanh": torch.tanh, "relu": torch.relu}[act]
    torch.testing.assert_close(gemm_ref.ideal(form, ops), fn(lin + ops["residual"].double()), rtol=1e-12, atol=1e-12)
    before = dict(ops, act_after_residual=False)
    torch.testing.assert_close(gemm_ref.ideal(form, before), fn(lin) + ops["residual"].double(), rtol=1e-12, atol=1e-12)
    assert bool(torch.isfinite(gemm_ref.bound(form, ops)).all())
    assert _outside(gemm_ref.round_to(form, gemm_ref.ideal(form, ops)), form, ops) == 0.0


def test_grid_operands_as_fp32_are_the_same_integers_and_batches_stack():
    form = F32_RES
    bf = gemm_ref.make_grid_operands(form, 70, 264, 128, seed=3, alpha=0.5)
    f32 = gemm_ref.make_grid_operands(form, 70, 264, 128, seed=3, alpha=0.5, f32_operands=True)
    assert f32["A"].dtype == torch.float32 and torch.equal(f32["A"], bf["A"].float()) and torch.equal(f32["W"], bf["W"].float())
    assert torch.equal(f32["bias"], bf["bias"]) and torch.equal(f32["residual"], bf["residual"])
    ops = gemm_ref.make_grid_operands(form, 33, 40, 100, seed=4, alpha=0.5, f32_operands=True, batch=3, shared_bias=True)
    assert ops["A"].shape == (3, 33, 100) and ops["bias"].shape == (40,)
    want = gemm_ref.ideal(form, ops)
    one = {k: (v[2] if isinstance(v, torch.Tensor) and v.dim() == 3 else v) for k, v in ops.items() if k != "_prod"}
    assert torch.equal(gemm_ref.ideal(form, one), want[2])
    big = gemm_ref.make_grid_operands(form, 263, 263, 1028, seed=1, alpha=0.5, f32_operands=True)
    assert gemm_ref.grid_bits(form, big) < 20.0


def _cached_f32_problem():
    from tests import test_gemm_f32_f64_gpu as T
    import functools

    @functools.lru_cache(maxsize=None)
    def get(M, N, K, grid, batch):
        return T.make_ops("none", M, N, K, grid, batch, False, "cpu")
    return T, get


def _drop_last_quad(ops):
    P, Sp, Kw = ops["_prod"]
    A, W = ops["A"].double(), ops["W"].double()
    return dict(ops, _prod=(P - A[..., Kw - 4:] @ W[..., Kw - 4:].transpose(-1, -2), Sp, Kw))


def test_planted_faults_fail_the_random_cases_of_the_fp32_gemm_tests():
    """The random case list of tests/test_gemm_f32_f64_gpu.py, with two wrong kernels written as mutated results: the
    activation applied before the residual, and one K quad dropped.  In every family (tile edge x activation) each fault it
    applies to puts more than half of the elements of at least one case outside the bound; a correctly rounded result none."""
    T, get = _cached_f32_problem()
    quad, order = {}, {}
    for act, M, N, K, batch, bias, res in T.random_problems():
        form = Form(False, "f32", act, "f32" if res else None)
        ops = T.variant(get(M, N, K, False, batch), bias, res)
        assert _outside(gemm_ref.round_to(form, gemm_ref.ideal(form, ops)), form, ops) == 0.0
        fam = (M, act)
        got = gemm_ref.round_to(form, gemm_ref.ideal(form, _drop_last_quad(ops)))
        quad[fam] = max(quad.get(fam, 0.0), _outside(got, form, ops))
        if res and act != "none":
            got = gemm_ref.round_to(form, gemm_ref.ideal(form, dict(ops, act_after_residual=False)))
            order[fam] = max(order.get(fam, 0.0), _outside(got, form, ops))
    assert len(quad) == 12 and len(order) == 9
    assert min(quad.values()) > 0.5, quad
    assert min(order.values()) > 0.5, order


def test_planted_faults_change_the_grid_cases_of_the_fp32_gemm_tests():
    """The grid case list of tests/test_gemm_f32_f64_gpu.py: the generator's precondition holds with bits to spare, fp32
    accumulation gives the float64 value bit for bit, and a dropped K quad changes more than half of the elements of EVERY
    problem."""
    T, get = _cached_f32_problem()
    rows = {}
    for M, N, K, batch, alpha in T.grid_problems(cus=256):
        assert alpha in (0.5, 1.0)
        rows[(N, K, batch)] = max(M, rows.get((N, K, batch), 0))
    assert len(rows) >= 60
    for (N, K, batch), M in rows.items():
        batch = min(batch, 8)                    # (the plan's batches of one small tile per CU: eight entries of them)
        ops = get(M, N, K, True, batch)
        form = F32_RES
        assert gemm_ref.grid_bits(form, ops) < 20.0, (M, N, K)
        want = gemm_ref.ideal(form, ops)
        f32 = torch.baddbmm(ops["residual"], ops["A"], ops["W"].transpose(-1, -2), alpha=0.5) if batch else \
            torch.addmm(ops["residual"], ops["A"], ops["W"].t(), alpha=0.5)
        f32 = f32 + (ops["bias"].unsqueeze(-2) if batch else ops["bias"])
        assert torch.equal(f32.double(), want) and torch.equal(gemm_ref.round_to(form, want), want)
        assert float((gemm_ref.ideal(form, _drop_last_quad(ops)) != want).double().mean()) > 0.5, (M, N, K)


# ---- the transposed product (csrc/gemm_tn.hip; tests/test_gemm_tn_f64_gpu.py) --------------------------------------------
def test_tn_plan_arithmetic_and_rounding_count():
    assert [gemm_ref.tn_plan(577, s) for s in range(1, 6)] == [(1, 640), (2, 320), (3, 256), (4, 192), (5, 128)]
    assert gemm_ref.tn_plan(129, 2) == (2, 128) and gemm_ref.tn_plan(1, 1) == (1, 64) and gemm_ref.tn_plan(300, 2) == (2, 192)
    dy, x = gemm_ref.make_tn_operands(300, 136, 72, seed=1)
    form, ops_w, ops_b = gemm_ref.tn_problem(dy, x, "f32", 2, 192)
    assert form == Form(False, "f32", "none", None) and ops_w["roundings"] == 192 + 1 + 2 + 1
    assert gemm_ref.accumulation_constant(ops_w, 300) == 196 * gemm_ref.U32
    torch.testing.assert_close(gemm_ref.ideal(form, ops_w), dy.double().t() @ x.double(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(gemm_ref.ideal(form, ops_b)[:, 0], dy.double().sum(0), rtol=1e-13, atol=1e-13)
    assert gemm_ref.products(form, ops_w)[2] == 300


def test_planted_faults_fail_the_cases_of_the_tn_tests():
    """The case list of tests/test_gemm_tn_f64_gpu.py with two wrong kernels: the last row of R left out of dW, and the bias
    gradient taken over one row too few.  Random operands: each puts more than half of the elements of at least one case
    outside the bound, for both output types (and float32 torch, split as the plan splits, stays inside it).  Grid
    operands: each changes more than half of the elements of at least one case of every family, and a correctly rounded
    result is what round_to gives back."""
    from tests import test_gemm_tn_f64_gpu as T
    fams = {"ring": T.cases_ring_fills(), "splits": T.cases_splits(), "columns": T.cases_column_walk(),
            "renumbering": T.cases_renumbering(), "batched": T.cases_batched(), "random": T.cases_random()}
    assert sum(len(v) for v in fams.values()) == len(T.all_cases())
    for fam, cases in fams.items():
        worst = {}
        for case in cases:
            dy, x = T.make(case, "cpu")
            S, rps = T.expected_S(case)
            for out in ("f32", "bf16"):
                form, ops_w, ops_b = gemm_ref.tn_problem(dy, x, out, S, rps)
                _, short_w, short_b = gemm_ref.tn_problem(dy[..., :-1, :], x[..., :-1, :], out, S, rps)
                for what, ops, short in (("dw", ops_w, short_w), ("dbias", ops_b, short_b)):
                    want = gemm_ref.round_to(form, gemm_ref.ideal(form, ops))
                    got = gemm_ref.round_to(form, gemm_ref.ideal(form, short))
                    if case.grid:
                        assert gemm_ref.grid_bits(form, ops) < 20.0
                        if out == "f32":
                            assert torch.equal(want, gemm_ref.ideal(form, ops))
                        frac = float((got != want).double().mean())
                    else:
                        assert _outside(want, form, ops) == 0.0
                        parts = [ops["A"][..., s * rps:(s + 1) * rps].float() @ ops["W"][..., s * rps:(s + 1) * rps].float().transpose(-1, -2)
                                 for s in range(S)]
                        assert _ratio(gemm_ref.round_to(form, sum(parts).double()), form, ops) <= 1.0
                        frac = _outside(got, form, ops)
                    worst[(what, out)] = max(worst.get((what, out), 0.0), frac)
        assert len(worst) == 4 and min(worst.values()) > 0.5, (fam, worst)
