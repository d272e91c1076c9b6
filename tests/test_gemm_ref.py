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
