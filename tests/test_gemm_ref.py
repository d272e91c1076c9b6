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
