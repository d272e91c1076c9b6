"""The float64 references of tests/ssd_ref.py against each other, on the CPU: the written-out backward of the Mamba-2 scan
(what csrc/mamba2_scan_bwd.hip evaluates) equals autograd of the sequential recurrence, and the suffix sums that form g_la on
the kernel tests' inputs do not cancel beyond what those tests' bound allows for."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ssd_ref

# (B, L, H) of tests/test_mamba_train_gpu.py's kernel cases
KERNEL_SHAPES = [(1, 1, 1), (2, 13, 2), (2, 45, 3), (2, 83, 3), (1, 64, 1)]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("B,L,H", [(1, 1, 1), (2, 13, 2), (2, 45, 2)])
def test_closed_forms_equal_float64_autograd(B, L, H, reverse):
    xbc, dt, la, gy = ssd_ref.make_inputs(B, L, H, seed=5)
    ref = ssd_ref.autograd_grads(xbc, dt, la, gy, H, reverse)
    got = ssd_ref.closed_forms(xbc, dt, la, gy, H, reverse)
    for k in ("y", "g_x", "g_B", "g_C", "g_dt", "g_la"):
        assert float((got[k] - ref[k]).abs().max()) <= 1e-10, k
    assert float((got["g_la_suffix"] - ref["g_la"]).abs().max()) <= 1e-10


def test_reverse_is_the_flipped_recurrence():
    xbc, dt, la, gy = ssd_ref.make_inputs(2, 13, 2, seed=6)
    fl = lambda t: torch.flip(t, [1])
    a = ssd_ref.autograd_grads(xbc, dt, la, gy, 2, reverse=True)
    b = ssd_ref.autograd_grads(fl(xbc), fl(dt), fl(la), fl(gy), 2)
    for k in a:
        assert torch.equal(a[k], fl(b[k])), k


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("B,L,H", KERNEL_SHAPES)
def test_g_la_cancellation_scale_of_the_kernel_inputs(B, L, H, reverse):
    """The kernel tests bound g_la's error by 2e-4 * S, S = max sum_s (|gy_s . y_s| + |dt_s g_dt_s|): that bound says something
    about g_la only while S stays within 64 x max |g_la|.  (L = 1 has no such ratio: the first step decays the empty state,
    g_la_0 = a_0 <G_0, h_{-1}> = 0 identically, the two terms of the sum cancel exactly; there the reference must say zero.)"""
    _, _, _, _, ref, S = ssd_ref.kernel_case(B, L, H, reverse)
    first = ref["g_la"][:, -1 if reverse else 0]
    assert float(first.abs().max()) <= 1e-12 * S
    if L > 1:
        assert S <= 64 * float(ref["g_la"].abs().max()), (S, float(ref["g_la"].abs().max()))


def test_chain_reaches_every_parameter():
    """mamba2_chain restates transformer/mamba2.py with the module's parameter names (the module's own scan needs the GPU: the two
    are compared in tests/test_mamba_train_gpu.py); here: its shapes, and a gradient for every parameter."""
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2
    torch.manual_seed(2)
    m = Mamba2(128, headdim=64)
    params = {k: v.detach().double().requires_grad_() for k, v in m.named_parameters()}
    u = torch.randn(1, 9, 128, dtype=torch.float64)
    out = ssd_ref.mamba2_chain(params, u)
    assert out.shape == (1, 9, 128)
    out.sum().backward()
    for k, v in params.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and float(v.grad.abs().max()) > 0, k


# ---- the forward scan's references and acceptance rule (tests/test_mamba_kernels_gpu.py) -------------------------------------

RECIPES = ["mid", "slow", "fast"]


@functools.lru_cache(maxsize=None)
def _fwd_case(recipe, reverse=False):
    """B = 2, L = 83, H = 3 (three 32-step chunks, the last block partial): inputs, float64 y and yabs."""
    xbc, dt, la, _ = ssd_ref.make_inputs(2, 83, 3, seed=31, recipe=recipe)
    x, Bm, Cm = ssd_ref.split_xbc(xbc, 3)
    y = ssd_ref.scan_seq(x, Bm, Cm, dt.double(), la.double(), reverse)
    yabs = ssd_ref.abs_scan(x, Bm, Cm, dt.double(), la.double(), reverse)
    return xbc, dt, la, y, yabs


@pytest.mark.parametrize("recipe", RECIPES)
def test_recipes_stay_in_their_ranges(recipe):
    (d0, d1), (a0, a1) = ssd_ref.RECIPES[recipe]
    _, dt, la, _ = ssd_ref.make_inputs(2, 83, 3, seed=31, recipe=recipe)
    assert d0 <= float(dt.min()) and float(dt.max()) <= d1
    A = -la / dt
    assert a0 - 1e-4 <= float(A.min()) and float(A.max()) <= a1 + 1e-4
    if recipe == "fast":          # sixteen steps of it underflow fp32: e^{cum_15} = 0 in the kernel
        assert float(la.max()) <= -8 and 16 * float(la.max()) < math.log(2.0 ** -149)


def test_mid_recipe_is_the_backward_tests_recipe():
    """The default recipe draws what it drew before it had a name (tests/test_mamba_train_gpu.py's inputs)."""
    g = torch.Generator().manual_seed(5)
    xbc = (torch.randn(2, 13, 2 * 64 + 256, generator=g) * 0.5).to(torch.bfloat16)
    dt = torch.rand(2, 13, 2, generator=g) * 0.2 + 0.01
    la = -dt * (torch.rand(2, generator=g) * 8 + 0.5)
    got = ssd_ref.make_inputs(2, 13, 2, seed=5)
    assert torch.equal(got[0], xbc) and torch.allclose(got[1], dt, rtol=1e-6, atol=0) and torch.allclose(got[2], la, rtol=1e-6, atol=0)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("recipe", RECIPES)
def test_abs_scan_dominates_the_scan(recipe, reverse):
    xbc, dt, la, _ = ssd_ref.make_inputs(2, 37, 2, seed=32, recipe=recipe)
    x, Bm, Cm = ssd_ref.split_xbc(xbc, 2)
    h0 = torch.randn(2, 2, 128, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(33))
    for h in (None, h0):
        y, hT = ssd_ref.scan_seq(x, Bm, Cm, dt.double(), la.double(), reverse, h0=h, return_state=True)
        yabs, habs = ssd_ref.abs_scan(x, Bm, Cm, dt.double(), la.double(), reverse, h0=h, return_state=True)
        assert bool((yabs >= y.abs()).all()) and bool((habs >= hT.abs()).all())
        assert bool((yabs > 0).all())


@pytest.mark.parametrize("reverse", [False, True])
def test_state_carry_splits_the_sequence(reverse):
    """scan(whole) == scan(first part) then scan(second part from the first's final state); reverse walks from the right."""
    xbc, dt, la, _ = ssd_ref.make_inputs(2, 29, 2, seed=34)
    ops = (*ssd_ref.split_xbc(xbc, 2), dt.double(), la.double())
    y, hT = ssd_ref.scan_seq(*ops, reverse, return_state=True)
    cut = 12
    first, second = (slice(cut, None), slice(0, cut)) if reverse else (slice(0, cut), slice(cut, None))
    ya, ha = ssd_ref.scan_seq(*(t[:, first] for t in ops), reverse, return_state=True)
    yb, hb = ssd_ref.scan_seq(*(t[:, second] for t in ops), reverse, h0=ha, return_state=True)
    assert float((y[:, first] - ya).abs().max()) <= 1e-12 and float((y[:, second] - yb).abs().max()) <= 1e-12
    assert float((hT - hb).abs().max()) <= 1e-12


@pytest.mark.parametrize("recipe", RECIPES)
def test_fp32_recurrence_passes_scan_accept(recipe):
    """The bound is not within fp32 noise: the recurrence run in fp32 passes with room (its error over yabs is about 2e-7)."""
    xbc, dt, la, y, yabs = _fwd_case(recipe)
    x, Bm, Cm = ssd_ref.split_xbc(xbc, 3, torch.float32)
    got = ssd_ref.scan_seq(x, Bm, Cm, dt, la)
    ssd_ref.scan_accept(got, y, yabs, name=f"ssd_ref fp32 recurrence[{recipe}]", recipe=recipe)
    assert float(((got.double() - y).abs() / yabs).max()) <= 2.0 ** -20


@pytest.mark.parametrize("recipe", RECIPES)
def test_scan_accept_is_not_vacuous(recipe):
    """2^-13 yabs against the largest output of the same (batch, head): at most 0.1 % at the median element, 1 % at the worst."""
    _, _, _, y, yabs = _fwd_case(recipe)
    rel = ssd_ref.SCAN_REL * yabs / y.abs().amax((1, 3), keepdim=True)
    assert float(rel.median()) <= 1e-3 and float(rel.max()) <= 1e-2, (float(rel.median()), float(rel.max()))


def _wrong_candidates(recipe):
    """Three subtly wrong scans built from the float64 reference."""
    xbc, dt, la, y, _ = _fwd_case(recipe)
    x, Bm, Cm = ssd_ref.split_xbc(xbc, 3)
    no_diag = y - (Bm * Cm).sum(-1).view(2, 83, 1, 1) * dt.double().unsqueeze(-1) * x       # the s = t term dropped
    tail = y.clone()
    tail[:, 80:] = 0                       # chunks of 32: the last chunk's last, partial 16-step block (steps 80 .. 82) zeroed
    scaled = y.clone()
    scaled[:, :, 1] *= 1 + 2.0 ** -10      # one head's output scaled
    return {"no_diag": no_diag, "tail": tail, "scaled": scaled}


@pytest.mark.parametrize("which", ["no_diag", "tail", "scaled"])
@pytest.mark.parametrize("recipe", RECIPES)
def test_scan_accept_refuses_wrong_candidates(recipe, which):
    _, _, _, y, yabs = _fwd_case(recipe)
    ssd_ref.scan_accept(y.clone(), y, yabs, name="ssd_ref exact", recipe=recipe)
    with pytest.raises(AssertionError):
        ssd_ref.scan_accept(_wrong_candidates(recipe)[which], y, yabs, name=f"ssd_ref wrong[{recipe}-{which}]", recipe=recipe)


def test_scan_accept_bf16_interval():
    """The interval form: the rounding of any value within tol passes, a value one bf16 step beyond the interval does not."""
    xbc, dt, la, y, yabs = _fwd_case("mid")
    x, _, _ = ssd_ref.split_xbc(xbc, 3)
    D = torch.tensor([0.7, -1.3, 0.2], dtype=torch.float64).view(1, 1, 3, 1)
    ref, tol = y + D * x, ssd_ref.SCAN_REL * (yabs + (D * x).abs())
    for shift in (-1.0, 0.0, 1.0):
        ssd_ref.scan_accept_bf16((ref + shift * tol).float().to(torch.bfloat16), ref, tol, name="ssd_ref bf16 interval")
    hi = (ref + tol).float().to(torch.bfloat16)
    beyond = torch.where(hi.float() > 0, hi.float() * (1 + 2.0 ** -6), hi.float()).to(torch.bfloat16)    # at least one bf16 step up
    assert bool((beyond.double() > hi.double()).any())
    with pytest.raises(AssertionError):
        ssd_ref.scan_accept_bf16(beyond, ref, tol, name="ssd_ref bf16 beyond")
    with pytest.raises(AssertionError):
        ssd_ref.scan_accept_bf16((y).float().to(torch.bfloat16), ref, tol, name="ssd_ref bf16 no skip term")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_glue_references_restate_the_module(dtype):
    """gate_norm_ref / finish_ref / prep_ref / conv_silu_ref against the framework lines of transformer/mamba2.py on the CPU."""
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import RMSNormGated
    g = torch.Generator().manual_seed(40)
    Bsz, L, H = 2, 5, 2
    di = H * 64
    tol = dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else dict(rtol=2.0 ** -7, atol=1e-3)
    y = torch.randn(Bsz, L, di, generator=g).to(dtype)
    z = (torch.randn(Bsz, L, di, generator=g) * 3).to(dtype)
    norm = RMSNormGated(di).to(dtype)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(di, generator=g) + 0.5)
        want = norm(y, z)
    got = ssd_ref.gate_norm_ref(y, z, norm.weight.detach(), norm.eps, dtype)
    torch.testing.assert_close(got.float(), want.float(), **tol)
    # conv: F.conv1d with the module's padding, keep the first L
    C, K = 12, 4
    x = torch.randn(Bsz, L, C, generator=g).to(dtype)
    w, b = (torch.randn(C, 1, K, generator=g) * 0.4).to(dtype), (torch.randn(C, generator=g) * 0.1).to(dtype)
    conv = lambda t: F.silu(F.conv1d(t.float().transpose(1, 2), w.float(), b.float(), padding=K - 1, groups=C)[..., :t.shape[1]].transpose(1, 2))
    torch.testing.assert_close(ssd_ref.conv_silu_ref(x, w, b, dtype).float(), conv(x), **tol)
    torch.testing.assert_close(ssd_ref.conv_silu_ref(x, w, b, dtype, reverse=True).float(), torch.flip(conv(torch.flip(x, [1])), [1]), **tol)
    whole = ssd_ref.conv_silu_ref(x, w, b, dtype)
    part = ssd_ref.conv_silu_ref(x[:, 3:], w, b, dtype, prefix=x[:, :3])
    assert torch.equal(part, whole[:, 3:])
    # prep: the lines of Mamba2.forward
    xbc = (torch.randn(Bsz, L, di + 256, generator=g) * 0.5).to(dtype)
    dt_raw = (torch.randn(Bsz, L, H, generator=g) * 2).to(dtype)
    dt_bias, A_log = torch.randn(H, generator=g), torch.rand(H, generator=g)
    r0, r1, k0, k1, v, wl = ssd_ref.prep_ref(xbc, dt_raw, dt_bias, A_log, di)
    dt = F.softplus(dt_raw.float() + dt_bias)
    logdec = dt * -torch.exp(A_log)
    nxt = torch.cat([logdec[:, 1:], torch.zeros_like(logdec[:, :1])], dim=1)
    f32 = dict(rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(v.float(), (xbc[..., :di].float().view(Bsz, L, H, 64) * dt.unsqueeze(-1)).reshape(Bsz, L, di), **f32)
    torch.testing.assert_close(wl.float().view(Bsz, L, H, 64)[..., 0], torch.log((-nxt).clamp_min(1e-30)), **f32)
    torch.testing.assert_close(k1.float().view(Bsz, L, H, 64), torch.exp(nxt).unsqueeze(-1) * xbc[..., di + 64:di + 128].float().unsqueeze(2), **f32)
    assert torch.equal(r0.view(Bsz, L, H, 64)[:, :, 1], xbc[..., di + 128:di + 192].double())
    assert torch.equal(k0[:, -1].view(Bsz, H, 64)[:, 0], xbc[:, -1, di:di + 64].double())           # a_next = 1 at the last step
    # finish with the s = t term == the scan's own output + D x, gated and normed: chain the references
    x, Bm, Cm = ssd_ref.split_xbc(xbc, H)
    la = (dt * -torch.exp(A_log)).double()
    yfull = ssd_ref.scan_seq(x, Bm, Cm, dt.double(), la).reshape(Bsz, L, di)
    ydiag = ((Bm * Cm).sum(-1).view(Bsz, L, 1, 1) * dt.double().unsqueeze(-1) * x).reshape(Bsz, L, di)
    D = torch.randn(H, generator=g)
    a = ssd_ref.finish_ref((yfull - ydiag).float(), None, xbc, dt_raw, z, dt_bias, D, norm.weight.detach(), 1e-5, di, True, dtype)
    b = ssd_ref.finish_ref(yfull.float(), None, xbc, dt_raw, z, dt_bias, D, norm.weight.detach(), 1e-5, di, False, dtype)
    torch.testing.assert_close(a.float(), b.float(), **tol)
    with torch.no_grad():
        want = norm((yfull + (x * D.double().view(1, 1, H, 1)).reshape(Bsz, L, di)).float().to(dtype), z)
    torch.testing.assert_close(b.float(), want.float(), **tol)
