"""The float64 references of tests/ssd_ref.py against each other, on the CPU: the written-out backward of the Mamba-2 scan
(what csrc/mamba2_scan_bwd.hip evaluates) equals autograd of the sequential recurrence, and the suffix sums that form g_la on
the kernel tests' inputs do not cancel beyond what those tests' bound allows for."""
import pytest
import torch

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
