"""Training the Mamba-2 slot: the SSD scan's backward kernel (csrc/mamba2_scan_bwd.hip) against float64 autograd of the
sequential recurrence, its argument checks, and the gradients of the module and of an encoder that contains it."""
import ctypes

import pytest
import torch

from tests import parity_log, ssd_ref, synth

pytestmark = pytest.mark.gpu

# (B, L, H, chunk_len): one step; under one block; blocks with a partial last one; three chunks with a partial last block; four
# one-block chunks
CASES = [(1, 1, 1, 0), (2, 13, 2, 0), (2, 45, 3, 0), (2, 83, 3, 32), (1, 64, 1, 16)]
BF16_ULP = 2.0 ** -7          # one unit in the last place of a bf16 value in [1, 2)


def _check_kernel(name, B, L, H, chunk_len, reverse, ldx=None):
    from paper_accurate_fast_cheap_amd import hip_ops
    xbc, dt, la, gy, ref, S = ssd_ref.kernel_case(B, L, H, bool(reverse), ldx)
    g_xbc, g_dt, g_la = hip_ops.mamba2_scan_backward(xbc.cuda(), dt.cuda(), la.cuda(), gy.cuda(), H, bool(reverse), chunk_len)
    assert g_xbc.dtype == torch.bfloat16 and g_xbc.shape == xbc.shape and g_dt.shape == g_la.shape == dt.shape
    d = H * 64
    g_xbc = g_xbc.cpu()
    got = dict(g_x=g_xbc[..., :d].double().view(B, L, H, 64), g_B=g_xbc[..., d:d + 128].double(),
               g_C=g_xbc[..., d + 128:d + 256].double(), g_dt=g_dt.cpu().double(), g_la=g_la.cpu().double())
    if ldx:
        assert not g_xbc[..., d + 256:].any()          # the padding columns of a wider row carry no gradient
    ratio = {}
    for k in ("g_x", "g_B", "g_C", "g_dt"):
        scale = float(ref[k].abs().max())
        ratio[k] = float((got[k] - ref[k]).abs().max()) / scale
    ratio["g_la"] = float((got["g_la"] - ref["g_la"]).abs().max()) / S
    parity_log.record(name, **{"err_over_ref_" + k: v for k, v in ratio.items()})
    print(name, ratio)
    # 2e-4 of the output's largest reference value: the forward kernel's bound for the same arithmetic against float64
    assert ratio["g_dt"] <= 2e-4, ratio
    # g_B, g_C: summed over the heads in fp32 and rounded to bf16 once: one bf16 ulp of the largest reference value on top
    assert ratio["g_B"] <= 2e-4 + BF16_ULP, ratio
    assert ratio["g_C"] <= 2e-4 + BF16_ULP, ratio
    # g_x leaves the kernel in bf16 as well (one rounding of dt gxu): every element must be the rounding of a value within
    # 2e-4 max|ref| of the reference, i.e. lie between the roundings of the interval's ends
    tol = 2e-4 * float(ref["g_x"].abs().max())
    lo, hi = (ref["g_x"] - tol).float().to(torch.bfloat16).double(), (ref["g_x"] + tol).float().to(torch.bfloat16).double()
    assert bool(((got["g_x"] >= lo) & (got["g_x"] <= hi)).all()), ratio
    # g_la: the same per-product bound carried through the suffix sum, S = max sum_s (|gy_s . y_s| + |dt_s g_dt_s|)
    assert ratio["g_la"] <= 2e-4, ratio


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("B,L,H,chunk_len", CASES)
def test_scan_backward_kernel_vs_float64(hip, B, L, H, chunk_len, reverse):
    _check_kernel(f"mamba2_scan_bwd[{B}-{L}-{H}-{chunk_len}-{reverse}]", B, L, H, chunk_len, reverse)


def test_scan_backward_kernel_padded_rows(hip):
    """ldx = ldg = H * 64 + 256 + 64: rows wider than [x | B | C]."""
    _check_kernel("mamba2_scan_bwd[padded]", 2, 45, 3, 0, 0, ldx=3 * 64 + 256 + 64)


def test_scan_backward_argument_checks(hip):
    """Bad arguments answer with an error code before anything is launched."""
    B, L, H = 1, 32, 2
    ldx = H * 64 + 256
    dev = "cuda"
    xbc = torch.zeros(B, L, ldx, dtype=torch.bfloat16, device=dev)
    dt, la = torch.zeros(B, L, H, device=dev), torch.zeros(B, L, H, device=dev)
    gy = torch.zeros(B, L, H * 64, device=dev)
    g_xbc, g_dt, g_la = torch.zeros_like(xbc), torch.zeros_like(dt), torch.zeros_like(la)
    nws = hip.pafc_mamba2_scan_bwd_workspace_bytes(B, L, H, 16)
    assert nws > hip.pafc_mamba2_scan_bwd_workspace_bytes(B, L, H, 0) > 0
    ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(gy_p=P(gy), ld=ldx, nbytes=nws):
        return hip.pafc_mamba2_scan_backward(B, L, H, P(xbc), ld, P(dt), P(la), gy_p, P(g_xbc), ldx, P(g_dt), P(g_la), 0, 16,
                                             P(ws), nbytes, None)
    assert call(gy_p=None) == -1                     # PAFC_ERR_NULL_POINTER
    assert call(nbytes=nws - 4) == -4                # PAFC_ERR_WORKSPACE
    assert call(ld=H * 64 + 252) == -2               # PAFC_ERR_BAD_DIMS: the row is shorter than [x | B | C]
    assert call() == 0
    torch.cuda.synchronize()
    assert not g_xbc.any() and not g_dt.any() and not g_la.any()      # zero gradient in, zero gradients out


def _grads(m, u, w):
    m.zero_grad(set_to_none=True)
    u = u.detach().clone().requires_grad_()
    out = m(u)
    (out.float() * w).sum().backward()
    g = {k: v.grad.detach().double().clone() if v.grad is not None else None for k, v in m.named_parameters()}
    g["input"] = u.grad.detach().double().clone()
    return out.detach(), g


@pytest.mark.parametrize("kind", ["uni", "bi"])
def test_module_gradients_bf16(hip, monkeypatch, kind):
    """bf16 module: every parameter -- A_log and dt_bias included -- gets a gradient, and each gradient is as close to the one
    taken through a float64 recurrence (b) as the fp32 recurrence's own gradient (a) is, everything but the scan shared:
        |g_kernel - g_b| <= 4 |g_a - g_b| + 2^-8 |g_b|   per tensor
    (4: room for bf16 rounding flips downstream of a 2^-16 against a 2^-24 product error; 2^-8: one bf16 ulp)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2, Mamba2Bidirectional
    torch.manual_seed(7)
    m = (Mamba2 if kind == "uni" else Mamba2Bidirectional)(128, headdim=64).bfloat16().cuda().train()
    u = synth.randn((2, 45, 128), 21).to(torch.bfloat16).cuda()
    w = synth.randn((2, 45, 128), 22).cuda()
    _, gk = _grads(m, u, w)
    for k, v in gk.items():
        assert v is not None, f"{k}: no gradient"
        assert torch.isfinite(v).all() and float(v.abs().max()) > 0, k
    ref = {}
    for tag, dtype in (("a", torch.float32), ("b", torch.float64)):
        monkeypatch.setattr(hip_ops, "mamba2_scan_train",
                            lambda xbc, dt, la, H, reverse=False, dtype=dtype: ssd_ref.scan_xbc(xbc, dt, la, H, reverse, dtype).float())
        _, ref[tag] = _grads(m, u, w)
    monkeypatch.undo()
    worst = 0.0
    for k in gk:
        dk, da, nb = float((gk[k] - ref["b"][k]).norm()), float((ref["a"][k] - ref["b"][k]).norm()), float(ref["b"][k].norm())
        print(kind, k, "kernel-b", dk, "a-b", da, "|b|", nb)
        worst = max(worst, dk / (4 * da + 2.0 ** -8 * nb))
        assert dk <= 4 * da + 2.0 ** -8 * nb, (k, dk, da, nb)
    parity_log.record(f"mamba2_module_grads_bf16[{kind}]", worst_over_bound=worst)


def test_module_gradients_fp32(hip):
    """fp32 parameters (the YAML's precision for this slot): the scan runs on the WKV-6 kernels, whose backward carries the
    gradient.  All gradients against the float64 chain of tests/ssd_ref.py, at the figures of
    test_mamba_slot_matches_sequential_recurrence; the forward is the one the op-by-op inference route computes, bit for bit."""
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2
    torch.manual_seed(8)
    m = Mamba2(128, headdim=64).cuda().train()
    u = synth.randn((1, 21, 128), 23).cuda()
    w = synth.randn((1, 21, 128), 24).cuda()
    out, g = _grads(m, u, w)
    with torch.no_grad():
        m.fused_inference = False
        plain = m(u)
        m.fused_inference = True
    assert torch.equal(out, plain)
    params = {k: v.detach().double().cpu().requires_grad_() for k, v in m.named_parameters()}
    u64 = u.double().cpu().requires_grad_()
    ref_out = ssd_ref.mamba2_chain(params, u64)
    (ref_out * w.double().cpu()).sum().backward()
    torch.testing.assert_close(out.cpu(), ref_out.detach().float(), rtol=2e-3, atol=2e-4)
    for k, v in params.items():
        assert g[k] is not None, f"{k}: no gradient"
        torch.testing.assert_close(g[k].cpu().float(), v.grad.float(), rtol=2e-3, atol=2e-4, msg=lambda s, k=k: f"{k}: {s}")
    torch.testing.assert_close(g["input"].cpu().float(), u64.grad.float(), rtol=2e-3, atol=2e-4)


def test_encoder_training_step_bf16_autocast(hip):
    """One training step of a two-layer bidirectional mamba_att encoder under bf16 autocast with a CTC loss."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    torch.manual_seed(9)
    enc = ConformerEncoder(80, output_size=128, attention_heads=2, linear_units=256, num_blocks=2, input_layer="conv2d",
                           cnn_module_kernel=31, cnn_module_norm="layer_norm", activation_type="swish",
                           pos_enc_layer_type="rel_pos", selfattention_layer_type="mamba_att", rnn_att_version="mamba2",
                           rnn_att_direction="bi").cuda().train()
    head = torch.nn.Linear(128, 16).cuda()
    xs, lens = synth.randn((2, 99, 80), 1).cuda(), torch.tensor([99, 60]).cuda()
    ys, ylens = torch.tensor([[3, 5, 7, 2], [4, 9, 0, 0]]).cuda(), torch.tensor([4, 2]).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out, mask = enc(xs, lens)
        logp = head(out).float().log_softmax(-1)
    loss = torch.nn.functional.ctc_loss(logp.transpose(0, 1), ys, mask.squeeze(1).sum(1), ylens, blank=0, reduction="sum")
    loss.backward()
    assert torch.isfinite(loss)
    for k, v in list(enc.named_parameters()) + list(head.named_parameters()):
        assert v.grad is not None, f"{k}: no gradient"
        assert torch.isfinite(v.grad).all(), k
    for layer in enc.encoders:
        for blk in (layer.self_attn.mamba.mamba_forward, layer.self_attn.mamba.mamba_backward):
            assert float(blk.A_log.grad.abs().max()) > 0 and float(blk.dt_bias.grad.abs().max()) > 0
