"""Training the Conformer baseline's slot on the GPU: LimitedRelPositionMultiHeadedAttention with `trainable` set, in fp32
against float64 autograd through the restatement (tests/lca_ref.py) and under bf16 autocast, and a two-layer baseline
ConformerEncoder in training mode.

Bound of the fp32 module test, per gradient: 8 x the error of float32 CPU autograd through the restatement against float64
autograd on the same case, the module bound of tests/test_lca_encoder_gpu.py."""
import pytest
import torch

from tests import lca_ref, parity_log, synth
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

W, B, T = 16, 2, 67


def _module(g, w):
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    m = WENET_ATTENTION_CLASSES["limited_rel_selfattn"](g["heads"], g["d"], 0.1, True, [w, w], 0, 1, False, 0)   # (dropout: a no-op in eval)
    m.load_state_dict(synth.synth_state_dict(g["spec"], g["weight_seed"]), strict=True)
    m.trainable = True                                   # what ConformerEncoder sets on the slots it builds
    return m.cuda().eval()


def _cpu_grads(g, c, dtype):
    """Gradients of sum(out * dy) through the restatement in `dtype` on the CPU: {"x" | parameter name: gradient}."""
    sd = {k: v.to(dtype).requires_grad_(True) for k, v in synth.synth_state_dict(g["spec"], g["weight_seed"]).items()}
    x = synth.randn((B, T, g["d"]), c["seed"]).to(dtype).requires_grad_(True)
    dy = synth.randn((B, T, g["d"]), c["seed"] + 500).to(dtype)
    y, _ = lca_ref.lca_attention(x, g["pos_rows"][:, :T].to(dtype), sd, g["heads"], W)
    names = sorted(sd)
    grads = torch.autograd.grad((y * dy).sum(), [x] + [sd[k] for k in names])
    return dict(zip(["x"] + names, grads))


def _case(g):
    return next(c for c in g["cases"] if (c["w"], c["B"], c["T"]) == (W, B, T))


def test_trainable_module_fp32_against_float64_autograd(hip):
    g = load_golden("lca_attention")
    c = _case(g)
    m = _module(g, W)
    x = synth.randn((B, T, g["d"]), c["seed"]).cuda()
    dy = synth.randn((B, T, g["d"]), c["seed"] + 500).cuda()
    pos = g["pos_rows"][:, :T].cuda()
    mask = torch.ones(B, 1, T, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        y0, cache0 = m(x, x, x, mask, pos)
    xg = x.clone().requires_grad_(True)
    y, cache = m(xg, xg, xg, mask, pos)
    assert y.requires_grad and torch.equal(y, y0) and torch.equal(cache, cache0)          # the no-grad output, bit for bit
    (y * dy).sum().backward()
    torch.cuda.synchronize()
    want, cpu = _cpu_grads(g, c, torch.float64), _cpu_grads(g, c, torch.float32)
    got = {"x": xg.grad}
    got.update({k: p.grad for k, p in m.named_parameters()})
    assert set(got) == set(want)
    failures = []
    for k in sorted(want):
        assert got[k] is not None and got[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        ek = (got[k].double().cpu() - want[k]).abs().max().item()
        ec = (cpu[k].double() - want[k]).abs().max().item()
        print(f"lca train fp32 {k}: max|err| {ek:.3e}, float32 CPU restatement {ec:.3e}, ratio {ek / ec if ec else float('inf'):.2f}")
        parity_log.record(f"lca_train_fp32_{k}", max_abs_err=ek, cpu_float32_err=ec)
        if not (ec > 0 and ek <= 8 * ec):
            failures.append((k, ek, ec))
    assert not failures, failures


def test_trainable_module_under_bf16_autocast(hip):
    """fp32 master weights under autocast(bfloat16): the kernel runs in bf16 with the biases cast.  Every gradient is finite, of
    its parameter's dtype and shape.  No bound for a bf16 stack against the float64 gradients of the fp32 weights is derived
    here (the kernel's own bf16 bound is in tests/test_mha_band_bwd_gpu.py), so the differences are recorded, not asserted."""
    g = load_golden("lca_attention")
    c = _case(g)
    m = _module(g, W)
    x = synth.randn((B, T, g["d"]), c["seed"]).cuda().requires_grad_(True)
    dy = synth.randn((B, T, g["d"]), c["seed"] + 500).cuda()
    pos = g["pos_rows"][:, :T].cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y, _ = m(x, x, x, torch.ones(B, 1, T, dtype=torch.bool, device="cuda"), pos)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, T, g["d"])
    (y.float() * dy).sum().backward()
    torch.cuda.synchronize()
    want = _cpu_grads(g, c, torch.float64)
    got = {"x": x.grad}
    got.update({k: p.grad for k, p in m.named_parameters()})
    for k in sorted(want):
        assert got[k] is not None and got[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        assert torch.isfinite(got[k]).all(), k
        parity_log.record(f"lca_train_bf16_autocast_{k}", max_abs_diff=(got[k].double().cpu() - want[k]).abs().max().item(),
                          ref_abs_max=want[k].abs().max().item())


def test_two_layer_baseline_encoder_trains(hip):
    """The encoder_lca golden's configuration in training mode, B = 2 with 160 input frames: a sum-of-outputs loss gives every
    parameter a finite, non-zero gradient; the no-grad forward afterwards still carries its earlier bits; and the backward of an
    encoder-built slot lists no library GEMM kernel under torch.profiler (rocBLAS / hipBLASLt "Cijk_", at::native gemm / gemv,
    aten::mm / addmm / bmm), the attention running in the mha_band_bwd kernels."""
    from torch.profiler import ProfilerActivity, profile
    from paper_accurate_fast_cheap_amd.transformer.cmvn import GlobalCMVN
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_lca")
    enc = ConformerEncoder(80, global_cmvn=GlobalCMVN(torch.zeros(80), torch.ones(80)), **g["conf"])
    enc.load_state_dict(synth.synth_state_dict(g["spec"], g["seed"]))
    enc = enc.cuda().eval()
    xs, lens = synth.randn((2, 160, 80), 11, 2.0).cuda(), torch.tensor([160, 120]).cuda()
    with torch.no_grad():
        before, _ = enc(xs, lens)
    enc.train()
    torch.manual_seed(3)
    out, _ = enc(xs, lens)
    assert out.requires_grad and tuple(out.shape) == tuple(before.shape)
    out.sum().backward()
    torch.cuda.synchronize()
    for name, p in enc.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        assert torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, name
    enc.zero_grad(set_to_none=True)
    enc.eval()
    with torch.no_grad():
        after, _ = enc(xs, lens)
    assert torch.equal(after, before)

    slot = enc.encoders[0].self_attn
    assert slot.trainable
    Tp, D = before.shape[1], before.shape[2]
    h = synth.randn((2, Tp, D), 12).cuda().requires_grad_(True)
    pos = lca_ref.position_rows(0, Tp, D, torch.float32).cuda()
    mask = torch.ones(2, 1, Tp, dtype=torch.bool, device="cuda")
    slot(h, h, h, mask, pos)[0].sum().backward()                                            # (warm: library load)
    y, _ = slot(h, h, h, mask, pos)
    loss = y.sum()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        loss.backward()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    for kernel in ("mha_band_bwd_dq_kernel", "mha_band_bwd_dkv_kernel", "mha_band_bwd_reduce_kernel"):
        assert any(kernel in n for n in names), (kernel, names)
    bad = [n for n in names if "Cijk_" in n or ("gemm" in n.lower() and "at::native" in n)
           or n in ("aten::mm", "aten::addmm", "aten::bmm")]
    assert not bad, bad


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
def test_linear_own_fp32_against_float64(hip, bias):
    """hip_ops.linear_own in an fp32 model outside autocast: the forward carries linear_fused's bits, and y, dX, dW and db are
    held element by element to the bound of a length-n fp32 sum of exact products in ANY order (Higham, Accuracy and Stability
    of Numerical Algorithms, section 3.1): |err| <= (n + 2) 2^-24 (sum_k |a_k b_k| + |bias|), n the length of the reduction
    (K for y, N for dX, the rows R for dW and db).  R = 2 * 67 is no multiple of 4, so dW runs on zero-padded transposed copies;
    N = 136 is no multiple of a tile."""
    from paper_accurate_fast_cheap_amd import hip_ops
    Bq, Tq, K, N = 2, 67, 128, 136
    R, u = Bq * Tq, 2.0 ** -24
    x64 = synth.randn((Bq, Tq, K), 21).double()
    w64 = (synth.randn((N, K), 22) * K ** -0.5).double()
    b64 = (synth.randn((N,), 23) * 0.3).double() if bias else None
    dy64 = synth.randn((Bq, Tq, N), 24).double()
    x, w = x64.float().cuda().requires_grad_(True), w64.float().cuda().requires_grad_(True)
    b = b64.float().cuda().requires_grad_(True) if bias else None
    y = hip_ops.linear_own(x, w, b)
    assert type(y.grad_fn).__name__ == "_LinearOwnF32Backward"                       # the package's GEMM, not F.linear
    with torch.no_grad():
        assert torch.equal(y, hip_ops.linear_fused(x, w, b, "none", split_ok=False))
    y.backward(dy64.float().cuda())
    torch.cuda.synchronize()
    x2, dy2 = x64.reshape(R, K), dy64.reshape(R, N)
    checks = [("y", y.detach().reshape(R, N), x2 @ w64.T + (b64 if bias else 0),
               (K + 2) * u * (x2.abs() @ w64.abs().T + (b64.abs() if bias else 0))),
              ("dx", x.grad.reshape(R, K), dy2 @ w64, (N + 2) * u * (dy2.abs() @ w64.abs())),
              ("dw", w.grad, dy2.T @ x2, (R + 2) * u * (dy2.abs().T @ x2.abs()))]
    if bias:
        checks.append(("db", b.grad, dy2.sum(0), (R + 2) * u * dy2.abs().sum(0)))
    for name, got, want, bound in checks:
        assert got.dtype == torch.float32 and got.shape == want.shape, name
        err = (got.double().cpu() - want).abs()
        parity_log.record(f"linear_own_fp32_{name}_{'bias' if bias else 'no_bias'}", max_abs_err=err.max().item(),
                          max_err_over_bound=(err / bound).max().item())
        assert bool((err <= bound).all()), (name, err.max().item(), (err / bound).max().item())
