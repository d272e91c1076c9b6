"""The fused RNN-T joint + loss on the MI355X (csrc/rnnt_loss.hip through hip_ops.rnnt_joint_loss and
Transducer(transducer_type="fused_joint")).  Every comparison feeds the restated path (TransducerJoint.forward_optimized's
arithmetic + transducer.loss.transducer_loss) the SAME bf16-rounded E, P, W, b, with h = tanh(E + P) rounded to bf16 as the
kernel does, and computes it in fp64 (the rounding passes the gradient straight through: d h / d x = 1 - tanh^2)."""
import copy
import itertools
import math
import warnings

import pytest
import torch

from paper_accurate_fast_cheap_amd.transducer.loss import transducer_loss

pytestmark = pytest.mark.gpu


def _brute(logp, y, blank):
    """-log of the sum over every monotone alignment of T blanks and U labels through the (T, U + 1) lattice."""
    T, U1, _ = logp.shape
    U = U1 - 1
    total = []
    for pos in itertools.combinations(range(T + U), U):
        t = u = 0
        s = 0.0
        ok = True
        for step in range(T + U):
            if step in pos:
                if t >= T:
                    ok = False
                    break
                s += float(logp[t, u, y[u]])
                u += 1
            else:
                s += float(logp[t, u, blank])
                t += 1
        if ok and t == T and u == U:
            total.append(s)
    m = max(total)
    return -(m + math.log(sum(math.exp(v - m) for v in total)))


def _inputs(B, T, Up1, J, V, seed, scale_w=3.0):
    g = torch.Generator().manual_seed(seed)
    E = (torch.randn(B, T, J, generator=g) * 0.6).to(torch.bfloat16)
    P = (torch.randn(B, Up1, J, generator=g) * 0.6).to(torch.bfloat16)
    W = (torch.randn(V, J, generator=g) * scale_w / math.sqrt(J)).to(torch.bfloat16)
    b = (torch.randn(V, generator=g) * 0.5).to(torch.bfloat16)
    return E.cuda(), P.cuda(), W.cuda(), b.cuda()


def _targets(Us, V, blank, seed, pad=-1):
    g = torch.Generator().manual_seed(seed + 1)
    Umax = max(max(Us), 1)
    ys = torch.full((len(Us), Umax), pad, dtype=torch.int64)
    for n, u in enumerate(Us):
        lab = torch.randint(0, V - 1, (u,), generator=g)
        ys[n, :u] = lab + (lab >= blank).to(torch.int64)          # never the blank
    return ys


def _restated_fp64(E, P, W, b, Ts, Us, ys, blank):
    """Per-utterance nll of the restated joint + loss in fp64 on bf16-rounded h (straight-through gradient)."""
    J = E.shape[-1]
    rows = []
    for n, (t, u) in enumerate(zip(Ts, Us)):
        th = torch.tanh(E[n, :t, None, :] + P[n, None, :u + 1, :])
        h = th + (th.to(torch.bfloat16).to(torch.float64) - th).detach()
        rows.append(h.reshape(-1, J))
    logits = torch.cat(rows) @ W.t() + b
    yt = torch.where(ys < 0, 0, ys)
    return transducer_loss(logits, yt, torch.tensor(Ts), torch.tensor(Us), blank, reduction="none")


def _fused(E, P, W, b, Ts, Us, ys, blank, weights=None):
    """nll and the gradients of sum_n weights[n] nll[n] through the kernels (fp32 operands that hold bf16 values)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    Ef, Pf, Wf, bf = (x.float().requires_grad_(True) for x in (E, P, W, b))
    nll = hip_ops.rnnt_joint_loss(Ef, Pf, Wf, bf, torch.tensor(Ts, device="cuda"), ys.cuda(), torch.tensor(Us, device="cuda"), blank)
    wts = torch.ones_like(nll) if weights is None else weights
    (nll * wts).sum().backward()
    return nll.detach(), Ef.grad, Pf.grad, Wf.grad, bf.grad


def _rel_fro(got, want):
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-30))


@pytest.mark.parametrize("blank", [0, 7])
def test_equals_brute_force_enumeration(hip, blank):
    J, V = 64, 40
    cases = [(1, 0), (3, 2), (5, 4), (4, 1), (2, 4), (5, 0)]
    Ts, Us = [c[0] for c in cases], [c[1] for c in cases]
    E, P, W, b = _inputs(len(cases), 5, 5, J, V, seed=11 + blank)
    ys = _targets(Us, V, blank, seed=blank)
    nll = _fused(E, P, W, b, Ts, Us, ys, blank)[0].cpu()
    Wd, bd = W.double(), b.double()
    for n, (T, U) in enumerate(cases):
        h = torch.tanh(E[n, :T, None, :].double() + P[n, None, :U + 1, :].double()).to(torch.bfloat16).double()
        logp = (h @ Wd.t() + bd).log_softmax(-1).cpu()
        want = _brute(logp, ys[n, :U].tolist(), blank)
        assert float(nll[n]) == pytest.approx(want, rel=1e-5), (T, U, float(nll[n]), want)


def test_full_dims_against_fp64_restatement(hip):
    J, V, blank = 640, 5000, 0
    cases = [(1, 0), (37, 5), (120, 40), (200, 60)]
    Ts, Us = [c[0] for c in cases], [c[1] for c in cases]
    E, P, W, b = _inputs(4, 210, 64, J, V, seed=3)                # padded beyond every length
    ys = _targets(Us, V, blank, seed=3)
    wts = torch.tensor([0.5, 1.0, 2.0, 0.25], device="cuda")
    nll, dE, dP, dW, db = _fused(E, P, W, b, Ts, Us, ys, blank, wts)
    Ed, Pd, Wd, bd = (x.double().requires_grad_(True) for x in (E, P, W, b))
    want = _restated_fp64(Ed, Pd, Wd, bd, Ts, Us, ys.cuda(), blank)
    (want * wts.double()).sum().backward()
    rel = ((nll.double() - want.detach()).abs() / want.detach().abs()).max().item()
    assert rel <= 1e-4, (nll.tolist(), want.tolist())
    for name, got, ref in (("dE", dE, Ed.grad), ("dP", dP, Pd.grad), ("dW", dW, Wd.grad), ("db", db, bd.grad)):
        assert torch.isfinite(got).all(), name
        assert _rel_fro(got, ref) <= 1e-2, (name, _rel_fro(got, ref))
    # frames / labels beyond the lengths get no gradient
    assert dE[0, 1:].abs().max() == 0 and dP[0, 1:].abs().max() == 0 and dE[3, 200:].abs().max() == 0


def test_training_size_batch(hip):
    J, V, blank, B = 640, 5000, 0, 32
    g = torch.Generator().manual_seed(7)
    Ts = torch.randint(60, 500, (B,), generator=g).tolist()
    Us = torch.randint(0, 161, (B,), generator=g).tolist()
    Us[5] = 0
    E, P, W, b = _inputs(B, max(Ts), max(Us) + 1, J, V, seed=8)
    ys = _targets(Us, V, blank, seed=8)
    R = sum(t * (u + 1) for t, u in zip(Ts, Us))
    from paper_accurate_fast_cheap_amd import hip_ops
    Ef, Pf, Wf, bf = (x.float().requires_grad_(True) for x in (E, P, W, b))
    hl, yl, yc = torch.tensor(Ts, device="cuda"), torch.tensor(Us, device="cuda"), ys.cuda()

    def run():
        for x in (Ef, Pf, Wf, bf):
            x.grad = None
        nll = hip_ops.rnnt_joint_loss(Ef, Pf, Wf, bf, hl, yc, yl, blank)
        nll.sum().backward()
        return [nll.detach()] + [x.grad.clone() for x in (Ef, Pf, Wf, bf)]

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    first = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    dense = R * V * 4
    assert peak <= 0.25 * dense, (peak / 2**30, dense / 2**30)
    second = run()
    for a, c in zip(first, second):
        assert torch.isfinite(a).all()
        assert torch.equal(a, c)                  # bitwise: no float atomics anywhere
    nll = first[0].cpu()
    rows = [t * (u + 1) for t, u in zip(Ts, Us)]
    picks = {max(range(B), key=lambda n: rows[n]), min(range(B), key=lambda n: rows[n]), 5}
    Wd, bd = W.double(), b.double()
    with torch.no_grad():
        for n in sorted(picks):
            want = _restated_fp64(E[n:n + 1].double(), P[n:n + 1].double(), Wd, bd, Ts[n:n + 1], Us[n:n + 1], ys[n:n + 1].cuda(), blank)
            assert float(nll[n]) == pytest.approx(float(want[0]), rel=1e-4), (n, Ts[n], Us[n])


def test_at_most_one_synchronising_call(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    J, V = 128, 512
    Ts, Us = [30, 17, 9], [6, 0, 3]
    E, P, W, b = _inputs(3, 30, 7, J, V, seed=21)
    ys = _targets(Us, V, 0, seed=21).cuda()
    hl, yl = torch.tensor(Ts, device="cuda"), torch.tensor(Us, device="cuda")
    Ef, Pf, Wf, bf = (x.float().requires_grad_(True) for x in (E, P, W, b))
    hip_ops.rnnt_joint_loss(Ef, Pf, Wf, bf, hl, ys, yl, 0).sum().backward()        # warm-up (binding, allocator)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            hip_ops.rnnt_joint_loss(Ef, Pf, Wf, bf, hl, ys, yl, 0).sum().backward()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    syncs = [w for w in caught if "called a synchronizing" in str(w.message)]
    assert len(syncs) <= 1, [str(w.message) for w in syncs]


def test_transducer_fused_joint_training_step(hip, monkeypatch):
    """Transducer(transducer_type="fused_joint") on the reduced encoder: one bf16-autocast train_step runs the kernels (the
    restated loss is patched to raise), its loss agrees with the default path on the same weights, every parameter gets a
    finite gradient."""
    from tests.conftest import load_golden
    from paper_accurate_fast_cheap_amd.transducer import loss as loss_mod
    from paper_accurate_fast_cheap_amd.transducer import transducer as tr_mod
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    from paper_accurate_fast_cheap_amd.utils.train_utils import train_step
    gd = load_golden("encoder_reduced_bf16slot")
    conf = dict(gd["conf"], dropout_rate=0.0, positional_dropout_rate=0.0)
    torch.manual_seed(1)
    enc = ConformerEncoder(80, **conf)
    V, D, J = 256, enc.output_size(), 64
    fused = tr_mod.Transducer(V, 0, enc, RNNPredictor(V, 32, 48, 0.0, 48, 1, dropout=0.0), TransducerJoint(V, D, 48, J),
                              ctc=CTC(V, D), ctc_weight=0.3, transducer_weight=0.7, transducer_type="fused_joint").cuda()
    default = copy.deepcopy(fused)
    default.fused_joint = False
    gen = torch.Generator().manual_seed(5)
    batch = {"feats": torch.randn(3, 90, 80, generator=gen), "feats_lengths": torch.tensor([90, 71, 50]),
             "target": torch.randint(1, V, (3, 5), generator=gen), "target_lengths": torch.tensor([5, 4, 2])}
    batch["target"][2, 2:] = -1

    info_default = train_step(default, batch, torch.optim.Adam(default.parameters(), lr=1e-4), torch.device("cuda"),
                              grad_clip=5.0, amp_dtype=torch.bfloat16)

    def boom(*a, **k):
        raise AssertionError("the restated transducer loss ran")

    monkeypatch.setattr(loss_mod, "transducer_loss", boom)
    monkeypatch.setattr(tr_mod, "transducer_loss", boom)
    grads = {}
    hooks = [p.register_hook(lambda gr, n=n: grads.__setitem__(n, gr)) for n, p in fused.named_parameters()]
    info = train_step(fused, batch, torch.optim.Adam(fused.parameters(), lr=1e-4), torch.device("cuda"), grad_clip=5.0,
                      amp_dtype=torch.bfloat16)
    for h in hooks:
        h.remove()
    assert torch.isfinite(info["loss"]) and torch.isfinite(info["grad_norm"])
    assert float(info["loss"]) == pytest.approx(float(info_default["loss"]), rel=1e-2)
    missing = [n for n, _ in fused.named_parameters() if n not in grads]
    assert not missing, missing
    assert all(torch.isfinite(v).all() for v in grads.values())
