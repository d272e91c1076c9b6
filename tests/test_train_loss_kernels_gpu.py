"""The training step's CTC loss (csrc/ctc_loss.hip) and first-convolution weight gradient (csrc/conv_sub.hip) against float64
references of the same operations on the same values, through their C entry points, at the shapes and edges where they branch:
every lattice width, both logit dtypes, large vocabularies, non-zero blanks, infeasible utterances, padded strides, NaN
poison outside what may be read, ragged row blocks and more partial blocks than the reduce has slices.  Bounds come from
torch's own fp32 error on the same input (CTC) or from the kernel's summation order (conv1), and each is shown to see a
one-frame, one-label or one-block error."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


# ---- CTC loss ----------------------------------------------------------------------------------------------------------------

def _labels(n, reps, V, blank, g):
    """n labels in [0, V) without blank, with exactly `reps` adjacent repeats."""
    rep_at = set((torch.randperm(n - 1, generator=g)[:reps] + 1).tolist()) if n > 1 else set()
    out = []
    for j in range(n):
        if j in rep_at:
            out.append(out[-1])
            continue
        while True:
            c = int(torch.randint(0, V, (1,), generator=g))
            if c != blank and (not out or c != out[-1]):
                break
        out.append(c)
    return out


def _ctc_batch(Lmax, V, blank, seed, T=None):
    """Rows: (L, repeats, T_b).  Every batch mixes a full row, L = 0, T_b = 1, a tight row (T_b = L + repeats: one alignment),
    the same one frame short (L <= T_b, infeasible inside the lattice), L > T_b (the early-out) and rows with T_b < T."""
    g = torch.Generator().manual_seed(seed)
    T = T or Lmax + Lmax // 4 + 3
    h = max(2, Lmax // 2)
    rows = [(Lmax, Lmax // 8, T), (0, 0, T // 2 + 1), (1, 0, 1), (h, h // 3, h + h // 3), (h, max(1, h // 3), h + max(1, h // 3) - 1),
            (Lmax, 0, Lmax - 1), (Lmax // 3, Lmax // 6, T - 5), (Lmax // 4, Lmax // 8, T // 2 + 2)]
    B = len(rows)
    ys = torch.full((B, Lmax), -1, dtype=torch.long)
    ys[:, 1::3] = V + 7                                             # junk beyond ylens: -1 and values >= V
    ylens, hlens = [], []
    for b, (n, reps, tb) in enumerate(rows):
        assert 1 <= tb <= T and n <= Lmax
        ys[b, :n] = torch.tensor(_labels(n, reps, V, blank, g), dtype=torch.long)
        ylens.append(n)
        hlens.append(tb)
    return T, ys, torch.tensor(ylens), torch.tensor(hlens), g


def _ctc_call(hip_ops, logits, B, T, V, hlens, ys, ylens, blank, grad_out, scale, ldg, Lmax=None):
    """pafc_ctc_loss_forward + _backward on the current stream, exactly as _CtcHeadLoss calls them, with explicit strides;
    nll and dlogits are prefilled with NaN over their whole extent."""
    from paper_accurate_fast_cheap_amd import _lib
    L = hip_ops._bind_ctc_loss()
    dev = logits.device
    Lmax = ys.shape[1] if Lmax is None else Lmax
    hl = hlens.to(dev, torch.int32).contiguous()
    yl = ylens.to(dev, torch.int32).contiguous()
    ysd = ys.to(dev, torch.int64).contiguous()
    code = _lib.dtype_code(logits.dtype)
    nbytes = L.pafc_ctc_loss_workspace_bytes(B, T, Lmax)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nll = torch.full((B,), float("nan"), device=dev)
    st = _lib.stream_of(logits)
    _lib.check(L.pafc_ctc_loss_forward(code, B, T, V, _lib.ptr(logits), logits.stride(0), _lib.ptr(hl), _lib.ptr(ysd), ysd.stride(0),
                                       _lib.ptr(yl), Lmax, blank, _lib.ptr(nll), _lib.ptr(ws), nbytes, st), "pafc_ctc_loss_forward")
    dl = torch.full((B * T, ldg), float("nan"), dtype=logits.dtype, device=dev)
    gf = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    _lib.check(L.pafc_ctc_loss_backward(code, B, T, V, _lib.ptr(logits), logits.stride(0), _lib.ptr(hl), _lib.ptr(ysd), ysd.stride(0),
                                        _lib.ptr(yl), Lmax, blank, _lib.ptr(nll), _lib.ptr(gf), scale, _lib.ptr(dl), ldg, _lib.ptr(ws),
                                        nbytes, st), "pafc_ctc_loss_backward")
    return nll, dl


def _ctc_ref(z, ys, ylens, hlens, blank, gscale, dtype):
    """torch on the CPU in `dtype` (float64: the reference; float32: the rounding yardstick): per-utterance nll with
    zero_infinity and d(gscale * sum nll) / d logits through log_softmax."""
    zz = z.to(dtype).requires_grad_()
    lp = zz.log_softmax(-1).transpose(0, 1)
    nll = F.ctc_loss(lp, ys, hlens, ylens, blank=blank, reduction="none", zero_infinity=True)
    (nll.sum() * gscale).backward()
    return nll.detach().double(), zz.grad.double()


def _poisoned_logits(z, hlens, ldl, dtype):
    """(B T, ldl) device logits holding z, NaN in columns [V, ldl) and in rows t >= hlens[b]."""
    B, T, V = z.shape
    buf = torch.full((B, T, ldl), float("nan"), dtype=dtype)
    buf[:, :, :V] = z.to(dtype)
    for b, tb in enumerate(hlens.tolist()):
        buf[b, tb:] = float("nan")
    return buf.reshape(B * T, ldl).cuda()


def _check_ctc(hip_ops, z, ys, ylens, hlens, blank, dtype, grad_out=0.75, scale=0.37, ldl_pad=24, ldg_pad=40):
    """Run the kernels on z (B, T, V) (fp32 values exact in `dtype`) and compare with the float64 reference under bounds
    set by torch's fp32 error.  Returns (nll, float64 nll, the loss bound per utterance, which utterances have an alignment)."""
    B, T, V = z.shape
    ldl, ldg = V + ldl_pad, V + ldg_pad
    assert ldl != ldg and ldg > V
    gs = grad_out * scale
    nll, dl = _ctc_call(hip_ops, _poisoned_logits(z, hlens, ldl, dtype), B, T, V, hlens, ys, ylens, blank, grad_out, scale, ldg)
    nll, dl = nll.cpu().double(), dl.cpu().double().view(B, T, ldg)
    ys_t = ys.clamp(0, V - 1)                                    # (torch is handed clean padding; the kernel gets the junk)
    n64, g64 = _ctc_ref(z, ys_t, ylens, hlens, blank, gs, torch.float64)
    n32, g32 = _ctc_ref(z, ys_t, ylens, hlens, blank, gs, torch.float32)
    # poison stays out: finite everywhere, exact zeros where nothing may be written but zeros
    assert torch.isfinite(nll).all() and torch.isfinite(dl).all()
    assert (dl[:, :, V:] == 0).all()
    lp64 = z.double().log_softmax(-1).transpose(0, 1)
    raw = F.ctc_loss(lp64, ys_t, hlens, ylens, blank=blank, reduction="none", zero_infinity=False)
    feasible = torch.isfinite(raw)
    for b in range(B):
        assert (dl[b, hlens[b]:] == 0).all(), b
        if not feasible[b]:
            assert nll[b] == 0 and (dl[b] == 0).all(), b
    # loss per utterance
    e_k, e_t = (nll - n64).abs(), (n32 - n64).abs()
    bound = 2 * e_t + 1e-6 * (1 + n64.abs())
    assert (e_k <= bound).all(), (e_k.max().item(), [(b, e_k[b].item(), bound[b].item()) for b in range(B) if e_k[b] > bound[b]])
    # gradient per element
    d = dl[:, :, :V]
    gk, gt = (d - g64).abs(), (g32 - g64).abs()
    gbound = 2 * gt + 1e-6 * abs(gs)
    if dtype == torch.bfloat16:
        gbound = gbound + 2 ** -8 * g64.abs()
    bad = gk > gbound
    assert not bad.any(), (int(bad.sum()), gk[bad][:5].tolist(), gbound[bad][:5].tolist(), bad.nonzero()[:5].tolist())
    print(f"CTC V={V} blank={blank} {dtype} T={T} Lmax={ys.shape[1]}: max |nll err| {e_k.max():.3e} (torch fp32 {e_t.max():.3e}),"
          f" max |grad err| {gk.max():.3e} (torch fp32 {gt.max():.3e}); max share of bound: nll {(e_k / bound).max():.3g},"
          f" grad {(gk / gbound).max():.3g}")
    return nll, n64, bound, feasible


def _logits(B, T, V, g, dtype):
    z = torch.randn(B, T, V, generator=g) * 2.0
    return z.to(dtype).float()                                   # values exact in the kernel's dtype


@pytest.mark.parametrize("Lmax", [20, 50, 100, 200, 400])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ctc_every_lattice_width_against_float64(hip, Lmax, dtype):
    """Smax = 41 / 101 / 201 / 401 / 801: the 64-, 128-, 256-, 512-thread lattices and the strided 512-thread loop."""
    from paper_accurate_fast_cheap_amd import hip_ops
    V, blank = 40, [0, 39, 17, 0, 39][[20, 50, 100, 200, 400].index(Lmax)]
    T, ys, ylens, hlens, g = _ctc_batch(Lmax, V, blank, seed=Lmax)
    z = _logits(len(ylens), T, V, g, dtype)
    _check_ctc(hip_ops, z, ys, ylens, hlens, blank, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ctc_eligibility_limit_of_3000_labels(hip, dtype):
    """max_target_len = 3000 (Smax = 6001: the strided lattice with 94 KB of fp64 LDS), rows feasible and not."""
    from paper_accurate_fast_cheap_amd import hip_ops
    V, blank = 40, 3
    T, ys, ylens, hlens, g = _ctc_batch(3000, V, blank, seed=11, T=3400)
    nll, n64, _, feasible = _check_ctc(hip_ops, _logits(len(ylens), T, V, g, dtype), ys, ylens, hlens, blank, dtype)
    assert bool(feasible[0]) and not bool(feasible[4]) and not bool(feasible[5])


@pytest.mark.parametrize("V", [5000, 20000, 38400])
@pytest.mark.parametrize("blank_at", ["zero", "last", "mid"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ctc_vocabulary_and_blank(hip, V, blank_at, dtype):
    """V = 5000, 20000 (the gradient's > 48 KB LDS attribute), 38400 (the eligibility edge); blank 0, V - 1 or mid-vocabulary."""
    from paper_accurate_fast_cheap_amd import hip_ops
    blank = {"zero": 0, "last": V - 1, "mid": V // 2 + 3}[blank_at]
    T, ys, ylens, hlens, g = _ctc_batch(20, V, blank, seed=V + len(blank_at))
    _check_ctc(hip_ops, _logits(len(ylens), T, V, g, dtype), ys, ylens, hlens, blank, dtype, grad_out=1.5, scale=1 / 8)


def _production_batch(seed=21):
    B, T, V, blank = 32, 499, 5000, 0
    g = torch.Generator().manual_seed(seed)
    Ls = torch.randint(1, 161, (B,), generator=g)
    Ls[0] = 160
    ys = torch.full((B, 160), -1, dtype=torch.long)
    hl = []
    for b in range(B):
        n = int(Ls[b])
        reps = int(torch.randint(0, max(1, n // 10), (1,), generator=g))
        ys[b, :n] = torch.tensor(_labels(n, reps, V, blank, g))
        hl.append(int(torch.randint(n + reps + 1, T + 1, (1,), generator=g)) if b else T)
    return ys, Ls, torch.tensor(hl), _logits(B, T, V, g, torch.bfloat16), blank


def test_ctc_production_shape_and_its_bound_sees_one_frame_or_one_label(hip):
    """B = 32, T = 499, V = 5000, bf16, labels up to 160 (the 512-thread lattice): within bounds, and the loss bound is tight
    enough that dropping each utterance's last frame, or changing one label, moves the float64 loss by more than 10x it."""
    from paper_accurate_fast_cheap_amd import hip_ops
    ys, ylens, hlens, z, blank = _production_batch()
    nll, n64, bound, feasible = _check_ctc(hip_ops, z, ys, ylens, hlens, blank, torch.bfloat16, grad_out=1.0, scale=1 / 32)
    assert feasible.all()
    lp = z.double().log_softmax(-1).transpose(0, 1)
    drop = F.ctc_loss(lp, ys.clamp_min(0), hlens - 1, ylens, blank=blank, reduction="none", zero_infinity=True)
    assert ((drop - n64).abs() > 10 * bound).all()
    ys2 = ys.clone()
    for b, n in enumerate(ylens.tolist()):
        j = n // 2
        ys2[b, j] = ys2[b, j] % 4999 + 1                          # another non-blank label
    changed = F.ctc_loss(lp, ys2.clamp_min(0), hlens, ylens, blank=blank, reduction="none", zero_infinity=True)
    assert float(((changed - n64).abs() > 10 * bound).double().mean()) >= 0.9


def test_ctc_bitwise_repeatable_across_calls_and_streams(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    ys, ylens, hlens, z, blank = _production_batch(seed=22)
    B, T, V = z.shape
    logits = z.bfloat16().reshape(B * T, V).cuda()
    a = _ctc_call(hip_ops, logits, B, T, V, hlens, ys, ylens, blank, 1.0, 1 / B, V + 60)
    b = _ctc_call(hip_ops, logits, B, T, V, hlens, ys, ylens, blank, 1.0, 1 / B, V + 60)
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        c = _ctc_call(hip_ops, logits, B, T, V, hlens, ys, ylens, blank, 1.0, 1 / B, V + 60)
    torch.cuda.current_stream().wait_stream(s2)
    torch.cuda.synchronize()
    for other in (b, c):
        assert torch.equal(a[0], other[0])
        assert torch.equal(a[1].view(torch.int16), other[1].view(torch.int16))


def test_ctc_head_loss_equals_the_direct_call(hip):
    """ctc_head_loss (GEMM + the same two entry points) is the direct call on gemm_bf16's logits, bit for bit."""
    from paper_accurate_fast_cheap_amd import hip_ops
    torch.manual_seed(4)
    T, C, V, Lmax = 57, 128, 5000, 20
    _, ys, ylens, hlens, _ = _ctc_batch(Lmax, V, 0, seed=5, T=T)
    B = len(ylens)
    x = (torch.randn(B, T, C, device="cuda") * 0.7).bfloat16()
    w = (torch.randn(V, C, device="cuda") * 0.2).bfloat16()
    bias = (torch.randn(V, device="cuda") * 0.1).bfloat16()
    got = hip_ops.ctc_head_loss(x, w, bias, hlens.cuda(), ys.cuda(), ylens.cuda(), 0)
    Vp = (V + 63) // 64 * 64
    logits = torch.zeros((B * T, Vp), dtype=torch.bfloat16, device="cuda")
    hip_ops.gemm_bf16(x.reshape(B * T, C), w, bias, out=logits[:, :V])
    nll, _ = _ctc_call(hip_ops, logits, B, T, V, hlens, ys, ylens, 0, 1.0, 1 / B, Vp)
    assert torch.equal(got, nll.sum() / B)


# ---- conv1 weight / bias gradient -------------------------------------------------------------------------------------------

def _conv1_data(B, T, F_, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    T1, F1 = (T - 3) // 2 + 1, (F_ - 3) // 2 + 1
    x = (4.0 + 1.5 * torch.randn(B, T, F_, generator=g, device="cuda")).bfloat16()      # log-mel-like: non-zero mean
    act = torch.randn(B, T1, F1, C, generator=g, device="cuda")
    act[torch.rand(B, T1, F1, C, generator=g, device="cuda") < 0.2] = 0.0              # exact zeros and negatives: masked out
    act = act.bfloat16()
    dact = (0.5 + torch.randn(B, T1, F1, C, generator=g, device="cuda")).bfloat16()
    dact[dact == 0] = 0.25                                        # non-zero everywhere: only the mask keeps positions out
    return x, act, dact


def _conv1_ref(x, act, dact, rows=None):
    """float64 (10, C) reference and (10, C) sum of |terms|, over output rows [0, rows) of B * T1 (all by default)."""
    B, T, F_ = x.shape
    C = act.shape[-1]
    xp = x.double().unfold(1, 3, 2).unfold(2, 3, 2)                           # (B, T1, F1, 3, 3): x[b, 2 t1 + kh, 2 f1 + kw]
    T1, F1 = xp.shape[1], xp.shape[2]
    xp = xp.reshape(B * T1, F1, 9)
    dy = (dact.double() * (act > 0)).reshape(B * T1, F1, C)
    n = B * T1 if rows is None else rows
    ref = torch.zeros(10, C, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    for r0 in range(0, n, 512):
        r1 = min(n, r0 + 512)
        p, d = xp[r0:r1].reshape(-1, 9), dy[r0:r1].reshape(-1, C)
        ref[:9] += p.t() @ d
        mag[:9] += p.abs().t() @ d.abs()
        ref[9] += d.sum(0)
        mag[9] += d.abs().sum(0)
    return ref, mag


def _conv1_bound(B, T, F_, C, mag):
    """|got - ref| <= sqrt(n_seq) 2^-22 sum|terms|, n_seq the longest chain of fp32 adds in sequence: a thread's fmas over its
    32 rows x ceil(F1 / ppi) positions, the ppi position lanes, then the reduce's ceil(nblk / 64) partials and its 64 slices."""
    T1, F1 = (T - 3) // 2 + 1, (F_ - 3) // 2 + 1
    ppi = 256 // (C // 8)
    nblk = (B * T1 + 31) // 32
    n_seq = 32 * math.ceil(F1 / ppi) + ppi + math.ceil(nblk / 64) + 64
    return math.sqrt(n_seq) * 2.0 ** -22 * mag


CONV1_CASES = [  # (B, T, F, C): ppi 256 .. 1, F1 = 1 / 39 / 40, the LDS switch at 3F > ppi C, B T1 = 1 / 31 / 32 / 33 / 2049 / 30969
    (1, 3, 3, 8), (31, 4, 80, 8), (32, 3, 81, 64), (33, 4, 80, 128), (2049, 3, 81, 512), (2, 2001, 80, 2048),
    (1, 41, 700, 512), (1, 3, 81, 2048), (2049, 3, 3, 64), (31, 2000, 80, 64),
]


@pytest.mark.parametrize("B,T,F_,C", CONV1_CASES, ids=[f"B{b}_T{t}_F{f}_C{c}" for b, t, f, c in CONV1_CASES])
def test_conv1_wgrad_against_float64(hip, B, T, F_, C):
    from paper_accurate_fast_cheap_amd import hip_ops
    x, act, dact = _conv1_data(B, T, F_, C, seed=B * 7 + T + F_ + C)
    got = hip_ops.conv3x3s2_c1_wgrad(x, act, dact)
    assert got.shape == (10, C) and got.dtype == torch.float32
    ref, mag = _conv1_ref(x, act, dact)
    bound = _conv1_bound(B, T, F_, C, mag)
    err = (got.double() - ref).abs()
    assert (err <= bound).all(), (float(err.max()), float((err / bound).max()))
    print(f"conv1 B={B} T={T} F={F_} C={C}: max |err| / sum|terms| = {float((err / mag.clamp_min(1e-300)).max()):.3e},"
          f" max |err| / bound = {float((err / bound).max()):.3f}")
    assert torch.equal(got, hip_ops.conv3x3s2_c1_wgrad(x, act, dact))               # fixed order: bitwise repeatable
    nrows = B * ((T - 3) // 2 + 1)
    if nrows % 32 and nrows > 64 * 32:
        # the bound sees the ragged last block: leaving its rows out moves the reference by more than 10x the bound
        short, _ = _conv1_ref(x, act, dact, rows=nrows // 32 * 32)
        assert float(((short - ref).abs() / bound).max()) > 10


def test_conv1_train_backward_is_the_direct_call_and_float64_conv2d(hip):
    """_Conv1Train.backward hands back the direct call's result bit for bit in the (C, 1, 3, 3) layout, and both match float64
    conv2d autograd when the ReLU mask comes from the forward kernel's own bf16 output."""
    from paper_accurate_fast_cheap_amd import hip_ops
    B, T, F_, C = 5, 203, 80, 256
    g = torch.Generator().manual_seed(9)
    x = (4.0 + 1.5 * torch.randn(B, T, F_, generator=g)).bfloat16().cuda()
    w = (torch.randn(C, 1, 3, 3, generator=g) * 0.3).cuda().requires_grad_()
    bias = (torch.randn(C, generator=g) * 0.1 - 0.2).cuda().requires_grad_()
    a = hip_ops._Conv1Train.apply(x, w, bias)
    dact = (0.5 + torch.randn(a.shape, generator=g)).bfloat16().cuda()
    a.backward(dact)
    direct = hip_ops.conv3x3s2_c1_wgrad(x, a.detach(), dact)
    assert torch.equal(w.grad, direct[:9].t().reshape(C, 1, 3, 3))
    assert torch.equal(bias.grad, direct[9])
    assert bool((a == 0).any()) and bool((a > 0).any())
    w64 = w.detach().cpu().double().requires_grad_()
    b64 = bias.detach().cpu().double().requires_grad_()
    y = F.conv2d(x.cpu().double().unsqueeze(1), w64, b64, stride=2)          # (B, C, T1, F1), float64 on the CPU
    mask = (a.detach() > 0).permute(0, 3, 1, 2).cpu()
    y.backward(dact.cpu().double().permute(0, 3, 1, 2) * mask)
    _, mag = _conv1_ref(x, a.detach(), dact)
    bound = _conv1_bound(B, T, F_, C, mag).cpu()
    ref = torch.cat([w64.grad.reshape(C, 9).t(), b64.grad[None]])
    assert ((direct.cpu().double() - ref).abs() <= bound).all()
