"""pafc_mha_band_lse and pafc_mha_band_bwd (include/pafc_attention.h) against float64 on the GPU, for fp32 and bf16, on the
cases of tests/lca_bwd_ref.CASES (H = 2, dk = 64).

The truth is float64 autograd through tests/lca_ref.band_attention (tests/test_lca_bwd_ref.py shows that the analytic
backward of tests/lca_bwd_ref.py equals it).  Bounds, asserted per case and per gradient (dq, dk, dv, dp, du, dvb) -- the rule
tests/test_mha_rows_bwd_gpu.py derives for the same arithmetic:
  fp32  the kernel's max |err| against float64 is at most 4 x the max |err| of float32 CPU autograd through the same formula
        on the same inputs: the margin covers another summation order and the device's exp.
  bf16  the yardstick is float32 CPU autograd on q, k, v, p, u, vb, dout rounded to bf16, with q + u and q + vb rounded once
        more (round_biased_q), against float64 on the unrounded inputs; the bound is 8 x, because beyond the forward's extra
        roundings (P, out) the backward rounds P, dS and its outputs.
The yardstick must be > 0 in every case -- with one exception that no kernel could meet: with w = 0 a query sees itself alone,
so P = 1 and dS = P (dP - delta) = 0, and dq, dk, dp, du and dvb are zero in exact arithmetic.  float64 and float32 CPU autograd
both return exact zeros there (the yardstick is 0), while a kernel that forms dP and delta as two separately rounded 64-term
dot products returns their rounding difference.  For those five gradients of that case the bound comes from a model of that
rounding (_self_only_bounds), written down here and not fitted to any measurement: delta is float64, so the error of
dS_ii = dP_ii - delta_i is that of the fp32 dP, a sum x_1 + ... + x_64 of exact products x_d = dout_id v_id that goes through
n_r = 20 fp32 roundings (16 accumulation steps in four chains of four, 3 adds, the final difference).  Each rounding is at most
u = 2^-24 of a partial sum; for terms of random sign a partial sum has the size of ||x||_2, and independent roundings add in
quadrature: std(dS_ii) <= u sqrt(n_r) ||x||_2.  The bound is SIX such standard deviations (the maximum of a few thousand values
lies near four), carried through the products that consume dS -- linearly for the one term of dq and dk, in quadrature over
the batch rows for dp and over all rows for du and dvb -- times 1 + 2^-7 in bf16 (q + u, dS and the outputs are rounded to
bf16).  It is a statistical bound, a few times the expected maximum; the worst-case bound (2 * 66 u sum |x_d|) would be
20 to 100 times wider.  This case therefore checks "zero up to rounding" and that nothing else leaks into these gradients;
the accuracy of dS rests on the other eight cases.  dv of that case, and everything else, keeps the yardstick rule.
lse: within 4e-6 * max(1, |lse|) of float64 on what the kernel reads, plus 2^-9 in bf16 (the forward sums the probabilities
after rounding them to bf16), that file's rule.

Every operand is a column slice of a NaN-filled wider buffer with NaN guard rows after its last row; the outputs and the
workspace are pre-filled with NaN: a finite result proves that nothing outside the operands was read and that every row of
every output (and every workspace entry that is read) was written, untouched guards that nothing else was."""
import functools

import pytest
import torch

from tests import lca_bwd_ref, lca_ref, parity_log
from tests.lca_bwd_ref import CASES, DK, H

pytestmark = pytest.mark.gpu

D, GUARD = H * DK, 3
NAMES = ("dq", "dk", "dv", "dp", "du", "dvb")


def _r16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _autograd(ins, w, t_pad, round_biased_q=None):
    leaves = [t.clone().requires_grad_(True) for t in ins[:6]]
    out = lca_ref.band_attention(*leaves, w, t_pad, round_biased_q=round_biased_q)
    return torch.autograd.grad(out, leaves, ins[6])


def _self_only_bounds(rin, bf16):
    """w = 0: the bounds on |dq|, |dk|, |dp|, |du|, |dvb| (all zero in exact arithmetic) from the inputs as the kernel reads
    them (float64 values): six standard deviations of the rounding model in the module docstring."""
    q, k, v, p, u, vb, dout = rin
    sd = 2.0 ** -24 * 20 ** 0.5 * (dout * v).pow(2).sum(-1, keepdim=True).sqrt()                # std of dS_ii, (B, T, H, 1)
    b = 6 * sd * ((1 + 2.0 ** -7) if bf16 else 1.0) / 8
    quad = lambda t, dims: t.pow(2).sum(dims).sqrt().max().item()                                # noqa: E731
    return {"dq": (b * (k.abs() + p.abs())).max().item(), "dk": (b * (q + u).abs()).max().item(),
            "dp": quad(b * (q + vb).abs(), 0), "du": quad(b * k.abs(), (0, 1)), "dvb": quad(b * p.abs(), (0, 1))}


@functools.lru_cache(maxsize=None)
def _case(n):
    """One case's float64 inputs, the float64 gradients, and per gradient the error of the two CPU yardsticks: computed once,
    shared by the fp32 and the bf16 test and left unchanged."""
    B, T, w, t_pad = CASES[n]
    t_pad = lca_bwd_ref.t_pad_of(T, w, t_pad)
    ins = lca_bwd_ref.case_inputs(B, T, 7000 + n)
    want = _autograd(ins, w, t_pad)
    f32 = _autograd([t.float() for t in ins], w, t_pad)
    b16 = _autograd([_r16(t.float()) for t in ins], w, t_pad, round_biased_q=_r16)
    err = lambda got: [(g.double() - x).abs().max().item() for g, x in zip(got, want)]      # noqa: E731
    return (B, T, w, t_pad), ins, want, err(f32), err(b16)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run_kernels(ins, B, T, w, t_pad, dtype, runs=2):
    """Forward with statistics, plain forward and `runs` backward runs -> (out, plain, lse, [(dq, dk, dv, dp, du, dvb)], whether
    every guard and every operand is untouched)."""
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    q, k, v, p, u, vb, dout = ins
    R, dev = B * T, "cuda"
    nan = lambda r, c: torch.full((r, c), float("nan"), dtype=dtype, device=dev)          # noqa: E731
    put = lambda t, n: t.reshape(n, -1).to(dtype).to(dev)                                 # noqa: E731
    qkv = nan(R + GUARD, 3 * D + 24)                                                       # [pad 8 | q | k | pad 8 | v | pad 8]
    cq, ck, cv = slice(8, 8 + D), slice(8 + D, 8 + 2 * D), slice(16 + 2 * D, 16 + 3 * D)
    qkv[:R, cq], qkv[:R, ck], qkv[:R, cv] = put(q, R), put(k, R), put(v, R)
    pbuf, dobuf = nan(T + GUARD, D + 8), nan(R + GUARD, D + 16)
    pbuf[:T, :D], dobuf[:R, 8:8 + D] = put(p, T), put(dout, R)
    ubuf, vbuf = nan(H + GUARD, DK), nan(H + GUARD, DK)
    ubuf[:H], vbuf[:H] = put(u, H), put(vb, H)
    ops = (qkv[:R, cq], qkv[:R, ck], qkv[:R, cv], pbuf[:T, :D], ubuf[:H], vbuf[:H])
    before = [t.clone() for t in (qkv, pbuf, dobuf, ubuf, vbuf)]
    out, lse = hip_ops.mha_band_lse(*ops, B, H, w, t_pad)
    plain = hip_ops.mha_band(*ops, B, H, w, t_pad)
    nbytes = _lib.lib().pafc_mha_band_bwd_workspace_bytes(B, T, H)
    results, ok = [], True
    for _ in range(runs):
        dqkv, dpbuf = nan(R + GUARD, 3 * D + 16), nan(T + GUARD, D + 8)                    # [pad 8 | dq | dk | dv | pad 8]
        ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)                     # (all-ones words are NaN)
        got = hip_ops.mha_band_bwd(*ops, out, dobuf[:R, 8:8 + D], lse, B, H, w, t_pad, dq=dqkv[:R, 8:8 + D],
                                   dk=dqkv[:R, 8 + D:8 + 2 * D], dv=dqkv[:R, 8 + 2 * D:8 + 3 * D], dp=dpbuf[:T, :D], workspace=ws)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == dqkv[:R, 8:8 + D].data_ptr() and got[3].data_ptr() == dpbuf.data_ptr()
        ok = ok and bool(torch.isnan(dqkv[R:]).all() and torch.isnan(dqkv[:, :8]).all() and torch.isnan(dqkv[:, 8 + 3 * D:]).all()
                         and torch.isnan(dpbuf[T:]).all() and torch.isnan(dpbuf[:, D:]).all())
        results.append([t.clone() for t in got])
    ok = ok and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, (qkv, pbuf, dobuf, ubuf, vbuf)))
    return out, plain, lse.double().cpu(), results, ok


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mha_band_bwd_against_float64_autograd(hip, dtype):
    tag = "fp32" if dtype == torch.float32 else "bf16"
    bound = 4 if dtype == torch.float32 else 8
    failures = []
    for n in range(len(CASES)):
        (B, T, w, t_pad), ins, want, e32, e16 = _case(n)
        name = f"B{B}_T{T}_w{w}_tpad{t_pad}"
        yard = e32 if dtype == torch.float32 else e16
        out, plain, lse, runs, untouched = _run_kernels(ins, B, T, w, t_pad, dtype)
        assert torch.equal(_bits(out), _bits(plain)), name                                # bit for bit pafc_mha_band's out
        assert untouched, name                                                             # guards and operands as they were
        for a, b in zip(runs[0], runs[1]):
            assert torch.equal(_bits(a), _bits(b)), name                                  # two runs: the same bits
        got = [t.double().cpu() for t in runs[0]]
        assert all(torch.isfinite(t).all() for t in got) and torch.isfinite(lse).all(), name
        assert runs[0][4].dtype == torch.float32 and runs[0][5].dtype == torch.float32    # du, dvb: float32 in both modes
        # lse against float64 of what the kernel reads
        rd = (lambda t: t.float().double()) if dtype == torch.float32 else (lambda t: _r16(t.float()).double())
        lse64 = lca_bwd_ref.band_attention_bwd(*[rd(t) for t in ins], w, t_pad,
                                               round_biased_q=None if dtype == torch.float32 else _r16)[-1]
        lerr = (lse.view(B, T, H) - lse64).abs().max().item()
        tol = 4e-6 * max(1.0, lse64.abs().max().item()) + (2.0 ** -9 if dtype == torch.bfloat16 else 0.0)
        print(f"mha_band_lse {name} {tag}: max|lse err| {lerr:.3e} (tolerance {tol:.3e})")
        if not lerr <= tol:
            failures.append((name, "lse", lerr, tol))
        shapes = [(B, T, H, DK)] * 3 + [(T, H, DK), (H, DK), (H, DK)]
        zero = _self_only_bounds([rd(t) for t in ins], dtype == torch.bfloat16) if w == 0 else {}
        for gname, g, x, ec, shape in zip(NAMES, got, want, yard, shapes):
            ek = (g.view(shape) - x).abs().max().item()
            if gname in zero:                          # zero in exact arithmetic: the format's bound, not the (zero) yardstick
                assert x.abs().max().item() == 0 and ec == 0, (name, gname)
                print(f"mha_band_bwd {name} {tag} {gname}: max|err| kernel {ek:.3e}, derived bound {zero[gname]:.3e}")
                parity_log.record(f"mha_band_bwd_{tag}_{name}_{gname}", max_abs_err=ek, derived_bound=zero[gname])
                if not ek <= zero[gname]:
                    failures.append((name, gname, ek, zero[gname]))
                continue
            print(f"mha_band_bwd {name} {tag} {gname}: max|err| kernel {ek:.3e}, cpu yardstick {ec:.3e}, "
                  f"ratio {ek / ec if ec else float('inf'):.2f}")
            parity_log.record(f"mha_band_bwd_{tag}_{name}_{gname}", max_abs_err=ek, cpu_yardstick_err=ec)
            if not (ec > 0 and ek <= bound * ec):
                failures.append((name, gname, ek, ec))
    assert not failures, failures


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batch_rows_are_independent(hip, dtype):
    """dq, dk, dv of row b of the B = 3 case equal that row run alone with B = 1, bit for bit; dp of the batch is the sum of
    the rows' (its bound against the float64 sum is asserted with the other gradients above), du / dvb likewise."""
    n = next(i for i, c in enumerate(CASES) if c[0] == 3)
    (B, T, w, t_pad), ins, want, _, _ = _case(n)
    _, _, _, runs, _ = _run_kernels(ins, B, T, w, t_pad, dtype, runs=1)
    dq, dk, dv, dp = (t.view(B, T, D) if i < 3 else t for i, t in enumerate(runs[0][:4]))
    dp_sum = torch.zeros(T, D, dtype=torch.float64)
    for b in range(B):
        alone = [t[b:b + 1] if t.dim() == 4 else t for t in ins]
        _, _, _, one, ok = _run_kernels(alone, 1, T, w, t_pad, dtype, runs=1)
        assert ok
        for name, batch, single in zip(("dq", "dk", "dv"), (dq, dk, dv), one[0][:3]):
            assert torch.equal(_bits(batch[b].contiguous()), _bits(single.contiguous())), (name, b)
        dp_sum += one[0][3].double().cpu()
    # the batch's dp against the sum of the rows' own: one rounding of the sum apart (bf16: each row's dp was rounded too)
    eps = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -8
    assert (dp.double().cpu() - dp_sum).abs().max().item() <= 4 * eps * dp_sum.abs().max().item()


def test_mha_band_train_autograd_function(hip):
    """hip_ops.mha_band_train hands dq | dk | dv to the thirds of one stacked projection and returns gradients for p and both
    biases; separate q, k, v get gradients of their own shapes."""
    from paper_accurate_fast_cheap_amd import hip_ops
    n = next(i for i, c in enumerate(CASES) if (c[0], c[1]) == (2, 67))
    (B, T, w, t_pad), ins, want, e32, _ = _case(n)
    q, k, v, p, u, vb, dout = ins
    R = B * T
    dev = lambda t, r: t.reshape(r, -1).float().cuda()                                    # noqa: E731
    for stacked in (True, False):
        pp, uu, vv = dev(p, T).requires_grad_(True), dev(u, H).requires_grad_(True), dev(vb, H).requires_grad_(True)
        if stacked:
            qkv = torch.cat([dev(q, R), dev(k, R), dev(v, R)], dim=1).requires_grad_(True)
            leaves = (qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:])
        else:
            qq, kv = dev(q, R).requires_grad_(True), torch.cat([dev(k, R), dev(v, R)], dim=1).requires_grad_(True)
            leaves = (qq, kv[:, :D], kv[:, D:])
        out = hip_ops.mha_band_train(*leaves, pp, uu, vv, B, H, w)
        out.backward(dev(dout, R))
        torch.cuda.synchronize()
        got_qkv = qkv.grad if stacked else torch.cat([qq.grad, kv.grad], dim=1)
        want_qkv = torch.cat([t.reshape(R, D) for t in want[:3]], dim=1)
        assert (got_qkv.double().cpu() - want_qkv).abs().max().item() <= 4 * max(e32[:3])
        for g, x, ec in zip((pp.grad, uu.grad, vv.grad), want[3:], e32[3:]):
            assert g.dtype == torch.float32 and (g.double().cpu() - x.reshape(g.shape)).abs().max().item() <= 4 * ec


def test_mha_band_bwd_refuses_bad_arguments(hip):
    """dk != 64, t_pad < T, a misaligned pitch and a short workspace (and the rest of the list) each give an error code with no
    launch; the wrapper names what is unmet."""
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    from tests.test_lca_bwd_ref import check_band_bad_arguments
    check_band_bad_arguments(hip)
    x = torch.zeros(10, 128, device="cuda")
    p, u = torch.zeros(5, 128, device="cuda"), torch.zeros(2, 64, device="cuda")
    lse = torch.zeros(10, 2, device="cuda")
    ok = lambda **kw: hip_ops.mha_band_bwd(**dict(dict(q=x, k=x, v=x, p=p, pos_bias_u=u, pos_bias_v=u, out=x, dout=x, lse=lse,  # noqa: E731
                                                       batch=2, heads=2, w=2), **kw))
    assert tuple(ok()[0].shape) == (10, 128)
    for kw, word in ((dict(t_pad=4), "t_pad"), (dict(lse=lse[:, :1]), "lse"), (dict(dout=x[:5]), "dout"),
                     (dict(dq=torch.zeros(10, 132, device="cuda")[:, 1:129]), "dq"),
                     (dict(dp=torch.zeros(4, 128, device="cuda")), "dp"), (dict(w=-1), "negative")):
        with pytest.raises(_lib.PafcError, match=word):
            ok(**kw)
    with pytest.raises(_lib.PafcError, match="workspace"):
        ok(workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
