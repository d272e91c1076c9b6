"""pafc_mha_rows_lse and pafc_mha_rows_bwd (include/pafc_attention.h) against float64 autograd on the GPU.

Gradients are compared with float64 autograd through this file's own attention formula, for upstream gradients dout drawn
like the operands.  Bounds, asserted per case and per gradient (dq, dk, dv):
  fp32  the kernel's max |err| against float64 is at most 4 x the max |err| of float32 CPU autograd through the same formula
        on the same inputs -- the forward test's rule (tests/test_mha_rows_gpu.py): the margin covers another summation order
        and the device's exp.
  bf16  the yardstick is float32 CPU autograd on q, k, v, dout rounded to bf16, against float64 on the unrounded inputs; the
        bound is 8 x, because beyond the forward's two extra roundings (P, out) the backward rounds P, dS and its three
        outputs.
The key ranges are disjoint (the backward's precondition); the operands are column slices of NaN-filled wider buffers and
dq / dk / dv are pre-filled with NaN, so a read past a slice or a row left unwritten shows."""
import math

import pytest
import torch

from tests import parity_log

pytestmark = pytest.mark.gpu

H, DK = 2, 64
D = H * DK


def _attention(q, k, v, q_off, kv_off, kv_len, causal, want_lse=False):
    """softmax(Q K^T / sqrt(dk)) V per group and head in the dtype of q (differentiable); rows of a group without keys stay zero.
    want_lse: also the (rows, H) log of the softmax denominators (-inf without keys)."""
    out = torch.zeros(q.shape[0], D, dtype=q.dtype)
    lse = torch.full((q.shape[0], H), -float("inf"), dtype=q.dtype)
    parts = []
    for g in range(len(kv_len)):
        a, e, n = q_off[g], q_off[g + 1], kv_len[g]
        if e == a or n == 0:
            continue
        for h in range(H):
            cs = slice(h * DK, (h + 1) * DK)
            s = q[a:e, cs] @ k[kv_off[g]:kv_off[g] + n, cs].T / math.sqrt(DK)
            if causal:
                hidden = torch.arange(n)[None, :] > torch.arange(e - a)[:, None]
                s = s.masked_fill(hidden, -float("inf"))
            parts.append((a, e, cs, torch.softmax(s, dim=-1) @ v[kv_off[g]:kv_off[g] + n, cs]))
            lse[a:e, h] = torch.logsumexp(s.detach(), dim=-1)
    for a, e, cs, o in parts:
        out = out.index_put((torch.arange(a, e)[:, None], torch.arange(cs.start, cs.stop)[None, :]), o)
    return (out, lse) if want_lse else out


def _grads(q, k, v, dout, q_off, kv_off, kv_len, causal):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = _attention(q, k, v, q_off, kv_off, kv_len, causal)
    return torch.autograd.grad(out, (q, k, v), dout)


def _cases():
    """[(name, causal, q, dout (rows, D), k, v (kv rows, D), q_off, kv_off, kv_len)] in float64; kv rows has 5 unowned rows at the
    end, and the rows of groups without query rows are unowned too."""
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    kv_lens = [0, 1, 15, 16, 17, 31, 33, 64, 65, 130, 7]
    nq = [3, 1, 16, 17, 2, 5, 33, 1, 4, 18, 0]
    q_off, kv_off, at = [0], [], 3                                            # (3 unowned rows in front)
    for n, m in zip(kv_lens, nq):
        q_off.append(q_off[-1] + m)
        kv_off.append(at)
        at += n
    cross = ("cross", False, rnd(q_off[-1], D), rnd(q_off[-1], D), rnd(at + 5, D), rnd(at + 5, D), q_off, kv_off, kv_lens)
    # 70: a wave of the forward (four per block) takes a second turn of its tile loop; 130: one of the backward (eight) does
    rows = [1, 16, 17, 47, 0, 5, 70, 130]
    q_off = [0]
    for m in rows:
        q_off.append(q_off[-1] + m)
    R = q_off[-1]
    causal = ("causal", True, rnd(R, D), rnd(R, D), rnd(R, D), rnd(R, D), q_off, q_off[:-1], rows)
    return [cross, causal]


def _owned(q_off, kv_off, kv_len, n_kv):
    own = torch.zeros(n_kv, dtype=torch.bool)
    for g in range(len(kv_len)):
        if q_off[g + 1] > q_off[g]:
            own[kv_off[g]:kv_off[g] + kv_len[g]] = True
    return own


def _run_kernels(q, k, v, dout, q_off, kv_off, kv_len, causal, dtype):
    """Forward with statistics, plain forward, and backward twice; every operand a column slice of a NaN-filled wider buffer."""
    from paper_accurate_fast_cheap_amd import hip_ops
    dev = "cuda"
    nan = lambda r, c: torch.full((r, c), float("nan"), dtype=dtype, device=dev)          # noqa: E731
    qbuf = nan(q.shape[0], D + 24)
    qbuf[:, 8:8 + D] = q.to(dtype)
    kvbuf = nan(k.shape[0], 2 * D + 16)
    kvbuf[:, :D] = k.to(dtype)
    kvbuf[:, D + 8:2 * D + 8] = v.to(dtype)
    dobuf = nan(q.shape[0], D + 8)
    dobuf[:, :D] = dout.to(dtype)
    qs, ks, vs = qbuf[:, 8:8 + D], kvbuf[:, :D], kvbuf[:, D + 8:2 * D + 8]
    i32 = lambda t: torch.tensor(t, dtype=torch.int32, device=dev)              # noqa: E731
    tabs = (i32(q_off), i32(kv_off), i32(kv_len))
    out, lse = hip_ops.mha_rows_lse(qs, ks, vs, *tabs, H, causal)
    plain = hip_ops.mha_rows(qs, ks, vs, *tabs, H, causal)
    runs = []
    for _ in range(2):
        dqbuf, dkvbuf = nan(q.shape[0], D + 16), nan(k.shape[0], 2 * D + 8)
        got = hip_ops.mha_rows_bwd(qs, ks, vs, out, dobuf[:, :D], lse, *tabs, H, causal, dq=dqbuf[:, 8:8 + D],
                                   dk=dkvbuf[:, :D], dv=dkvbuf[:, D + 8:])
        torch.cuda.synchronize()
        runs.append([t.clone() for t in got])
    return out, plain, lse.double().cpu(), runs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mha_rows_bwd_against_float64_autograd(hip, dtype):
    tag = "fp32" if dtype == torch.float32 else "bf16"
    bound = 4 if dtype == torch.float32 else 8
    for name, causal, q, dout, k, v, q_off, kv_off, kv_len in _cases():
        want = _grads(q, k, v, dout, q_off, kv_off, kv_len, causal)
        r = (lambda t: t.float()) if dtype == torch.float32 else (lambda t: t.to(torch.bfloat16).float())
        cpu = _grads(r(q), r(k), r(v), r(dout), q_off, kv_off, kv_len, causal)
        out, plain, lse, runs = _run_kernels(q, k, v, dout, q_off, kv_off, kv_len, causal, dtype)
        in_group = torch.zeros(q.shape[0], dtype=torch.bool)
        in_group[q_off[0]:q_off[-1]] = True
        assert torch.equal(out[in_group.cuda()], plain[in_group.cuda()]), name          # bit for bit pafc_mha_rows' out
        # lse against float64 of what the kernel reads (a few float32 roundings of a number of size log(keys) + |s|)
        _, lse64 = _attention(r(q).double(), r(k).double(), r(v).double(), q_off, kv_off, kv_len, causal, want_lse=True)
        has_keys = torch.isfinite(lse64[:, 0])
        assert torch.equal(torch.isfinite(lse[:, 0]), has_keys), name
        assert (lse[~has_keys] == -float("inf")).all(), name
        lerr = (lse[has_keys] - lse64[has_keys]).abs().max().item()
        print(f"mha_rows_lse {name} {tag}: max|lse err| {lerr:.3e}")
        # bf16: the forward sums the probabilities AFTER rounding them to bf16 (so that the weights PV applies sum to one); each
        # is off by at most 2^-9 of itself, hence so is their sum, and its log by 2^-9
        tol = 4e-6 * max(1.0, lse64[has_keys].abs().max().item()) + (2.0 ** -9 if dtype == torch.bfloat16 else 0.0)
        assert lerr <= tol, (name, lerr, tol)
        for a, b in zip(runs[0], runs[1]):
            assert torch.equal(a, b), name                                                # two runs: the same bits
        dq, dk, dv = (t.double().cpu() for t in runs[0])
        own = _owned(q_off, kv_off, kv_len, k.shape[0])
        assert torch.isfinite(dq).all() and torch.isfinite(dk).all() and torch.isfinite(dv).all(), name
        assert (dk[~own] == 0).all() and (dv[~own] == 0).all(), name                     # rows outside every range: zero
        assert name != "cross" or (~own).sum() >= 15              # 3 in front, 5 behind, the 7 of the group without queries
        for g in range(len(kv_len)):
            if kv_len[g] == 0:
                assert (dq[q_off[g]:q_off[g + 1]] == 0).all(), name                       # no keys: out does not depend on q
        for gname, got, w, c in zip(("dq", "dk", "dv"), (dq, dk, dv), want, cpu):
            ek, ec = (got - w).abs().max().item(), (c.double() - w).abs().max().item()
            print(f"mha_rows_bwd {name} {tag} {gname}: max|err| kernel {ek:.3e}, cpu yardstick {ec:.3e}, ratio {ek / ec:.2f}")
            parity_log.record(f"mha_rows_bwd_{tag}_{name}_{gname}", max_abs_err=ek, cpu_yardstick_err=ec)
            assert ec > 0 and ek <= bound * ec, (name, gname, ek, ec)


def test_mha_rows_train_autograd_function(hip):
    """hip_ops.mha_rows_train hands the three gradients to slices of one stacked projection."""
    from paper_accurate_fast_cheap_amd import hip_ops
    name, causal, q, dout, k, v, q_off, kv_off, kv_len = _cases()[1]
    qkv = torch.cat([q, k, v], dim=1).float().cuda().requires_grad_(True)
    i32 = lambda t: torch.tensor(t, dtype=torch.int32, device="cuda")              # noqa: E731
    out = hip_ops.mha_rows_train(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], i32(q_off), i32(kv_off), i32(kv_len), H, True)
    out.backward(dout.float().cuda())
    want = torch.cat(_grads(q, k, v, dout, q_off, kv_off, kv_len, causal), dim=1)
    assert (qkv.grad.double().cpu() - want).abs().max().item() < 1e-4


def test_mha_rows_bwd_refuses_bad_arguments(hip):
    from tests.test_att_loss import check_bad_arguments
    check_bad_arguments(hip)
