"""The two kernels of include/pafc_attention.h against float64 on the GPU: pafc_mha_rows (attention over packed row groups)
and pafc_logp_gather_rows (log p(target) per row straight from the logits).

Bounds, asserted per case (each case's own inputs).  fp32: the kernel's max |err| against float64 is at most 4 x the max |err|
of the same formula run in float32 on the CPU against float64 on the same inputs; the margin covers a different summation
order and the device's exp.  (Where a case's CPU error rounds to exactly zero, a single row can, the case joins the next
non-zero yardstick of its test instead of demanding an exact kernel.)  bf16: the kernel reads q, k, v rounded to bf16, so the
yardstick is the float32 CPU run on q, k, v rounded to bf16, against float64 on the unrounded inputs -- the error the bf16
operands alone cause; the kernel adds one bf16 rounding of the probabilities and one of the output, each of the size of one
operand's rounding, which the factor 4 covers."""
import math

import pytest
import torch

from tests import parity_log

pytestmark = pytest.mark.gpu

H, DK = 2, 64
D = H * DK


def _attention(q, k, v, q_off, kv_off, kv_len, causal):
    """softmax(Q K^T / sqrt(dk)) V per group and head in the dtype of q; rows of a group without keys stay zero."""
    out = torch.zeros(q.shape[0], D, dtype=q.dtype)
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
            out[a:e, cs] = torch.softmax(s, dim=-1) @ v[kv_off[g]:kv_off[g] + n, cs]
    return out


def _cases():
    """[(name, causal, q (rows, D), k, v (kv rows, D), q_off, kv_off, kv_len)] in float64."""
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    # cross-attention: every kv_len around the 16- and 32-key tiles, query counts around the 16-row tile, a group without
    # queries, and one memory (130 rows at offset 0) shared by three groups
    kv_lens = [0, 1, 15, 16, 17, 31, 33, 64, 65, 130, 130, 130, 7]
    nq = [3, 1, 16, 17, 2, 5, 33, 1, 4, 18, 2, 47, 0]
    q_off, kv_off, at = [0], [], 0
    for n, m in zip(kv_lens, nq):
        q_off.append(q_off[-1] + m)
        if n == 130:
            kv_off.append(0)
        else:
            kv_off.append(130 + at)
            at += n
    cross = ("cross", False, rnd(q_off[-1], D), rnd(130 + at, D), rnd(130 + at, D), q_off, kv_off, kv_lens)
    # self-attention over packed rows: kv_off = q_off, kv_len = the group's rows
    rows = [1, 16, 17, 47, 0, 5]
    q_off = [0]
    for m in rows:
        q_off.append(q_off[-1] + m)
    R = q_off[-1]
    causal = ("causal", True, rnd(R, D), rnd(R, D), rnd(R, D), q_off, q_off[:-1], rows)
    return [cross, causal]


def _run_kernel(q, k, v, q_off, kv_off, kv_len, causal, dtype):
    """q, k, v as column slices of wider buffers (ldq, ldkv > H * dk; k and v in one stacked buffer)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    dev = "cuda"
    qbuf = torch.full((q.shape[0], D + 24), float("nan"), dtype=dtype, device=dev)
    qbuf[:, 8:8 + D] = q.to(dtype)
    kvbuf = torch.full((k.shape[0], 2 * D + 16), float("nan"), dtype=dtype, device=dev)
    kvbuf[:, :D] = k.to(dtype)
    kvbuf[:, D + 8:2 * D + 8] = v.to(dtype)
    out = torch.full((q.shape[0], D), float("nan"), dtype=dtype, device=dev)
    i32 = lambda t: torch.tensor(t, dtype=torch.int32, device=dev)              # noqa: E731
    got = hip_ops.mha_rows(qbuf[:, 8:8 + D], kvbuf[:, :D], kvbuf[:, D + 8:2 * D + 8], i32(q_off), i32(kv_off), i32(kv_len), H,
                           causal, out=out)
    torch.cuda.synchronize()
    return got.double().cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mha_rows_against_float64(hip, dtype):
    for name, causal, q, k, v, q_off, kv_off, kv_len in _cases():
        want = _attention(q, k, v, q_off, kv_off, kv_len, causal)
        if dtype == torch.float32:
            cpu = _attention(q.float(), k.float(), v.float(), q_off, kv_off, kv_len, causal)
        else:
            r = lambda t: t.to(torch.bfloat16).float()                            # noqa: E731
            cpu = _attention(r(q), r(k), r(v), q_off, kv_off, kv_len, causal)
        got = _run_kernel(q, k, v, q_off, kv_off, kv_len, causal, dtype)
        assert torch.isfinite(got).all(), name                                    # every row of every group was written
        for g in range(len(kv_len)):
            if kv_len[g] == 0:
                assert (got[q_off[g]:q_off[g + 1]] == 0).all(), name              # no keys: exact zeros
        ek, ec = (got - want).abs().max().item(), (cpu.double() - want).abs().max().item()
        print(f"mha_rows {name} {dtype}: max|err| kernel {ek:.3e}, cpu yardstick {ec:.3e}")
        parity_log.record(f"mha_rows_{'fp32' if dtype == torch.float32 else 'bf16'}_{name}", max_abs_err=ek, cpu_yardstick_err=ec)
        assert ec > 0 and ek <= 4 * ec, (name, ek, ec)


def test_mha_rows_refuses_other_head_sizes_and_bad_arguments(hip):
    from paper_accurate_fast_cheap_amd import _lib
    x = torch.zeros(4, 64, device="cuda")
    off = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    one = torch.tensor([4], dtype=torch.int32, device="cuda")
    p, st = _lib.ptr, _lib.stream_of(x)

    def call(dtype=0, G=1, Hh=1, dk=64, ld=64, q=x):
        return hip.pafc_mha_rows(dtype, G, Hh, dk, p(q), ld, p(x), p(x), ld, p(off), p(off), p(one), 0, p(x), ld, st)

    assert call(Hh=2, dk=32) == -7                     # PAFC_ERR_UNSUPPORTED
    assert call(dtype=5) == -6
    assert call(G=0) == -2 and call(ld=60) == -2 and call(ld=66) == -2
    assert call(q=None) == -1
    assert call() == 0
    torch.cuda.synchronize()


def test_logp_gather_rows_against_float64(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    g = torch.Generator().manual_seed(9)
    pending = []                                       # cases whose CPU yardstick rounded to zero: judged with the next one
    for V in (53, 5000):
        for rows in (1, 67):
            x = torch.randn(rows, V, generator=g, dtype=torch.float64) * 3
            x[rows // 2, V // 3] = 80.0                                           # a row with one value of 80
            t = torch.randint(0, V, (rows,), generator=g)
            t[0] = 0 if rows == 1 and V == 53 else V - 1                          # the first and the last column
            if rows > 1:
                t[1], t[2], t[rows // 2] = 0, V - 1, V // 3
            t32 = t.to(torch.int32).cuda()
            buf = torch.full((rows, V + 3), float("nan"), device="cuda")          # a row pitch wider than V
            buf[:, :V] = x.float()
            # fp32 logits against float64 of the unrounded values, and bf16 logits (the same values rounded; fp32 arithmetic
            # inside) against float64 of the rounded ones; the yardstick is the float32 CPU log_softmax of what the kernel reads
            xb = x.to(torch.bfloat16)
            for tag, x64, xin, dev_in in (("fp32", x, x.float(), buf[:, :V]), ("bf16", xb.double(), xb, xb.cuda())):
                want = torch.log_softmax(x64, -1).gather(1, t[:, None])[:, 0]
                cpu = torch.log_softmax(xin.float(), -1).gather(1, t[:, None])[:, 0].double()
                got = hip_ops.logp_gather_rows(dev_in, t32).double().cpu()
                assert torch.isfinite(got).all()
                ek, ec = (got - want).abs().max().item(), (cpu - want).abs().max().item()
                print(f"logp_gather_rows V={V} rows={rows} {tag}: max|err| kernel {ek:.3e}, cpu yardstick {ec:.3e}")
                parity_log.record(f"logp_gather_rows_V{V}_rows{rows}_{tag}", max_abs_err=ek, cpu_yardstick_err=ec)
                pending.append(ek)
                if ec > 0:
                    assert max(pending) <= 4 * ec, (V, rows, tag, pending, ec)
                    pending = []
    assert not pending
    nan_row = torch.randn(3, 300, device="cuda")
    nan_row[1, 299] = float("nan")                                                # a NaN logit: NaN for its row alone
    out = hip_ops.logp_gather_rows(nan_row, torch.tensor([0, 0, 5], dtype=torch.int32, device="cuda"))
    assert torch.isnan(out[1]) and torch.isfinite(out[0]) and torch.isfinite(out[2])
    inf_row = torch.randn(2, 53, device="cuda")
    inf_row[0, 7] = -float("inf")                                                 # -inf is an ordinary logit
    out = hip_ops.logp_gather_rows(inf_row, torch.tensor([7, 1], dtype=torch.int32, device="cuda")).cpu()
    assert out[0] == -float("inf") and torch.isfinite(out[1])
    bad = hip_ops.logp_gather_rows(torch.zeros(2, 5, device="cuda"), torch.tensor([5, -1], dtype=torch.int32, device="cuda"))
    assert torch.isnan(bad).all()                                                 # a target outside [0, V): NaN, nothing read
    assert hip.pafc_logp_gather_rows(0, 0, 5, 16, 5, 16, 16, None) == -2
    assert hip.pafc_logp_gather_rows(0, 2, 5, 16, 4, 16, 16, None) == -2
