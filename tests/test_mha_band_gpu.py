"""pafc_mha_band (include/pafc_attention.h) against float64 on the GPU: limited-context attention with the positional term
and the reference's unmasked padding keys, restated in tests/lca_ref.py.

Bounds, asserted per case on that case's own inputs -- the project's own, from tests/test_mha_rows_gpu.py.  fp32: the kernel's
max |err| against float64 is at most 4 x the max |err| of the same formula run in float32 on the CPU; the margin covers a
different summation order and the device's exp.  bf16: the kernel reads q, k, v, p, u, v rounded to bf16 and rounds q + u and
q + v once more, so the yardstick is the float32 CPU run on exactly those values against float64 on the unrounded inputs;
the kernel adds one bf16 rounding of the probabilities and one of the output, which the factor 4 covers.  Where a case's
yardstick rounds to zero, the case joins the next non-zero one.

Every operand is a slice of a NaN-filled buffer with NaN guard rows before and after it, q / k / v column slices of ONE wider
buffer: a finite output proves that nothing outside the operands was read, untouched guards that nothing outside the output
was written."""
import functools

import pytest
import torch

from tests import lca_ref, parity_log

pytestmark = pytest.mark.gpu

DK, GUARD = 64, 2
CONTEXTS = (2, 3, 16, 17, 40)


def _lengths(w):
    return sorted({1, 2 * w - 1, 2 * w, 2 * w + 1, 63, 64, 65, 4 * w + 3, 200})


def _special_cases():
    """(name, B, T, H, w, t_pad)"""
    return [("t_pad_T_plus_1", 3, 10, 2, 3, 11),            # not a multiple of 2 w: one padding key, seen by the last 3 queries
            ("t_pad_T_plus_1_tile_edge", 1, 64, 2, 16, 65),
            ("full_attention_w_ge_t_pad", 3, 70, 2, 300, 70),    # the band covers everything
            ("full_attention_padded", 1, 50, 2, 64, 64),         # ... and every query sees all 14 padding keys
            ("real_context", 1, 700, 8, 256, 1024)]


@functools.lru_cache(maxsize=None)
def _case(B, T, H, w, t_pad):
    """Inputs in float64 and the three CPU results of one case, computed once and shared by the fp32 and the bf16 test:
    (inputs, float64 truth, float32 yardstick error, bf16-operand yardstick error)."""
    g = torch.Generator().manual_seed(1000003 * w + 1009 * T + 17 * B + H)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    q, k, v, p = rnd(B, T, H, DK), rnd(B, T, H, DK), rnd(B, T, H, DK), rnd(T, H, DK)
    u, vb = rnd(H, DK) * 0.5, rnd(H, DK) * 0.5
    ops = (q, k, v, p, u, vb)
    want = lca_ref.band_attention(*ops, w, t_pad)
    f32 = lca_ref.band_attention(*[t.float() for t in ops], w, t_pad).double()
    r = lambda t: t.to(torch.bfloat16).float()                                # noqa: E731
    b16 = lca_ref.band_attention(*[r(t) for t in ops], w, t_pad, round_biased_q=r).double()
    return ops, want, (f32 - want).abs().max().item(), (b16 - want).abs().max().item()


def _run_kernel(ops, B, T, H, w, t_pad, dtype):
    """-> (out (B, T, H, dk) float64 on the CPU, whether every guard is untouched)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    q, k, v, p, u, vb = ops
    D, R, nan, dev = H * DK, B * T, float("nan"), "cuda"
    qkv = torch.full((GUARD + R + GUARD, 3 * D + 24), nan, dtype=dtype, device=dev)       # [pad 8 | q | k | pad 8 | v | pad 8]
    rows = slice(GUARD, GUARD + R)
    cq, ck, cv = slice(8, 8 + D), slice(8 + D, 8 + 2 * D), slice(16 + 2 * D, 16 + 3 * D)
    qkv[rows, cq], qkv[rows, ck], qkv[rows, cv] = (t.reshape(R, D).to(dtype).to(dev) for t in (q, k, v))
    pbuf = torch.full((GUARD + T + GUARD, D + 8), nan, dtype=dtype, device=dev)
    pbuf[GUARD:GUARD + T, :D] = p.reshape(T, D).to(dtype).to(dev)
    ubuf = torch.full((GUARD + H + GUARD, DK), nan, dtype=dtype, device=dev)
    vbuf = ubuf.clone()
    ubuf[GUARD:GUARD + H], vbuf[GUARD:GUARD + H] = u.to(dtype).to(dev), vb.to(dtype).to(dev)
    obuf = torch.full((GUARD + R + GUARD, D + 8), nan, dtype=dtype, device=dev)
    before = [t.clone() for t in (qkv, pbuf, ubuf, vbuf)]
    out = hip_ops.mha_band(qkv[rows, cq], qkv[rows, ck], qkv[rows, cv], pbuf[GUARD:GUARD + T, :D], ubuf[GUARD:GUARD + H],
                           vbuf[GUARD:GUARD + H], B, H, w, t_pad, out=obuf[rows, :D])
    torch.cuda.synchronize()
    assert out.data_ptr() == obuf[rows, :D].data_ptr()
    same = lambda a, b: torch.equal(a.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),    # noqa: E731
                                    b.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))     # (NaN == NaN by bits)
    guards_ok = all(same(a, b) for a, b in zip(before, (qkv, pbuf, ubuf, vbuf)))
    guards_ok = guards_ok and bool(torch.isnan(obuf[:GUARD]).all() and torch.isnan(obuf[GUARD + R:]).all()
                                   and torch.isnan(obuf[:, D:]).all())
    return obuf[rows, :D].double().cpu().view(B, T, H, DK), guards_ok


def _check(cases, dtype):
    tag = "fp32" if dtype == torch.float32 else "bf16"
    pending = []                                       # cases whose CPU yardstick rounded to zero: judged with the next one
    for name, B, T, H, w, t_pad in cases:
        ops, want, e32, e16 = _case(B, T, H, w, t_pad)
        ec = e32 if dtype == torch.float32 else e16
        got, guards_ok = _run_kernel(ops, B, T, H, w, t_pad, dtype)
        assert torch.isfinite(got).all(), name         # every row written, nothing outside the operands read
        assert guards_ok, name                         # nothing outside the output written
        ek = (got - want).abs().max().item()
        print(f"mha_band {name} {tag}: max|err| kernel {ek:.3e}, cpu yardstick {ec:.3e}, ratio {ek / ec if ec else float('inf'):.2f}")
        parity_log.record(f"mha_band_{tag}_{name}", max_abs_err=ek, cpu_yardstick_err=ec)
        pending.append(ek)
        if ec > 0:
            assert max(pending) <= 4 * ec, (name, pending, ec)
            pending = []
    assert not pending


@pytest.mark.parametrize("w", CONTEXTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mha_band_against_float64(hip, dtype, w):
    _check([(f"w{w}_T{T}_B{B}", B, T, 2, w, lca_ref.reference_t_pad(T, w)) for T in _lengths(w) for B in (1, 3)], dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mha_band_other_paddings_full_attention_and_the_real_context(hip, dtype):
    _check(_special_cases(), dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_runs_give_the_same_bits(hip, dtype):
    ops, _, _, _ = _case(3, 200, 2, 17, lca_ref.reference_t_pad(200, 17))
    a, _ = _run_kernel(ops, 3, 200, 2, 17, 204, dtype)
    b, _ = _run_kernel(ops, 3, 200, 2, 17, 204, dtype)
    assert torch.equal(a, b)


def test_wrapper_names_what_is_unmet(hip):
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    x = torch.zeros(10, 128, device="cuda")
    p, u = torch.zeros(5, 128, device="cuda"), torch.zeros(2, 64, device="cuda")
    ok = lambda **kw: hip_ops.mha_band(**dict(dict(q=x, k=x, v=x, p=p, pos_bias_u=u, pos_bias_v=u, batch=2, heads=2, w=2), **kw))  # noqa: E731
    assert tuple(ok().shape) == (10, 128)
    for kw, word in ((dict(p=torch.zeros(4, 128, device="cuda")), "p holds T"), (dict(batch=3), "multiple of batch"),
                     (dict(w=-1), "negative"), (dict(t_pad=4), "t_pad"), (dict(pos_bias_u=torch.zeros(2, 32, device="cuda")), "pos_bias_u"),
                     (dict(k=torch.zeros(10, 128, device="cuda", dtype=torch.bfloat16)), "k is"), (dict(q=x.cpu()), "q is"),
                     (dict(v=torch.zeros(10, 256, device="cuda")[:, :128]), "row pitch"),
                     (dict(q=torch.zeros(10, 132, device="cuda")[:, 1:129]), "16-byte")):
        with pytest.raises(_lib.PafcError, match=word):
            ok(**kw)
    torch.cuda.synchronize()
