"""score_attention(backend="kernels") and the three attention decode modes on the GPU: the packed second pass against the
float64 restatement (tests/attn_decoder_ref.py) on the model and hypotheses of the CPU test, no library GEMM on the path, and
the modes once at full dimensions."""
import math

import pytest
import torch

from tests import attn_decoder_ref as REF
from tests import attn_rescore_cases as C
from tests import parity_log

pytestmark = pytest.mark.gpu

_ref_cache = {}


def _reference(normalize_before):
    """(float64 log-probs, float32 CPU log-probs) of the restatement at reverse_weight 0.3 (the left decoder's are those of 0),
    computed once per model."""
    if normalize_before not in _ref_cache:
        model, hyps = C.model(normalize_before), C.hypotheses()
        sd, conf, enc = model.decoder.state_dict(), C.ref_conf(normalize_before), model.encoder.enc_out
        f64 = REF.score_attention(sd, conf, enc, C.LENS, hyps, model.sos, model.eos, 0.3)
        f32 = REF.score_attention(sd, conf, enc, C.LENS, hyps, model.sos, model.eos, 0.3, dtype=torch.float32)
        _ref_cache[normalize_before] = (f64, f32)
    return _ref_cache[normalize_before]


@pytest.mark.parametrize("normalize_before", [True, False], ids=["pre_norm", "post_norm"])
def test_kernels_backend_against_the_float64_restatement(hip, normalize_before):
    """Per-token log-prob error of the kernels backend <= 8 x the error of the restatement's own float32 CPU run against
    float64, with exact fp32 products (decoder.fp32_split_operands = False); with split-operand projections the bound is
    2^-16 / 2^-24 = 256 x wider (the ratio of the unit round-offs).  At this model's row counts (below
    hip_ops.DISPATCH["split_gemm_min_rows"]) both settings take the exact fp32 GEMM; both are measured and recorded.
    Kernels and framework backends pick the same best hypothesis on every utterance whose float64 top-two gap exceeds ten
    times the measured error; at most one utterance may be excluded this way."""
    (l64, r64), (l32, r32) = _reference(normalize_before)
    model, hyps = C.model(normalize_before, dtype=torch.float32).cuda(), C.hypotheses()
    enc = model.encoder.enc_out
    flat64 = {0.0: C.flatten(l64), 0.3: C.flatten(l64) + C.flatten(r64)}
    flat32 = {0.0: C.flatten(l32), 0.3: C.flatten(l32) + C.flatten(r32)}
    for split, widen in ((False, 1.0), (True, 256.0)):
        model.decoder.fp32_split_operands = split
        for rw in (0.0, 0.3):
            got = model.score_attention(enc, C.LENS, hyps, rw, backend="kernels")
            vals = C.flatten(got.l2r_logp) + (C.flatten(got.r2l_logp) if rw > 0 else [])
            assert len(vals) == len(flat64[rw]) and all(math.isfinite(v) for v in vals)
            err = max(abs(a - b) for a, b in zip(vals, flat64[rw]))
            yard = max(abs(a - b) for a, b in zip(flat32[rw], flat64[rw]))
            tag = f"attn_rescore_kernels_{'pre' if normalize_before else 'post'}_{'split' if split else 'exact'}_rw{rw}"
            parity_log.record(tag, max_abs_logp_err=err, cpu_float32_err=yard)
            print(f"{tag}: max|dlogp| {err:.3e}, float32 CPU restatement {yard:.3e}")
            assert err <= 8 * widen * yard, (tag, err, yard)
            assert model.score_attention(enc, C.LENS, hyps, rw).l2r == got.l2r            # None on the GPU: the kernels
            # the same best hypothesis as the framework backend
            fw = model.score_attention(enc, C.LENS, hyps, rw, backend="framework")
            want_attn = REF_attn(l64, r64, rw)
            excluded = 0
            for b, nb in enumerate(hyps):
                if len(nb) < 2:
                    continue
                top = sorted(want_attn[b], reverse=True)
                if top[0] - top[1] <= 10 * err:
                    excluded += 1
                    continue
                best = lambda s: max(range(len(s)), key=lambda i: s[i])              # noqa: E731
                assert best(got.attn(rw)[b]) == best(fw.attn(rw)[b]) == best(want_attn[b]), (tag, b)
            assert excluded <= 1


def test_kernels_backend_split_operand_projections_past_the_row_threshold(hip, monkeypatch):
    """Above hip_ops.DISPATCH["split_gemm_min_rows"] packed rows the fp32 projections with N >= 256 and K % 128 == 0 take the
    split-operand GEMM (2^-16 per product) unless decoder.fp32_split_operands is False: d = 256, 4 heads, 512 units, 8
    hypotheses of 125-160 tokens (1 143 rows) over two memories of 30 and 21 frames.  Bounds as above: exact products 8 x the
    float32 CPU restatement's error, split operands 256 x wider; the two settings must differ, and the
    profiler tells the routes apart: with the switch off no projection of the call, plain or with a residual, runs a split
    kernel.  With the logits cap lowered to 300 rows the output_layer runs in chunks, an utterance alone is cut, and the
    exact-product bound holds."""
    import random
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer import attn_rescore
    rng = random.Random(2)
    hyps = [[[rng.randrange(1, C.V - 1) for _ in range(n)] for n in (125, 160, 141, 150)],
            [[rng.randrange(1, C.V - 1) for _ in range(n)] for n in (139, 128, 155, 137)]]
    lens = [30, 21]
    rows = sum(len(h) + 1 for nb in hyps for h in nb)
    assert rows >= hip_ops.DISPATCH["split_gemm_min_rows"]
    enc = torch.randn(2, 30, 256, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    kw = dict(enc_out=enc, attention_heads=4, linear_units=512)
    m64 = C.model(True, **kw)
    conf = C.ref_conf(True, heads=4)
    l64, r64 = REF.score_attention(m64.decoder.state_dict(), conf, enc, lens, hyps, m64.sos, m64.eos, 0.3)
    l32, r32 = REF.score_attention(m64.decoder.state_dict(), conf, enc, lens, hyps, m64.sos, m64.eos, 0.3, dtype=torch.float32)
    want, cpu32 = C.flatten(l64) + C.flatten(r64), C.flatten(l32) + C.flatten(r32)
    yard = max(abs(a - b) for a, b in zip(cpu32, want))
    model = C.model(True, dtype=torch.float32, **kw).cuda()
    from torch.profiler import ProfilerActivity, profile
    run = lambda: model.score_attention(model.encoder.enc_out, lens, hyps, 0.3, backend="kernels")          # noqa: E731
    got = {}
    for split, widen in ((False, 1.0), (True, 256.0)):
        model.decoder.fp32_split_operands = split
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            s = run()
            torch.cuda.synchronize()
        # the routes told apart: every split-operand projection splits its activation into planes first (split_planes_kernel),
        # and none may with the switch off -- neither that kernel nor the phase-pipelined split GEMM
        names = [e.key for e in prof.key_averages()]
        split_kernels = [n for n in names if "split_planes" in n or "gemm_ph" in n]
        assert bool(split_kernels) == split, (split, split_kernels)
        assert s.stats["rows"] == rows and s.stats["hypotheses"] == 8 and s.stats["chunks"] == 1
        got[split] = C.flatten(s.l2r_logp) + C.flatten(s.r2l_logp)
        err = max(abs(a - b) for a, b in zip(got[split], want))
        parity_log.record(f"attn_rescore_kernels_1143_rows_{'split' if split else 'exact'}", max_abs_logp_err=err,
                          cpu_float32_err=yard)
        print(f"1143 rows, split={split}: max|dlogp| {err:.3e}, float32 CPU restatement {yard:.3e}")
        assert err <= 8 * widen * yard, (split, err, yard)
    assert got[True] != got[False]
    # ... and with the row threshold above this call's rows the switch changes nothing: bit for bit the exact-product values
    monkeypatch.setattr(hip_ops, "_SPLIT_GEMM_MIN_ROWS", rows + 1)
    model.decoder.fp32_split_operands = True
    s = run()
    assert C.flatten(s.l2r_logp) + C.flatten(s.r2l_logp) == got[False]
    monkeypatch.setattr(attn_rescore, "LOGITS_CAP_BYTES", 300 * C.V * 4)     # 300 rows per chunk: an utterance alone is cut too
    model.decoder.fp32_split_operands = False
    s = run()
    assert s.stats["chunks"] >= 4 and s.stats["logits_peak_bytes"] <= 300 * C.V * 4
    chunked = C.flatten(s.l2r_logp) + C.flatten(s.r2l_logp)
    assert max(abs(a - b) for a, b in zip(chunked, want)) <= 8 * yard


def test_kernels_backend_bf16_model_runs_and_is_recorded(hip):
    """A bf16 decoder through the bf16 GEMMs and the bf16 attention kernel: finite log-probabilities of the right shape.  No
    bound for a bf16 stack against the float64 restatement of the fp32 weights can be derived here, so the difference is
    recorded (tests/parity_log.py), not asserted."""
    (l64, r64), _ = _reference(True)
    model, hyps = C.model(True, dtype=torch.float32).cuda(), C.hypotheses()
    model.decoder.to(torch.bfloat16)
    got = model.score_attention(model.encoder.enc_out, C.LENS, hyps, 0.3, backend="kernels")
    vals = C.flatten(got.l2r_logp) + C.flatten(got.r2l_logp)
    want = C.flatten(l64) + C.flatten(r64)
    assert len(vals) == len(want) and all(math.isfinite(v) and v < 1e-3 for v in vals)
    parity_log.record("attn_rescore_kernels_bf16_model", max_abs_logp_diff=max(abs(a - b) for a, b in zip(vals, want)))


def REF_attn(l64, r64, rw):
    out = []
    for b in range(len(l64)):
        out.append([sum(l) if rw == 0 else (1 - rw) * sum(l) + rw * sum(r) for l, r in zip(l64[b], r64[b])])
    return out


def test_score_attention_calls_no_library_gemm(hip, monkeypatch):
    """Under torch.profiler a score_attention call lists no library GEMM kernel (rocBLAS / hipBLASLt "Cijk_", at::native
    gemm / gemv), and F.linear / torch.matmul / torch.bmm are not called at all on the kernels path: the framework's fp32 GEMM
    stalls when two streams issue it."""
    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile
    model, hyps = C.model(True, dtype=torch.float32).cuda(), C.hypotheses()
    enc = model.encoder.enc_out
    want = model.score_attention(enc, C.LENS, hyps, 0.3, backend="kernels")              # (warm: stacked weights, library load)

    def refuse(*a, **k):
        raise AssertionError("a library GEMM was called on the second pass")
    monkeypatch.setattr(F, "linear", refuse)
    monkeypatch.setattr(torch, "bmm", refuse)
    monkeypatch.setattr(torch, "matmul", refuse)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        got = model.score_attention(enc, C.LENS, hyps, 0.3, backend="kernels")
        torch.cuda.synchronize()
    assert got.l2r == want.l2r and got.r2l == want.r2l
    names = [e.key for e in prof.key_averages()]
    assert any("mha_rows_kernel" in n for n in names) and any("logp_gather_kernel" in n for n in names), names
    bad = [n for n in names if "Cijk_" in n or ("gemm" in n.lower() and "at::native" in n)
           or n in ("aten::mm", "aten::addmm", "aten::bmm")]
    assert not bad, bad


@pytest.fixture(scope="module")
def full_model():
    """d = 512, 8 heads, V = 5000, 3 + 3 blocks, B = 2, short inputs: a Transducer around a fixed encoder output."""
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder
    torch.manual_seed(5)
    vocab, dim = 5000, 512
    enc_out = torch.randn(2, 24, dim)
    dec = BiTransformerDecoder(vocab, dim, attention_heads=8, linear_units=2048, num_blocks=3, r_num_blocks=3)
    model = Transducer(vocab, 0, C.FixedEncoder(enc_out), RNNPredictor(vocab, 256, 256, 0.1, 256, 2, True, "lstm", 0.1),
                       TransducerJoint(vocab, dim, 256, 256), ctc=CTC(vocab, dim), attention_decoder=dec).eval().cuda()
    return model, torch.zeros(2, 24, 2, device="cuda"), torch.tensor([24, 13], device="cuda")


def test_modes_at_full_dimensions(hip, full_model):
    from paper_accurate_fast_cheap_amd.transformer import attn_rescore
    model, speech, lens = full_model
    alone = model.score_attention(model.encoder.enc_out, lens, [[[7, 8, 9], []], [[5]]], 0.3)
    assert alone.stats["rows"] == 7 and 0 < alone.stats["logits_peak_bytes"] <= attn_rescore.LOGITS_CAP_BYTES
    modes = ["attention_rescoring", "ctc_beam_td_attn_rescoring", "rnnt_beam_attn_rescoring"]
    rw, wa, wc, wt = 0.3, 0.5, 0.3, 0.7
    out = model.decode(["ctc_prefix_beam_search", "rnnt_beam_search"] + modes, speech, lens, beam_size=4, ctc_weight=wc,
                       transducer_weight=wt, attn_weight=wa, reverse_weight=rw, search_ctc_weight=wc, search_transducer_weight=wt)
    for mode in modes:
        first = out["rnnt_beam_search" if mode.startswith("rnnt") else "ctc_prefix_beam_search"]
        for r1, r2 in zip(first, out[mode]):
            assert sorted(map(tuple, r2.nbest)) == sorted(map(tuple, r1.nbest))            # the first pass's hypothesis set
            n = len(r2.nbest)
            assert n >= 1 and len(r2.nbest_scores) == len(r2.nbest_attn_scores) == n
            assert all(math.isfinite(v) for v in r2.nbest_scores + r2.nbest_attn_scores)
            assert all(a >= b for a, b in zip(r2.nbest_scores, r2.nbest_scores[1:]))
            assert r2.tokens == r2.nbest[0] and r2.score == r2.nbest_scores[0]
            assert 0.0 < r2.confidence <= 1.0 and len(r2.tokens_confidence) == len(r2.tokens)
            assert all(0.0 <= c <= 1.0 for c in r2.tokens_confidence)
            firsts = {tuple(h): s for h, s in zip(r1.nbest, r1.nbest_scores)}
            for i, h in enumerate(r2.nbest):                                                # final from the raw terms
                if mode == "attention_rescoring":
                    assert r2.nbest_td_scores is None
                    want = r2.nbest_attn_scores[i] + wc * firsts[tuple(h)]
                else:
                    want = wa * r2.nbest_attn_scores[i] + wc * firsts[tuple(h)] + wt * r2.nbest_td_scores[i]
                assert r2.nbest_scores[i] == pytest.approx(want, rel=1e-9, abs=1e-9)
