"""The attention decoder's beam search, the checks that need no GPU: forward_one_step against forward, the framework backend of
attention_beam_search against the float64 restatement (tests/attn_search_ref.py) and against what the reference's own loop
decoded on this decoder (tests/golden/attn_search_tokens.json), the decode modes and the refusals.

The shared case: tests/attn_rescore_cases.py's models (d = 128, 2 heads, V = 53) in float64 with output_layer.bias[eos] raised by
EOS_BOOST = 0.5, the value at which the float64 search shows everything the masks and the freeze exist for
(test_the_case_exercises_the_search asserts it): utterances whose beams all end long before the cap, utterances that run into it,
and steps in which ended and live beams of one utterance stand side by side."""
import functools
import json
import math
import os

import pytest
import torch

from tests import attn_rescore_cases as C
from tests import attn_search_ref as SR

EOS_BOOST = 0.5
T = max(C.LENS)


def search_model(normalize_before: bool, dtype=torch.float64, sos=None, **kw):
    model = C.model(normalize_before, dtype=torch.float64, **kw)
    with torch.no_grad():
        model.decoder.left_decoder.output_layer.bias[model.eos] += EOS_BOOST
    if sos is not None:
        model.sos = sos
    return model.to(dtype)


def batch_mask():
    return (torch.arange(T)[None, :] < torch.tensor(C.LENS)[:, None]).unsqueeze(1)


def case_inputs(which):
    """"batch": the three utterances padded to 70 frames; 0 / 1 / 2: one utterance alone at its own length (the cap)."""
    enc = C.encoder_out()
    if which == "batch":
        return enc, batch_mask()
    n = C.LENS[which]
    return enc[which:which + 1, :n], torch.ones(1, 1, n, dtype=torch.bool)


@functools.lru_cache(maxsize=None)
def restated(normalize_before: bool, beam: int, which, sos=None):
    """The float64 restatement's search of a case, computed once and shared (nobody changes it)."""
    model = search_model(normalize_before, sos=sos)
    enc, mask = case_inputs(which)
    return SR.search(model.decoder.state_dict(), C.ref_conf(normalize_before), enc, mask, model.sos, model.eos, beam)


def same(a: float, b: float, tol: float) -> bool:
    if math.isinf(a) or math.isinf(b) or math.isnan(a) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= tol


def check_against(results, ref, eos, lp):
    fin = SR.finish(ref, eos, lp)
    assert [r.tokens for r in results] == fin["best"]
    for b, r in enumerate(results):
        assert r.nbest == fin["nbest"][b] and r.tokens == r.nbest[0] and r.score == r.nbest_scores[0]
        assert len(r.nbest_scores) == len(fin["nbest_scores"][b])
        for got, want in zip(r.nbest_scores, fin["nbest_scores"][b]):
            assert same(got, want, 1e-10), (got, want)


@pytest.mark.parametrize("beam", [1, 4, 10])
@pytest.mark.parametrize("normalize_before", [True, False])
def test_framework_backend_equals_the_float64_restatement(normalize_before, beam):
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    for which, sos in (("batch", None), ("batch", 1), (0, None), (1, None), (2, None)):
        model = search_model(normalize_before, sos=sos)
        assert (model.sos == model.eos) == (sos is None)
        enc, mask = case_inputs(which)
        ref = restated(normalize_before, beam, which, sos)
        for lp in (0.0, 0.6):
            got = attention_beam_search(model, enc, mask, beam, lp, backend="framework", return_trace=True)
            check_against(got, ref, model.eos, lp)
            tr = got[0].trace
            assert tr["parent"].shape == (ref["steps"], enc.size(0) * beam)
            assert tr["parent"].tolist() == ref["parent"] and tr["token"].tolist() == ref["token"]
            assert got[0].stats is None
        # None on the CPU is the framework backend; max_len lowers the cap and the result is the capped search's
        assert [r.nbest for r in attention_beam_search(model, enc, mask, beam, 0.6)] == [r.nbest for r in got]
    model = search_model(normalize_before)
    enc, mask = case_inputs("batch")
    short = attention_beam_search(model, enc, mask, beam, 0.0, backend="framework", max_len=5)
    ref5 = SR.search(model.decoder.state_dict(), C.ref_conf(normalize_before), enc, mask, model.sos, model.eos, beam, max_len=5)
    assert ref5["steps"] <= 5
    check_against(short, ref5, model.eos, 0.0)


def test_the_case_exercises_the_search():
    """Without these the masks and the freeze would not be tested: the float64 search of the shared case must show them."""
    cap = T
    # every utterance's beams all end before the cap: the loop breaks early
    early = restated(True, 4, "batch")
    assert early["steps"] < cap and all(bool(f) for f in early["flags"][-1].reshape(-1))
    # an utterance that runs into the cap, next to (post-norm) utterances that ended long before
    for pre in (True, False):
        late = restated(pre, 10, "batch")
        assert late["steps"] == cap and not late["flags"][-1].all()
    post = restated(False, 10, "batch")
    ended_at = [next((i for i, f in enumerate(post["flags"]) if f[b].all()), None) for b in range(3)]
    assert ended_at[0] is not None and ended_at[0] < cap - 1 and ended_at[2] is None
    # T' = 1 alone: exactly one step
    for beam in (1, 4, 10):
        assert restated(True, beam, 0)["steps"] == 1
    # steps where ended and live beams of one utterance coexist
    for ref in (early, post):
        assert sum(bool(f[b].any() and not f[b].all()) for f in ref["flags"] for b in range(3)) >= 3
    # with sos == eos the best hypothesis of some utterance at beam 10 is short: the zero-length rule is within reach
    assert min(len(h) for h in SR.finish(early, C.V - 1, 0.6)["best"]) <= 2


def test_length_penalty_of_a_zero_length_row():
    """lengths = hyps.ne(eos).sum(1) over the whole row: with sos == eos a row of nothing but eos has length 0; 0 ** 0 = 1 keeps
    its score, a positive penalty divides by 0 (search.py:347-348).  Both backends' host code mirrors that."""
    from paper_accurate_fast_cheap_amd.transformer.attn_search import penalised
    import numpy as np
    eos = 7
    hyps = [[eos, eos], [3, eos], [3, 4]]
    sc = np.array([-1.5, -2.0, -3.0], dtype=np.float32)
    assert penalised(sc, hyps, eos, eos, 0.0) == [-1.5, -2.0, -3.0]
    got = penalised(sc, hyps, eos, eos, 0.6)
    assert got[0] == -math.inf and got[1] == -2.0 and got[2] == pytest.approx(-3.0 / 2 ** 0.6, abs=1e-12)
    got = penalised(sc, hyps, 1, eos, 0.6)                                  # sos != eos: the prefix counts
    assert got[0] == -1.5 and got[1] == pytest.approx(-2.0 / 2 ** 0.6, abs=1e-12)
    ref = dict(hyps=torch.tensor([[[eos, eos, eos], [eos, 3, eos], [eos, 3, 4]]]), raw=torch.tensor([[-1.5, -2.0, -3.0]],
               dtype=torch.float64))
    fin = SR.finish(ref, eos, 0.6)
    # -3 / 2 ** 0.6 = -1.979 beats -2 / 1; the all-eos row divides by zero and comes last
    assert fin["best"] == [[3, 4]] and fin["nbest"] == [[[3, 4], [3], []]] and fin["nbest_scores"][0][2] == -math.inf


def test_reference_loop_decodes_the_same_tokens():
    """tests/golden/attn_search_tokens.json (make_goldens_attn_search.py): what the reference's own attention_beam_search
    returned on this project's decoder for the batched case."""
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    with open(os.path.join(os.path.dirname(__file__), "golden", "attn_search_tokens.json")) as f:
        gold = json.load(f)
    assert gold["eos_boost"] == EOS_BOOST and len(gold["cases"]) == 12
    enc, mask = case_inputs("batch")
    for case in gold["cases"]:
        model = search_model(case["normalize_before"])
        got = attention_beam_search(model, enc, mask, case["beam"], case["length_penalty"], backend="framework")
        assert [r.tokens for r in got] == case["tokens"], case


@pytest.mark.parametrize("normalize_before", [True, False])
def test_forward_one_step_equals_the_last_row_of_forward(normalize_before):
    from paper_accurate_fast_cheap_amd.transformer.decoder import subsequent_mask
    model = search_model(normalize_before)
    g = torch.Generator().manual_seed(5)
    enc, mask = case_inputs("batch")
    L = 9
    ys = torch.randint(0, C.V, (3, L), generator=g)
    for dec in (model.decoder, model.decoder.left_decoder):
        left = model.decoder.left_decoder
        cache = None
        with torch.no_grad():
            for i in range(1, L + 1):
                logp, cache = dec.forward_one_step(enc, mask, ys[:, :i], subsequent_mask(i)[None].repeat(3, 1, 1), cache)
                full, _, _ = left(enc, mask, ys[:, :i], torch.full((3,), i))
                want = torch.log_softmax(full[:, -1], dim=-1)
                assert (logp - want).abs().max().item() <= 1e-10
                assert len(cache) == len(left.decoders) and all(c.shape == (3, i, C.D) for c in cache)
                # and without a cache the method computes every row again: the same numbers
                cold, cold_cache = dec.forward_one_step(enc, mask, ys[:, :i], subsequent_mask(i)[None].repeat(3, 1, 1), None)
                assert (cold - want).abs().max().item() <= 1e-10
                assert max((a - b).abs().max().item() for a, b in zip(cache, cold_cache)) <= 1e-10


@pytest.mark.parametrize("normalize_before", [True, False])
def test_forward_without_a_cache_keeps_its_bits(normalize_before):
    """DecoderLayer.forward(cache=None) is the expression it was before it learnt about caches, evaluated in the same order."""
    model = search_model(normalize_before, dtype=torch.float32)
    layer = model.decoder.left_decoder.decoders[0]
    g = torch.Generator().manual_seed(9)
    x, mem = torch.randn(3, 6, C.D, generator=g), torch.randn(3, 11, C.D, generator=g)
    tgt_mask = torch.ones(6, 6, dtype=torch.bool).tril()[None].repeat(3, 1, 1)
    mem_mask = torch.ones(3, 1, 11, dtype=torch.bool)
    with torch.no_grad():
        got = layer(x, tgt_mask, mem, mem_mask)[0]
        if normalize_before:
            y = layer.norm1(x)
            w = x + layer.dropout(layer.self_attn(y, y, y, tgt_mask))
            w = w + layer.dropout(layer.src_attn(layer.norm2(w), mem, mem, mem_mask))
            w = w + layer.dropout(layer.feed_forward(layer.norm3(w)))
        else:
            w = layer.norm1(x + layer.dropout(layer.self_attn(x, x, x, tgt_mask)))
            w = layer.norm2(w + layer.dropout(layer.src_attn(w, mem, mem, mem_mask)))
            w = layer.norm3(w + layer.dropout(layer.feed_forward(w)))
        assert torch.equal(got, w)
        assert torch.equal(layer(x, tgt_mask, mem, mem_mask, cache=None)[0], w)


def _transducer():
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder
    torch.manual_seed(3)
    vocab, dim = 8, 6
    enc_out = torch.randn(3, 6, dim) * 1.5
    dec = BiTransformerDecoder(vocab, dim, attention_heads=2, linear_units=10, num_blocks=1, r_num_blocks=1)
    model = Transducer(vocab, 0, C.FixedEncoder(enc_out), RNNPredictor(vocab, 4, 7, 0.0, 7, 1, dropout=0.0),
                       TransducerJoint(vocab, dim, 7, 5), ctc=CTC(vocab, dim), attention_decoder=dec).eval()
    return model.to(torch.float64), torch.zeros(3, 6, 2, dtype=torch.float64), torch.tensor([6, 4, 1])


def test_decode_modes_equal_the_direct_call():
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    model = search_model(True)
    speech, lens = torch.zeros(3, T, 2, dtype=torch.float64), torch.tensor(C.LENS)
    tmodel, tspeech, tlens = _transducer()
    tmask = (torch.arange(6)[None, :] < tlens[:, None]).unsqueeze(1)
    for m, sp, ln, enc, mask, beam in ((model, speech, lens, model.encoder.enc_out, batch_mask(), 4),
                                       (tmodel, tspeech, tlens, tmodel.encoder.enc_out, tmask, 3)):
        out = m.decode(["attention_beam_search", "ctc_greedy_search"], sp, ln, beam_size=beam, length_penalty=0.6)
        assert sorted(out) == ["attention_beam_search", "ctc_greedy_search"]
        direct = attention_beam_search(m, enc, mask, beam, 0.6)
        assert [r.nbest for r in out["attention_beam_search"]] == [r.nbest for r in direct]
        assert [r.nbest_scores for r in out["attention_beam_search"]] == [r.nbest_scores for r in direct]
        plain = m.decode(["attention_beam_search"], sp, ln, beam_size=beam, score_backend="framework")["attention_beam_search"]
        assert [r.nbest for r in plain] == [r.nbest for r in attention_beam_search(m, enc, mask, beam, 0.0)]


def test_refusals():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    model = search_model(True)
    enc, mask = case_inputs("batch")
    speech, lens = torch.zeros(3, T, 2, dtype=torch.float64), torch.tensor(C.LENS)
    # no decoder
    bare = ASRModel(C.V, C.FixedEncoder(enc), CTC(C.V, C.D)).eval().double()
    with pytest.raises(NotImplementedError, match="needs an attention decoder"):
        attention_beam_search(bare, enc, mask, 4)
    with pytest.raises(NotImplementedError, match="'attention_beam_search' needs an attention decoder"):
        bare.decode(["attention_beam_search"], speech, lens)
    tmodel, tspeech, tlens = _transducer()
    tmodel.decoder = None
    with pytest.raises(NotImplementedError, match="'attention_beam_search' needs an attention decoder"):
        tmodel.decode(["attention_beam_search"], tspeech, tlens, beam_size=3)
    # the reference's spelling is still refused, and says where the mode lives
    for m, sp, ln in ((model, speech, lens), (_transducer()[0], tspeech, tlens)):
        with pytest.raises(NotImplementedError, match="attention_beam_search"):
            m.decode(["attention"], sp, ln, beam_size=3)
    # the kernels backend is never a fallback
    for beam in (0, 17):
        with pytest.raises(PafcError, match=rf"a beam of {beam} "):
            attention_beam_search(model, enc, mask, beam, backend="kernels")
    small = search_model(True)
    small.vocab_size = 8
    with pytest.raises(PafcError, match="a vocabulary of 8 for a beam of 10"):
        attention_beam_search(small, enc, mask, 10, backend="kernels")
    with pytest.raises(PafcError, match="not on the GPU"):
        attention_beam_search(model, enc, mask, 4, backend="kernels")
    with pytest.raises(ValueError, match="backend"):
        attention_beam_search(model, enc, mask, 4, backend="eager")
    with pytest.raises(ValueError):
        attention_beam_search(model, enc, mask, 0, backend="framework")
    with pytest.raises(ValueError, match="step_graph"):
        attention_beam_search(model, enc, mask, 4, backend="framework", step_graph=True)
    with pytest.raises(ValueError, match="max_len"):
        attention_beam_search(model, enc, mask, 4, max_len=0)
    with pytest.raises(ValueError, match="encoder_mask"):
        attention_beam_search(model, enc, mask[:, :, :5], 4)


def test_search_kernels_validate_before_they_launch():
    """pafc_mha_step / pafc_attn_beam_select answer bad arguments with a PAFC_ERR_* before anything is launched: callable on a
    machine without a GPU (the library builds here with hipcc; skipped where neither hipcc nor a built library exists)."""
    import ctypes
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    for name in ("pafc_mha_step", "pafc_attn_beam_select", "pafc_attn_beam_select_workspace_bytes"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]   # (a private handle, not the package's)
    one, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)      # non-null, 16-byte aligned, never dereferenced

    def step(dtype=0, R=8, N=4, H=2, dk=64, P=5, qkv=one, ldqkv=384, anc=one, ldo=128):
        return L.pafc_mha_step(dtype, R, N, H, dk, P, qkv, ldqkv, one, anc, one, one, one, ldo, NULL)

    assert step(qkv=NULL) == -1 and step(anc=NULL) == -1 and step(dtype=2) == -6
    assert step(R=0) == -2 and step(R=7) == -2 and step(H=0) == -2 and step(P=0) == -2       # R a multiple of N
    assert step(P=1 << 30) == -2                                                               # P * R beyond an int
    assert step(dk=32) == -7 and step(R=34, N=17) == -7                                        # heads of 64, beams up to 16
    assert step(ldqkv=256) == -2 and step(ldo=64) == -2 and step(ldqkv=386) == -2 and step(dtype=1, ldo=132) == -2
    assert step(qkv=ctypes.c_void_p(8)) == -8

    assert L.pafc_attn_beam_select_workspace_bytes(3, 4) == 3 * 4 * 4 * 12
    assert L.pafc_attn_beam_select_workspace_bytes(0, 4) == 0 and L.pafc_attn_beam_select_workspace_bytes(3, 17) == 0

    def select(dtype=0, B=2, N=4, V=53, P=6, cap=5, eos=52, logits=one, ldl=53, done=one, ws=one, ws_bytes=1 << 20):
        return L.pafc_attn_beam_select(dtype, B, N, V, P, cap, eos, logits, ldl, one, one, one, one, one, one, one, one, done, ws,
                                       ws_bytes, NULL)

    assert select(logits=NULL) == -1 and select(done=NULL) == -1 and select(ws=NULL) == -1 and select(dtype=4) == -6
    assert select(B=0) == -2 and select(N=0) == -2 and select(ldl=52) == -2 and select(eos=53) == -2 and select(eos=-1) == -2
    assert select(cap=0) == -2 and select(cap=6) == -2 and select(P=1, cap=1) == -2            # 1 <= cap < P
    assert select(N=17) == -7 and select(N=4, V=3, eos=2, ldl=3) == -7                         # beams up to 16, V >= N
    assert select(ws_bytes=2 * 4 * 4 * 12 - 1) == -4 and select(ws=ctypes.c_void_p(18)) == -8
