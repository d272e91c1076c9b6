"""Joint CTC/attention decoding (transformer/joint_search.py), the checks that need no GPU: the framework backend against the
float64 restatement (tests/joint_search_ref.py) and against what the reference's own BeamSearchTimeSync returned on this decoder
(tests/golden/joint_search.json), the decode modes, the refusals and the new entry point's error codes.

The shared case: tests/attn_rescore_cases.py's models (d = 128, 2 heads, V = 53) in float64 and their three utterances of 1, 17
and 70 frames.  That model's random CTC head emits a token on almost every frame, so ctc_lo.bias[blank] is raised by BLANK_BOOST
= 1.0, the value at which the float64 search is blank-dominated and still shows every quirk of the reference
(test_the_case_exercises_the_search asserts it); and since no frame of it reaches a blank probability of 0.9, the frames
SKIP_FRAMES of every utterance get SKIP_BOOST more on the blank logit, which puts them above it."""
import ctypes
import functools
import json
import math
import os

import pytest
import torch

from tests import attn_rescore_cases as C
from tests import joint_search_ref as JR

BLANK_BOOST = 1.0
SKIP_BOOST = 6.0
SKIP_FRAMES = (9, 30, 31, 55)
T = max(C.LENS)
SETTINGS = ((0.5, 0.5, 1.0), (0.3, 0.0, 1.0), (1.0, 0.5, 1.0), (0.5, 0.5, 0.9), (0.3, 0.5, 0.9), (1.0, 0.0, 0.9))   # ctc_w, bonus, thr


def joint_model(normalize_before: bool, dtype=torch.float64, **kw):
    model = C.model(normalize_before, dtype=torch.float64, **kw)
    with torch.no_grad():
        model.ctc.ctc_lo.bias[0] += BLANK_BOOST
    return model.to(dtype)


@functools.lru_cache(maxsize=None)
def ctc_case(normalize_before: bool = True):
    """(3, 70, V) float32 CTC log-probabilities of the shared case (computed in float64; nobody changes them)."""
    model = joint_model(normalize_before)
    with torch.no_grad():
        logits = model.ctc.ctc_lo(C.encoder_out())
        for t in SKIP_FRAMES:
            logits[:, t, 0] += SKIP_BOOST
        return logits.log_softmax(-1).float()


@functools.lru_cache(maxsize=None)
def shared_logp(normalize_before: bool, which: int):
    """The float64 decoder of utterance `which` as logp(prefix), each prefix forwarded once for all searches that ask."""
    model = joint_model(normalize_before)
    inner = JR.decoder_logp(model.decoder.state_dict(), C.ref_conf(normalize_before), C.encoder_out()[which, :C.LENS[which]])
    memo = {}

    def logp(prefix):
        if prefix not in memo:
            memo[prefix] = inner(prefix)
        return memo[prefix]
    return logp


@functools.lru_cache(maxsize=None)
def restated(normalize_before: bool, beam: int, which: int, ctc_weight=0.5, bonus=0.5, threshold=1.0):
    """The float64 restatement's search of one utterance, run once and shared (nobody changes it)."""
    model = joint_model(normalize_before)
    s = JR.Search(ctc_case(normalize_before)[which, :C.LENS[which]], shared_logp(normalize_before, which), model.sos, beam,
                  ctc_weight, bonus, blank_threshold=threshold)
    s.run()
    return s


def same(a: float, b: float, tol: float = 1e-10) -> bool:
    if math.isinf(a) or math.isinf(b) or math.isnan(a) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= tol


def check_against(result, search: JR.Search, tol: float = 1e-10):
    want = search.result()
    assert result.nbest == want["nbest"] and result.tokens == want["nbest"][0]
    assert result.nbest_times == want["nbest_times"] and result.times == want["nbest_times"][0]
    assert result.end_times == want["nbest_end_times"][0]
    assert result.stats["nbest_end_times"] == want["nbest_end_times"]
    assert len(result.nbest_scores) == len(want["nbest_scores"]) and result.score == result.nbest_scores[0]
    for got, ref in zip(result.nbest_scores, want["nbest_scores"]):
        assert same(got, ref, tol), (got, ref)
    for got, ref in zip(result.stats["nbest_tokens_confidence"], want["nbest_confidence"]):
        assert len(got) == len(ref) and all(same(g, r, tol) for g, r in zip(got, ref)), (got, ref)
    assert result.tokens_confidence == result.stats["nbest_tokens_confidence"][0]


@pytest.mark.parametrize("beam", [1, 4, 10])
@pytest.mark.parametrize("normalize_before", [True, False])
def test_framework_backend_equals_the_float64_restatement(normalize_before, beam):
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    model = joint_model(normalize_before)
    dec = model.decoder.left_decoder
    enc, ctc, lens = C.encoder_out(), ctc_case(normalize_before), torch.tensor(C.LENS)
    calls = []
    real = dec.forward_one_step
    dec.forward_one_step = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    for n, (ctc_w, bonus, thr) in enumerate(SETTINGS):
        del calls[:]
        got = joint_decoding(model, enc, lens, ctc, ctc_w, beam, 1.5, bonus, blank_threshold=thr, backend="framework",
                             return_trace=True)
        refs = [restated(normalize_before, beam, b, ctc_w, bonus, thr) for b in range(3)]
        for b in range(3):
            check_against(got[b], refs[b])
            frames = refs[b].frames
            assert got[b].trace["beam"] == [[list(h[1:]) for h in f["beam"]] for f in frames]
            assert got[b].stats["frames_skipped"] == sum(f["skipped"] for f in frames)
            # a prefix is decoded at most once per utterance, and exactly the prefixes the restatement asked for
            assert got[b].stats["decoder_evaluations"] == len(refs[b].rows)
        assert len(calls) == sum(len(r.rows) for r in refs)
        if ctc_w == 1.0:
            assert not calls                                              # dec_w == 0: the decoder is never run
        if n == 0:
            # None on the CPU is the framework backend; an utterance alone gives what it gives in the batch
            again = joint_decoding(model, enc, C.LENS, ctc, ctc_w, beam, 1.5, bonus)
            assert [r.nbest for r in again] == [r.nbest for r in got] and again[0].trace is None
            for b, L in enumerate(C.LENS):
                alone = joint_decoding(model, enc[b:b + 1, :L], [L], ctc[b:b + 1, :L], ctc_w, beam, 1.5, bonus)
                check_against(alone[0], refs[b])


def test_the_case_exercises_the_search():
    """Without these the quirks would not be tested: the float64 search of the shared case must show them."""
    from paper_accurate_fast_cheap_amd.transformer.attn_search import MAX_BEAM
    from paper_accurate_fast_cheap_amd.transformer.joint_search import MAX_PRE_BEAM
    runs = [restated(pre, beam, b) for pre in (True, False) for beam in (1, 4, 10) for b in range(3)]
    assert all(s.beam <= MAX_BEAM and s.pre_beam <= MAX_PRE_BEAM for s in runs)     # the case is one the kernels backend takes
    executed = lambda s: [f for f in s.frames if not f["skipped"]]                             # noqa: E731
    total = lambda key, which=runs: sum(f[key] for s in which for f in executed(s))           # noqa: E731
    assert total("repeated") > 0            # a repeated-token update
    assert total("dropped") > 0             # a beam prefix dropped because blank was no candidate
    assert total("reentry") > 0             # "considered before"
    assert total("back_on_beam") > 0        # a prefix that was on the beam (decoded once) comes back to it
    assert sum(s.result()["stale"] for s in runs) > 0      # a reported end frame / confidence that is the snapshot's
    for beam in (4, 10):                    # and in the runs the GPU tests use, not only somewhere
        mine = [restated(True, beam, b) for b in (1, 2)]
        assert total("repeated", mine) and total("dropped", mine) and total("reentry", mine)
        assert sum(s.result()["stale"] for s in mine)
    # frames skipped under blank_threshold = 0.9, none under 1.0
    skipped = [sum(f["skipped"] for f in restated(True, 4, b, 0.5, 0.5, 0.9).frames) for b in range(3)]
    assert skipped[0] == 0 and skipped[1] >= 1 and skipped[2] >= 2
    assert all(not f["skipped"] for s in runs for f in s.frames)
    # beam 1: pre_beam_size is 1 and the 17-frame utterance ends at -inf
    for pre in (True, False):
        s = restated(pre, 1, 1)
        assert s.pre_beam == 1 and s.result()["nbest_scores"] == [-math.inf] and len(s.result()["nbest"][0]) > 0
    # no ties of either kind
    for s in runs + [restated(pre, beam, b, *st) for pre in (True, False) for beam in (1, 4, 10) for b in range(3)
                     for st in SETTINGS[1:]]:
        assert not any(f["pre_beam_tie"] or f["score_tie"] for f in executed(s))


def test_reference_class_decodes_the_same():
    """tests/golden/joint_search.json (make_goldens_joint_search.py): what the reference's own BeamSearchTimeSync returned on
    this project's decoder with sos = model.sos.  It hands scores and confidences back as float32 tensors, so these two are
    held to float32's rounding (rel 1e-6); tokens and frames are exact."""
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    with open(os.path.join(os.path.dirname(__file__), "golden", "joint_search.json")) as f:
        gold = json.load(f)
    assert gold["blank_boost"] == BLANK_BOOST and gold["skip_boost"] == SKIP_BOOST and gold["skip_frames"] == list(SKIP_FRAMES)
    assert len(gold["cases"]) == 2 * 3 * 3
    enc, lens = C.encoder_out(), torch.tensor(C.LENS)
    for case in gold["cases"]:
        model = joint_model(case["normalize_before"])
        got = joint_decoding(model, enc, lens, ctc_case(case["normalize_before"]), case["ctc_weight"], case["beam"], 1.5,
                             case["length_bonus"], blank_threshold=case["blank_threshold"], backend="framework")
        for r, want in zip(got, case["utterances"]):
            assert r.tokens == want["tokens"] and r.times == want["times"] and r.end_times == want["end_times"], case
            score = -math.inf if want["score"] is None else want["score"]
            assert r.score == score or r.score == pytest.approx(score, rel=1e-6), case
            assert r.tokens_confidence == pytest.approx(want["tokens_confidence"], rel=1e-6, abs=1e-30), case


def test_every_frame_skipped_gives_the_empty_hypothesis():
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    model = joint_model(True)
    ctc = torch.full((1, 5, C.V), -20.0)
    ctc[:, :, 0] = math.log(0.95)
    got = joint_decoding(model, C.encoder_out()[:1, :5], [5], ctc, blank_threshold=0.9)[0]
    assert got.tokens == [] and got.score == 0.0 and got.nbest == [[]] and got.nbest_scores == [0.0] and got.times == []
    assert got.stats["frames_skipped"] == 5 and got.stats["decoder_evaluations"] == 0
    s = JR.Search(ctc[0], None, model.sos, 4, blank_threshold=0.9)
    assert s.run()["nbest"] == [[]]
    empty = joint_decoding(model, C.encoder_out()[:1, :5], [0], ctc)[0]                      # no frames at all
    assert empty.tokens == [] and empty.score == 0.0


def _transducer():
    from tests.test_attn_search import _transducer as make
    return make()


def test_decode_modes_equal_the_direct_call():
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    model = joint_model(True)
    speech, lens = torch.zeros(3, T, 2, dtype=torch.float64), torch.tensor(C.LENS)
    tmodel, tspeech, tlens = _transducer()
    for m, sp, ln, beam in ((model, speech, lens, 4), (tmodel, tspeech, tlens, 3)):
        enc = m.encoder.enc_out
        ctc = m.ctc_logprobs(enc)
        out = m.decode(["joint_decoding", "ctc_greedy_search"], sp, ln, beam_size=beam, ctc_weight=0.3, length_penalty=0.25)
        assert sorted(out) == ["ctc_greedy_search", "joint_decoding"]
        direct = joint_decoding(m, enc, ln, ctc, ctc_weight=0.3, beam_size=beam, length_bonus=0.25)
        for a, b in zip(out["joint_decoding"], direct):
            assert a.nbest == b.nbest and a.nbest_scores == b.nbest_scores and a.times == b.times and a.end_times == b.end_times
            assert a.tokens_confidence == b.tokens_confidence
        plain = m.decode(["joint_decoding"], sp, ln, beam_size=beam, score_backend="framework")["joint_decoding"]
        want = joint_decoding(m, enc, ln, ctc, ctc_weight=0.0, beam_size=beam, length_bonus=0.0)     # decode()'s own defaults
        assert [r.nbest for r in plain] == [r.nbest for r in want]


def test_refusals():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    model = joint_model(True)
    enc, ctc, lens = C.encoder_out(), ctc_case(), C.LENS
    speech, slens = torch.zeros(3, T, 2, dtype=torch.float64), torch.tensor(C.LENS)
    bare = ASRModel(C.V, C.FixedEncoder(enc), CTC(C.V, C.D)).eval().double()
    with pytest.raises(NotImplementedError, match="needs an attention decoder"):
        joint_decoding(bare, enc, lens, ctc)
    with pytest.raises(NotImplementedError, match="'joint_decoding' needs an attention decoder"):
        bare.decode(["joint_decoding"], speech, slens)
    tmodel, tspeech, tlens = _transducer()
    tmodel.decoder = None
    with pytest.raises(NotImplementedError, match="'joint_decoding' needs an attention decoder"):
        tmodel.decode(["joint_decoding"], tspeech, tlens, beam_size=3)
    with pytest.raises(ValueError, match="cat_embs"):
        joint_decoding(model, enc, lens, ctc, cat_embs=torch.zeros(1))
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match="ctc_weight"):
            joint_decoding(model, enc, lens, ctc, ctc_weight=w)
    with pytest.raises(ValueError, match="pre_beam_size"):
        joint_decoding(model, enc, lens, ctc, beam_size=1, pre_beam_ratio=0.5)               # int(0.5) = 0
    with pytest.raises(ValueError, match="pre_beam_size"):
        joint_decoding(model, enc, lens, ctc, beam_size=40)                                   # 60 candidates of 53 tokens
    with pytest.raises(ValueError, match="pre_beam_size"):
        joint_decoding(model, enc, lens, ctc, beam_size=0)
    with pytest.raises(ValueError, match="blank_threshold"):
        joint_decoding(model, enc, lens, ctc, blank_threshold=0.0)
    with pytest.raises(ValueError, match="ctc_probs"):
        joint_decoding(model, enc, lens, ctc[:, :5])
    with pytest.raises(ValueError, match="encoder_lens"):
        joint_decoding(model, enc, [1, 2], ctc)
    with pytest.raises(ValueError, match="backend"):
        joint_decoding(model, enc, lens, ctc, backend="eager")
    # the kernels backend is never a fallback
    for beam in (17, 20):
        with pytest.raises(PafcError, match=rf"a beam of {beam} "):
            joint_decoding(model, enc, lens, ctc, beam_size=beam, backend="kernels")
    with pytest.raises(PafcError, match="pre_beam_size = 32"):
        joint_decoding(model, enc, lens, ctc, beam_size=16, pre_beam_ratio=2.0, backend="kernels")
    with pytest.raises(PafcError, match="not on the GPU"):
        joint_decoding(model, enc, lens, ctc, backend="kernels")


def test_mha_step_paths_validates_before_it_launches():
    """pafc_mha_step_paths answers bad arguments with a PAFC_ERR_* before anything is launched: callable on a machine without
    a GPU (the library builds here with hipcc; skipped where neither hipcc nor a built library exists)."""
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    fn = L.pafc_mha_step_paths
    fn.restype, fn.argtypes = _lib.SIGNATURES["pafc_mha_step_paths"]                        # (a private handle)
    one, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)      # non-null, 16-byte aligned, never dereferenced

    def step(dtype=0, R=8, H=2, dk=64, rows=40, W=5, qkv=one, ldqkv=384, cache=one, path=one, ldpath=5, length=one, new_row=one,
             need=one, out=one, ldo=128):
        return fn(dtype, R, H, dk, rows, W, qkv, ldqkv, cache, path, ldpath, length, new_row, need, out, ldo, NULL)

    assert step(qkv=NULL) == -1 and step(cache=NULL) == -1 and step(path=NULL) == -1 and step(length=NULL) == -1
    assert step(new_row=NULL) == -1 and step(need=NULL) == -1 and step(out=NULL) == -1
    assert step(dtype=2) == -6
    assert step(R=0) == -2 and step(H=0) == -2 and step(rows=0) == -2 and step(W=0) == -2 and step(ldpath=4) == -2
    assert step(dk=32) == -7
    assert step(ldqkv=256) == -2 and step(ldo=64) == -2 and step(ldqkv=386) == -2 and step(dtype=1, ldo=132) == -2
    assert step(qkv=ctypes.c_void_p(8)) == -8 and step(cache=ctypes.c_void_p(24)) == -8


def test_joint_search_kernels_validate_before_they_launch():
    """pafc_joint_candidates / pafc_joint_frame / pafc_joint_collect answer bad arguments, and a pafc_joint_state that does not
    hold together, with a PAFC_ERR_* before anything is launched or any device pointer is followed: callable without a GPU.
    The state is hip_ops' own ctypes struct over dummy pointers, so no call here may be a valid one: every one names its fault."""
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    for name in ("pafc_joint_candidates", "pafc_joint_frame", "pafc_joint_collect"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]         # (a private handle)
    one, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)      # non-null, never dereferenced

    def cands(dtype=0, B=2, T=5, V=53, C=6, blank=0, ctc=one, lens=one, tok=one, p=one, pb=one, skip=one):
        return L.pafc_joint_candidates(dtype, B, T, V, C, blank, 0.0, ctc, lens, tok, p, pb, skip, NULL)

    assert cands(ctc=NULL) == -1 and cands(lens=NULL) == -1 and cands(tok=NULL) == -1 and cands(p=NULL) == -1
    assert cands(pb=NULL) == -1 and cands(skip=NULL) == -1 and cands(dtype=2) == -6
    assert cands(B=0) == -2 and cands(T=0) == -2 and cands(V=0) == -2 and cands(C=0) == -2 and cands(B=65536) == -2
    assert cands(blank=-1) == -2 and cands(blank=53) == -2
    assert cands(C=25) == -7 and cands(V=5, C=6) == -7                                       # 24 candidates at most, C <= V

    pointers = [n for n, kind in hip_ops._JointStateStruct._fields_ if kind is ctypes.c_void_p]
    assert len(pointers) == 38

    def state(B=2, N=4, C=6, T=5, M=None, HS=None, **null):
        M = 1 + T * N * C if M is None else M
        HS = 1 << (2 * M - 1).bit_length() if HS is None else HS
        return hip_ops._JointStateStruct(B, N, C, T, M, HS, **{n: 0 if n in null else 16 for n in pointers})

    weights = (ctypes.c_double * 3)(0.5, 0.5, 0.5)

    def frame(st=None, t=0, dtype=0, V=53, logits=one, ldl=53, lens=one, w=weights, blank=0):
        return L.pafc_joint_frame(ctypes.byref(st if st is not None else state()), t, dtype, V, logits, ldl, lens, w, blank, NULL)

    def collect(st=None, out_len=one, out_att=one):
        return L.pafc_joint_collect(ctypes.byref(st if st is not None else state()), out_len, one, one, one, one, out_att, NULL)

    # a state that does not hold together, through both entry points that take one
    for call in (frame, collect):
        assert call(state(B=0)) == -2 and call(state(N=0)) == -2 and call(state(C=0)) == -2 and call(state(T=0)) == -2
        assert call(state(N=17, M=4000)) == -7 and call(state(C=25, M=4000)) == -7             # beams to 16, candidates to 24
        assert call(state(M=120)) == -2                                                       # M >= 1 + T N C = 121
        assert call(state(HS=255)) == -2 and call(state(HS=128)) == -2                        # a power of two, at least 2 M
        assert call(state(HS=256, parent=True)) == -1                                         # 256 passes, up to the NULL field
        assert call(state(B=1 << 20, N=16, T=1 << 10, C=1, M=1 + (1 << 14))) == -2            # (T + 2) R beyond an int32
        for name in pointers:
            assert call(state(**{name: True})) == -1, name
    assert L.pafc_joint_frame(NULL, 0, 0, 53, one, 53, one, weights, 0, NULL) == -1
    assert L.pafc_joint_collect(NULL, one, one, one, one, one, one, NULL) == -1
    assert frame(lens=NULL) == -1 and frame(w=NULL) == -1 and frame(dtype=3) == -6
    assert frame(t=-1) == -2 and frame(t=5) == -2 and frame(V=0) == -2 and frame(blank=53) == -2 and frame(blank=-1) == -2
    assert frame(V=5, ldl=5) == -2                                                            # C = 6 candidates of 5 tokens
    assert frame(logits=NULL) == -1 and frame(ldl=52) == -2                                   # dec_w > 0 needs the logits
    assert collect(out_len=NULL) == -1 and collect(out_att=NULL) == -1
