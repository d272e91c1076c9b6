"""Streaming CTC-fused RNN-T prefix beam search on the host (BeamStreamer's host path): after any cut of the golden's
frames into chunks the n-best lists and scores are those of prefix_beam_search_decode on the same tensors, the committed
prefix is final and only grows, a row reset mid-stream decodes a second utterance as if fresh, and the new kernel entry
points are declared in the header and in the signature table.  No GPU."""
import os
import re

import pytest
import torch

from tests.conftest import load_golden
from tests.test_search import _build, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(beam_size=8, ctc_weight=0.3, transducer_weight=0.7)
CUTS = ["one", "sixteen", "irregular", "whole"]


def cuts(T, how):
    """Global cuts [a, b) of T frames."""
    if how == "irregular":
        sizes, out, a, i = [3, 1, 9, 2, 16, 5, 11, 4], [], 0, 0
        while a < T:
            out.append((a, min(T, a + sizes[i % len(sizes)])))
            a, i = out[-1][1], i + 1
        return out
    step = {"one": 1, "sixteen": 16, "whole": T}[how]
    return [(a, min(T, a + step)) for a in range(0, T, step)]


@pytest.fixture(scope="module")
def world():
    g = load_golden("search_c5")
    ctc, pred, joint, bs = _build(g)
    with torch.no_grad():
        logp = ctc.log_softmax(g["enc_out"])
        offline = bs.prefix_beam_search_decode(g["enc_out"], g["enc_lens"], logp, **KW)
    return g, bs, logp, offline


def _streamer(bs, B=3, max_frames=37, **kw):
    from paper_accurate_fast_cheap_amd.transducer.search.prefix_beam_search import BeamStreamer
    return BeamStreamer(bs, B, max_frames, 8, 0.3, 0.7, **kw)


def _is_prefix(p, full):
    return list(full[:len(p)]) == list(p)


@pytest.mark.parametrize("how", CUTS)
def test_host_streamer_equals_offline_decode_for_any_cut(world, how):
    g, bs, logp, offline = world
    enc, lens = g["enc_out"], g["enc_lens"].tolist()
    st = _streamer(bs)
    history = []
    for a, b in cuts(enc.shape[1], how):
        nf = [max(0, min(L - a, b - a)) for L in lens]
        part = st.feed(enc[:, a:b], logp[:, a:b], nf)
        assert len(part) == 3
        for r in range(3):                                  # committed = the common prefix of the row's live hypotheses
            common = min(len(n) for n in part[r].nbest)
            while any(list(n[:common]) != list(part[r].nbest[0][:common]) for n in part[r].nbest):
                common -= 1
            assert st.committed[r] == list(part[r].nbest[0][:common])
        history.append([list(c) for c in st.committed])
    res = st.results()
    for r, o in zip(res, offline):
        assert [list(n) for n in r.nbest] == [list(n) for n in o.nbest]
        assert r.nbest_scores == o.nbest_scores and r.score == o.score          # the same arithmetic: bit for bit
        assert list(r.tokens) == list(o.tokens)
    _same(res, g["rnnt"], 1e-4)
    # the committed prefix is final at every feed and never shrinks
    for b in range(3):
        prev = []
        for h in history:
            assert _is_prefix(h[b], res[b].tokens), (b, h[b])
            assert _is_prefix(prev, h[b])
            prev = h[b]
    assert [list(p.tokens) for p in st.partials()] == [list(r.tokens) for r in res]


def test_reset_restarts_one_row_and_leaves_the_others(world):
    """Row 2 (11 frames) ends inside the first chunk, is reset and then decodes utterance 1's frames as a fresh stream while
    rows 0 and 1 go on.  Tokens are exact; the scores are compared with test_search._same's 1e-4, the bound between the
    reference's float32 GEMMs and ours: a frame's GEMMs here see another set of live beams than the offline batch."""
    g, bs, logp, offline = world
    enc, lens = g["enc_out"], g["enc_lens"].tolist()
    st = _streamer(bs, max_frames=16)
    st.feed(enc[:, :16], logp[:, :16], [16, 16, 11])
    first = st.results()
    assert list(first[2].tokens) == list(offline[2].tokens) and [list(n) for n in first[2].nbest] == [list(n) for n in offline[2].nbest]
    assert first[2].nbest_scores == offline[2].nbest_scores                     # the same live beams as offline so far
    st.reset([2])
    assert st.committed[2] == [] and st.committed[0] == first[0].nbest[0][:len(st.committed[0])]
    pos2 = 0
    for a in (16, 32):
        b = min(a + 16, 37)
        e, c = enc[:, a:b].clone(), logp[:, a:b].clone()
        n2 = min(b - a, lens[1] - pos2)
        e[2, :n2], c[2, :n2] = enc[1, pos2:pos2 + n2], logp[1, pos2:pos2 + n2]
        st.feed(e, c, [max(0, min(lens[0] - a, b - a)), max(0, min(lens[1] - a, b - a)), n2])
        pos2 += n2
    e, c = torch.zeros(3, 16, enc.shape[2]), torch.zeros(3, 16, logp.shape[2])
    n2 = lens[1] - pos2
    e[2, :n2], c[2, :n2] = enc[1, pos2:pos2 + n2], logp[1, pos2:pos2 + n2]
    st.feed(e, c, [0, 0, n2])
    res = st.results()
    for got, want in ((res[0], offline[0]), (res[1], offline[1]), (res[2], offline[1])):
        assert [list(n) for n in got.nbest] == [list(n) for n in want.nbest]
        assert got.nbest_scores == pytest.approx(want.nbest_scores, abs=1e-4)


def test_overflow_refuses_the_row_and_serves_the_others(world):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    g, bs, logp, _ = world
    enc = g["enc_out"]
    st = _streamer(bs, max_frames=8, max_total_frames=10)
    st.feed(enc[:, :8], logp[:, :8], [8, 8, 2])
    with pytest.raises(PafcError, match=r"rows \[0, 1\]"):
        st.feed(enc[:, 8:16], logp[:, 8:16], [8, 8, 8])
    assert st._frames == [8, 8, 10]
    with pytest.raises(PafcError, match=r"rows \[0\]"):                          # the flag holds until the reset
        st.feed(enc[:, 8:9], logp[:, 8:9], [1, 0, 0])
    st.reset([0])
    st.feed(enc[:, :1], logp[:, :1], [1, 0, 0])
    assert st._frames == [1, 8, 10]


def test_stream_symbols_are_declared_in_the_header_and_the_table():
    from paper_accurate_fast_cheap_amd import _lib
    header = open(os.path.join(ROOT, "include", "pafc_search.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = ["pafc_rnnt_beam_stream_workspace_bytes", "pafc_rnnt_beam_stream_reset", "pafc_rnnt_beam_stream_feed",
             "pafc_rnnt_beam_stream_step", "pafc_rnnt_beam_stream_drain", "pafc_rnnt_beam_select_state"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["pafc_rnnt_beam_stream_workspace_bytes"][0] is _lib.Z
    src = os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc")
    assert os.path.exists(os.path.join(src, "rnnt_beam_stream.hip"))
    # one text for the candidate walk: both step kernels include it
    for f in ("rnnt_beam.hip", "rnnt_beam_stream.hip"):
        assert '#include "rnnt_beam_frame.inc"' in open(os.path.join(src, f)).read(), f


def test_stream_entry_points_validate_arguments_without_a_gpu():
    import ctypes
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists(build.OUT) and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib._bind(ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT))
    P = ctypes.c_void_p
    NULL, one = P(0), P(256)        # `one`: a non-null address that is never dereferenced (validation fails first)
    nws = L.pafc_rnnt_beam_stream_workspace_bytes(3, 40, 8)
    assert nws >= L.pafc_rnnt_beam_workspace_bytes(3, 40, 8) + 4 * 3 * 4
    assert L.pafc_rnnt_beam_stream_workspace_bytes(3, 40, 17) == 0
    assert L.pafc_rnnt_beam_stream_workspace_bytes(1, 1 << 28, 8) == 0           # max_total_frames * beam >= 2^31 - 1
    assert L.pafc_rnnt_beam_stream_reset(3, 40, 17, 0, NULL, one, 1 << 30, one, one, NULL) == -7
    assert L.pafc_rnnt_beam_stream_reset(3, 40, 8, 0, NULL, one, nws - 1, one, one, NULL) == -4
    assert L.pafc_rnnt_beam_stream_reset(3, 40, 8, 0, NULL, NULL, nws, one, one, NULL) == -1
    assert L.pafc_rnnt_beam_stream_reset(3, 40, 8, 0, NULL, one, nws, NULL, one, NULL) == -1
    assert L.pafc_rnnt_beam_stream_feed(3, 16, 40, 8, NULL, one, nws, NULL) == -1
    assert L.pafc_rnnt_beam_stream_feed(3, 0, 40, 8, one, one, nws, NULL) == -2
    assert L.pafc_rnnt_beam_stream_step(3, 16, 40, 8, 0, 0, NULL, NULL, one, one, nws, one, one, NULL) == -1
    assert L.pafc_rnnt_beam_stream_step(3, 16, 40, 8, 0, 16, NULL, one, one, one, nws, one, one, NULL) == -2
    assert L.pafc_rnnt_beam_stream_step(3, 16, 40, 8, 0, 0, NULL, one, one, one, 8, one, one, NULL) == -4
    assert L.pafc_rnnt_beam_stream_drain(3, 40, 8, one, nws, NULL, 4, NULL, one, one, one, one, one, NULL) == -1
    assert L.pafc_rnnt_beam_stream_drain(3, 40, 17, one, nws, NULL, 4, one, one, one, one, one, one, NULL) == -7
    assert L.pafc_rnnt_beam_select_state(0, 2, 3, 8, 64, NULL, one, one, one, one, NULL) == -1
    assert L.pafc_rnnt_beam_select_state(5, 2, 3, 8, 64, one, one, one, one, one, NULL) == -6
    assert L.pafc_rnnt_beam_select_state(0, 2, 3, 17, 64, one, one, one, one, one, NULL) == -7
    assert L.pafc_rnnt_beam_select_state(0, 0, 3, 8, 64, one, one, one, one, one, NULL) == -2


def test_the_frame_engine_dies_with_its_owner_not_in_a_later_collection():
    """_ResidentFrames holds a hipGraph.  Were it part of a reference cycle, the graph would be destroyed by whichever garbage
    collection comes next -- possibly inside another stream capture, which the runtime answers with an abort.  So with the
    collector off, dropping the last reference must free the engine and what it holds."""
    import gc
    import weakref
    from paper_accurate_fast_cheap_amd.transducer.search.prefix_beam_search import _ResidentFrames

    class Slots:
        B, beam = 1, 1

    for body in (None, object()):
        was = gc.isenabled()
        gc.disable()
        try:
            slots = Slots()
            eng = _ResidentFrames(None, slots, lambda tv, ti, t: slots, torch.zeros(1, 2, 4), torch.zeros(1, 2, 3),
                                  [torch.zeros(1, 1, 2), torch.zeros(1, 1, 2)], 0.7, 0.3, body=body)
            eng.frame                                                    # looking the frame up must not store it
            seen = weakref.ref(eng), weakref.ref(slots), weakref.ref(eng.t_dev)
            del eng, slots
            assert [r() for r in seen] == [None, None, None]
        finally:
            if was:
                gc.enable()
