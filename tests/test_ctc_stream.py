"""Streaming CTC greedy and prefix beam search on the CPU (transformer/search.CtcStreamer over the resumable host loop)
against the reference's golden and the offline functions, for several cuts of the frames into chunks; partial results and
the committed prefix; reset and max_total_frames; and, cross-compiled here without a GPU, the argument checks, workspace
sizes and register use of the new entry points (include/pafc_search.h: pafc_ctc_beam_stream_*, pafc_ctc_greedy_stream)."""
import ctypes
import os
import random
import re
import subprocess

import pytest
import torch

from tests.conftest import load_golden
from tests.test_ctc_context import Graph, make_graph, same_results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc")
CONFIGS = [(beam, cs) for beam in (4, 8) for cs in (None, 6.0, 2.5)]


@pytest.fixture(scope="module")
def gold():
    return load_golden("ctc_context")


def cuts_of(T, how, B, seed=0):
    """[(chunk width, per-row (start, count))]: every row's frames [0, T) in order; `ragged` gives rows different counts
    per feed and lets some sit a feed out."""
    if how != "ragged":
        return [(min(how, T - a), [(a, min(how, T - a))] * B) for a in range(0, T, how)]
    rng = random.Random(seed)
    pos, out = [0] * B, []
    while min(pos) < T:
        width = rng.choice([1, 3, 7, 16])
        rows = []
        for b in range(B):
            n = 0 if rng.random() < 0.25 else rng.randint(1, width)
            n = min(n, T - pos[b])
            rows.append((pos[b], n))
            pos[b] += n
        out.append((width, rows))
    return out


def stream(streamer, logp, lens, cuts, after_feed=None):
    """Feed logp (B, T, V) to the streamer by `cuts`, row b only up to lens[b]."""
    B, V = logp.shape[0], logp.shape[2]
    fed = [0] * B
    for width, rows in cuts:
        chunk = torch.zeros(B, width, V, dtype=logp.dtype, device=logp.device)
        nf = []
        for b, (a, n) in enumerate(rows):
            n = max(0, min(a + n, int(lens[b])) - a)
            chunk[b, :n] = logp[b, a:a + n]
            nf.append(n)
            fed[b] += n
        partial = streamer.feed(chunk, nf)
        if after_feed is not None:
            after_feed(partial, list(fed))
    return streamer.results()


def exactly_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g.tokens) == tuple(w.tokens) and [tuple(x) for x in g.nbest] == [tuple(x) for x in w.nbest]
        assert g.score == w.score and g.nbest_scores == w.nbest_scores              # float equality: the same bits
        assert g.times == w.times and g.nbest_times == w.nbest_times


def test_inputs_have_no_ties_in_a_frames_top16(gold):
    """topk of a chunk and topk of the whole sequence are certain to agree in order only without equal values."""
    top = gold["logp"].float().topk(16, dim=-1).values
    assert int((top[..., 1:] == top[..., :-1]).sum()) == 0


@pytest.mark.parametrize("how", [1, 7, 16, 80, "ragged"])
@pytest.mark.parametrize("beam,cs", CONFIGS)
def test_streamed_golden_equals_reference_and_offline(gold, beam, cs, how):
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_prefix_beam_search
    graph = None if cs is None else make_graph("bpe", cs)
    logp, lens = gold["logp"], gold["lens"]
    B, T = logp.shape[:2]
    cuts = cuts_of(T, how, B, seed=beam)
    if how == "ragged":
        assert any(len({n for _, n in rows}) > 1 for _, rows in cuts) and any(n == 0 for _, rows in cuts for _, n in rows)
    s = CtcStreamer(B, 80 if how == "ragged" else how, "ctc_prefix_beam_search", beam, graph, 0, max_total_frames=80)
    got = stream(s, logp, lens.tolist(), cuts)
    same_results(got, gold["beam"][(beam, cs)])
    exactly_equal(got, ctc_prefix_beam_search(logp, lens, beam, graph, 0))


def lcp(lists):
    n = min(len(x) for x in lists)
    for i in range(n):
        if len({x[i] for x in lists}) > 1:
            return i
    return n


@pytest.mark.parametrize("beam,cs", CONFIGS)
def test_partials_equal_the_offline_search_of_the_frames_so_far(gold, beam, cs):
    """After every one-frame feed the partial is the offline search of the frames so far (the finalize value included),
    and the committed tokens never shrink, are a prefix of the final 1-best, and grow along the way."""
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_prefix_beam_search
    graph = None if cs is None else make_graph("bpe", cs)
    logp, lens = gold["logp"], gold["lens"]
    B, T = logp.shape[:2]
    s = CtcStreamer(B, 1, "ctc_prefix_beam_search", beam, graph, 0, max_total_frames=80)
    history = []

    def check(partial, fed):
        want = ctc_prefix_beam_search(logp[:, :max(fed)], torch.tensor(fed), beam, graph, 0)
        for p, w in zip(partial, want):
            assert tuple(p.tokens) == tuple(w.tokens) and [tuple(x) for x in p.nbest] == [tuple(x) for x in w.nbest]
            assert p.score == w.score and p.nbest_scores == w.nbest_scores
        for b, w in enumerate(want):                          # committed is the common prefix of the offline n-best
            assert s.committed[b] == list(w.nbest[0][:lcp(w.nbest)])
        history.append([list(c) for c in s.committed])

    final = stream(s, logp, lens.tolist(), cuts_of(T, 1, B), check)
    grows = 0
    for b in range(B):
        prev = []
        for h in history:
            assert h[b][:len(prev)] == prev                   # never shrinks, never changes
            grows += len(h[b]) > len(prev)
            prev = h[b]
        assert list(final[b].tokens)[:len(prev)] == prev      # a prefix of the final 1-best
    assert grows >= 11, grows


def greedy_case():
    """(3, 40, 12) log-probs whose argmax path is written out: with chunks of 8, a token run (frames 6-9), a blank run
    (14-17), a repeat split exactly at a boundary (23 | 24) and token-blank-token around one (31, 32 blank, 33)."""
    B, T, V = 3, 40, 12
    path = torch.zeros(B, T, dtype=torch.long)
    path[0, 2] = 3
    path[0, 6:10] = 5
    path[0, 12:14] = 4
    path[0, 18] = 4
    path[0, 23:25] = 7
    path[0, 31] = 9
    path[0, 33] = 9
    path[0, 39] = 2
    path[1] = torch.tensor([(t // 3) % V for t in range(T)])
    path[2, 7:9] = 6
    path[2, 15:17] = 6
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, T, V, generator=g)
    logits.scatter_add_(2, path[..., None], torch.full((B, T, 1), 9.0))
    assert torch.equal(logits.argmax(-1), path)
    return logits.log_softmax(-1), torch.tensor([40, 37, 16]), path


def greedy_frames(path, lens, blank=0):
    out = []
    for b in range(path.shape[0]):
        fr, prev = [], -1
        for t in range(int(lens[b])):
            u = int(path[b, t])
            if u != blank and u != prev:
                fr.append(t)
            prev = u
        out.append(fr)
    return out


@pytest.mark.parametrize("how", [1, 8, 40, "ragged"])
def test_greedy_stream_equals_offline(how):
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_greedy_search
    logp, lens, path = greedy_case()
    want = ctc_greedy_search(logp, lens, 0)
    assert want[0].tokens == [3, 5, 4, 4, 7, 9, 9, 2]
    s = CtcStreamer(3, 40 if how == "ragged" else how, "ctc_greedy_search")
    got = stream(s, logp, lens.tolist(), cuts_of(40, how, 3, seed=1))
    assert [r.tokens for r in got] == [r.tokens for r in want]
    assert [r.times for r in got] == greedy_frames(path, lens)
    assert s.committed == [r.tokens for r in got]


def test_reset_restarts_only_the_given_rows(gold):
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_prefix_beam_search
    logp, graph = gold["logp"][:3], make_graph("bpe", 6.0)
    s = CtcStreamer(3, 16, "ctc_prefix_beam_search", 4, graph, 0, max_total_frames=80)
    s.feed(logp[:, :16])
    s.feed(logp[:, 16:32])
    s.reset([1])
    assert s.committed[1] == []
    for a in range(32, 80, 16):
        s.feed(logp[:, a:a + 16])
    got = s.results()
    whole = ctc_prefix_beam_search(logp, torch.tensor([80, 80, 80]), 4, graph, 0)
    late = ctc_prefix_beam_search(logp[1:2, 32:], torch.tensor([48]), 4, graph, 0)
    exactly_equal([got[0], got[2]], [whole[0], whole[2]])
    exactly_equal([got[1]], late)                             # frames since the reset, times counted from it


@pytest.mark.parametrize("mode", ["ctc_prefix_beam_search", "ctc_greedy_search"])
def test_streamer_refuses_bad_arguments(mode):
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer
    with pytest.raises(ValueError, match="mode"):
        CtcStreamer(2, 8, "attention")
    with pytest.raises(ValueError):
        CtcStreamer(2, 0, mode)
    s = CtcStreamer(2, 8, mode, 4)
    with pytest.raises(ValueError, match="chunk"):
        s.feed(torch.zeros(2, 9, 10))
    with pytest.raises(ValueError, match="chunk"):
        s.feed(torch.zeros(3, 8, 10))


def test_max_total_frames_names_the_row_and_spares_the_others(gold):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_prefix_beam_search
    logp = gold["logp"][:3]
    s = CtcStreamer(3, 16, "ctc_prefix_beam_search", 4, None, 0, max_total_frames=40)
    s.feed(logp[:, :16], [16, 16, 16])
    s.feed(logp[:, 16:32], [16, 8, 16])
    with pytest.raises(PafcError, match=r"rows \[0, 2\].*max_total_frames = 40"):
        s.feed(logp[:, 32:48], [16, 16, 9])                   # rows 0 and 2 would reach 48 and 41; row 1 reaches 40
    with pytest.raises(PafcError, match=r"rows \[2\]"):
        s.feed(logp[:, 32:48], [0, 0, 1])                     # a refused row takes nothing until its reset
    got = s.results()
    want = ctc_prefix_beam_search(logp, torch.tensor([32, 40, 32]), 4, None, 0)
    row1 = ctc_prefix_beam_search(torch.cat([logp[1:2, :24], logp[1:2, 32:48]], 1), torch.tensor([40]), 4, None, 0)
    exactly_equal([got[0], got[2]], [want[0], want[2]])
    exactly_equal([got[1]], row1)
    s.reset([0])
    s.feed(logp[:, 32:48], [16, 0, 0])
    exactly_equal([s.results()[0]], ctc_prefix_beam_search(logp[0:1, 32:48], torch.tensor([16]), 4, None, 0))


def test_model_method_exists_on_both_families():
    import inspect
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    want = ["speech", "decoding_chunk_size", "mode", "beam_size", "context_graph", "blank_id", "blank_penalty", "on_partial"]
    for cls in (ASRModel, Transducer):
        assert list(inspect.signature(cls.stream_ctc_search).parameters)[1:1 + len(want)] == want
    assert Transducer.stream_ctc_search is ASRModel.stream_ctc_search


def test_device_classes_refuse_the_cpu():
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd._lib import PafcError
    with pytest.raises(PafcError, match="no CPU fallback"):
        hip_ops.CtcBeamStream(2, 8, 4, 4, "cpu")
    with pytest.raises(PafcError, match="no CPU fallback"):
        hip_ops.CtcGreedyStream(2, 8, "cpu")


# ---- the C entry points, cross-compiled here -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    lib = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    G = ctypes.POINTER(Graph)
    lib.pafc_ctc_beam_stream_workspace_bytes.restype = Z
    lib.pafc_ctc_beam_stream_workspace_bytes.argtypes = [I, I, I, I]
    lib.pafc_ctc_beam_stream_reset.argtypes = [I, I, I, I, P, P, Z, P]
    lib.pafc_ctc_beam_stream_feed.argtypes = [I, I, I, P, P, P, I, I, I, G, I, P, Z, P]
    lib.pafc_ctc_beam_stream_drain.argtypes = [I, I, I, G, I, P, Z, P, I, P, P, P, P, P, P, I, P, P, P]
    lib.pafc_ctc_greedy_stream_workspace_bytes.restype = Z
    lib.pafc_ctc_greedy_stream_workspace_bytes.argtypes = [I]
    lib.pafc_ctc_greedy_stream_reset.argtypes = [I, P, P, Z, P]
    lib.pafc_ctc_greedy_stream.argtypes = [I, I, I, I, P, P, I, P, Z, P, P, P, P, P]
    return lib


ERR_NULL, ERR_DIMS, ERR_WS, ERR_DTYPE, ERR_UNSUP = -1, -2, -4, -6, -7


def test_workspace_size_is_monotone_and_documented(L):
    ws = L.pafc_ctc_beam_stream_workspace_bytes
    base = ws(8, 4000, 8, 1)
    assert base > 0
    assert ws(9, 4000, 8, 1) > base and ws(8, 4001, 8, 1) > base and ws(8, 4000, 9, 1) > base and base > ws(8, 4000, 8, 0)
    for bad in ((0, 10, 4, 1), (2, 0, 4, 1), (2, 10, 0, 1), (2, 10, 17, 1), (1, 1 << 30, 16, 1)):
        assert ws(*bad) == 0, bad
    # the header's memory per stream: 16 bytes per node with times, 8 without, 1 + max_total_frames * beam nodes
    assert ws(2, 4000, 8, 1) - ws(1, 4000, 8, 1) == pytest.approx(16 * (1 + 4000 * 8), abs=1536)
    assert ws(2, 4000, 8, 0) - ws(1, 4000, 8, 0) == pytest.approx(8 * (1 + 4000 * 8), abs=1536)
    assert L.pafc_ctc_greedy_stream_workspace_bytes(5) == 80 and L.pafc_ctc_greedy_stream_workspace_bytes(0) == 0


def test_stream_entry_points_validate_arguments(L):
    P = ctypes.c_void_p
    NULL, one = P(0), P(256)
    ws = L.pafc_ctc_beam_stream_workspace_bytes(2, 100, 4, 1)
    g = Graph(3, *[256] * 7)
    gp = ctypes.byref(g)
    reset, feed, drain = L.pafc_ctc_beam_stream_reset, L.pafc_ctc_beam_stream_feed, L.pafc_ctc_beam_stream_drain
    assert reset(2, 100, 4, 1, NULL, NULL, ws, NULL) == ERR_NULL
    assert reset(0, 100, 4, 1, NULL, one, ws, NULL) == ERR_DIMS
    assert reset(2, 100, 17, 1, NULL, one, 1 << 30, NULL) == ERR_UNSUP
    assert reset(2, 100, 4, 1, NULL, one, ws - 1, NULL) == ERR_WS
    assert reset(2, 100, 4, 1, NULL, one, L.pafc_ctc_beam_stream_workspace_bytes(2, 100, 4, 0), NULL) == ERR_WS   # no frame lists

    ok = dict(B=2, Tmax=16, K=4, p=one, i=one, nf=one, total=100, beam=4, blank=0, g=gp, times=1, ws=one, nws=ws)

    def f(**kw):
        a = dict(ok, **kw)
        return feed(a["B"], a["Tmax"], a["K"], a["p"], a["i"], a["nf"], a["total"], a["beam"], a["blank"], a["g"], a["times"],
                    a["ws"], a["nws"], NULL)
    for k in ("p", "i", "nf", "ws"):
        assert f(**{k: NULL}) == ERR_NULL, k
    for k, v in (("B", 0), ("Tmax", 0), ("K", 0), ("total", 0), ("beam", 0), ("blank", -1)):
        assert f(**{k: v}) == ERR_DIMS, k
    assert f(K=17, nws=1 << 30) == ERR_UNSUP and f(beam=17, nws=1 << 30) == ERR_UNSUP
    assert f(nws=ws - 1) == ERR_WS
    for i in range(1, 8):                                     # every table pointer of the graph
        bad = Graph(3, *[0 if j == i else 256 for j in range(1, 8)])
        assert f(g=ctypes.byref(bad)) == ERR_NULL, i
    assert f(g=ctypes.byref(Graph(0, *[256] * 7))) == ERR_DIMS

    def d(B=2, total=100, beam=4, g=gp, times=1, w=one, nws=ws, frm=one, ld=8, tok=one, ln=one, sc=one, cnt=one, com=one,
          ovf=one, ldt=0, tim=NULL, nt=NULL):
        return drain(B, total, beam, g, times, w, nws, frm, ld, tok, ln, sc, cnt, com, ovf, ldt, tim, nt, NULL)
    for k in ("w", "tok", "ln", "sc", "cnt", "com", "ovf"):
        assert d(**{k: NULL}) == ERR_NULL, k
    assert d(ldt=4, tim=NULL, nt=one) == ERR_NULL and d(ldt=4, tim=one, nt=NULL) == ERR_NULL
    assert d(B=0) == ERR_DIMS and d(ld=-1) == ERR_DIMS and d(ldt=-1) == ERR_DIMS
    assert d(beam=17, nws=1 << 30) == ERR_UNSUP
    assert d(times=0, nt=one, tim=one, ldt=4) == ERR_UNSUP   # frame lists asked of a workspace without them
    assert d(nws=ws - 1) == ERR_WS
    assert d(g=ctypes.byref(Graph(3, 256, 256, 256, 256, 256, 0, 256))) == ERR_NULL

    gs = L.pafc_ctc_greedy_stream
    gws = L.pafc_ctc_greedy_stream_workspace_bytes(2)
    assert gs(0, 2, 8, 10, NULL, one, 0, one, gws, one, one, one, NULL, NULL) == ERR_NULL
    assert gs(0, 2, 8, 10, one, NULL, 0, one, gws, one, one, one, NULL, NULL) == ERR_NULL
    assert gs(0, 2, 8, 10, one, one, 0, NULL, gws, one, one, one, NULL, NULL) == ERR_NULL
    assert gs(0, 2, 0, 10, one, one, 0, one, gws, one, one, one, NULL, NULL) == ERR_DIMS
    assert gs(0, 2, 8, 10, one, one, 10, one, gws, one, one, one, NULL, NULL) == ERR_DIMS     # blank >= V
    assert gs(5, 2, 8, 10, one, one, 0, one, gws, one, one, one, NULL, NULL) == ERR_DTYPE
    assert gs(0, 2, 8, 10, one, one, 0, one, gws - 1, one, one, one, NULL, NULL) == ERR_WS
    assert L.pafc_ctc_greedy_stream_reset(2, NULL, NULL, gws, NULL) == ERR_NULL
    assert L.pafc_ctc_greedy_stream_reset(0, NULL, one, gws, NULL) == ERR_DIMS
    assert L.pafc_ctc_greedy_stream_reset(2, NULL, one, gws - 1, NULL) == ERR_WS


def _asm(tmp_path, name):
    src = os.path.join(CSRC, name + ".hip")
    out = tmp_path / (name + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I",
                           os.path.join(ROOT, "include"), "-I", CSRC, "-S", "--cuda-device-only", src, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


@pytest.mark.parametrize("name,kernel,count", [("ctc_beam_stream", "ctc_beam_stream_feed_kernel", 4),
                                               ("ctc_beam_stream", "ctc_beam_stream_drain_kernel", 1),
                                               ("ctc_greedy", "ctc_collapse_stream_kernel", 1)])
def test_stream_kernels_do_not_spill(tmp_path, name, kernel, count):
    asm = _asm(tmp_path, name)
    names = set(re.findall(r"^(_ZN4pafc[^\s:]*" + kernel + r"[^\s:]*):", asm, flags=re.M))
    assert len(names) == count, names                           # the feed kernel: <CTX, TIMES> in all four combinations
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)
    assert spills and all(int(v) == 0 for v in spills)
    priv = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm)
    assert priv and all(int(v) == 0 for v in priv)
    assert "scratch_" not in asm


def test_offline_and_streaming_kernels_share_one_frame_body():
    """The per-frame arithmetic exists once, in ctc_beam_frame.inc, and both kernels include it: the two cannot drift."""
    inc = '#include "ctc_beam_frame.inc"'
    for name in ("ctc_beam.hip", "ctc_beam_stream.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert src.count(inc) == 1, name
        assert "log_add2(" not in src and "s_order[" not in src, f"{name} holds frame arithmetic of its own"
    body = open(os.path.join(CSRC, "ctc_beam_frame.inc")).read()
    assert "log_add2(" in body and "s_order[" in body
