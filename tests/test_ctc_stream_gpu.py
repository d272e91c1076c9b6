"""Streaming CTC search on the MI355X (hip_ops.CtcBeamStream / CtcGreedyStream, csrc/ctc_beam_stream.hip,
pafc_ctc_greedy_stream): the streamed search against the offline kernel on the concatenated frames bit for bit, in all
four <context graph, times> variants; against the host loop at the bound test_ctc_context_gpu.py uses for the offline
kernel; partial results; reset and overflow with a guard region behind the pools; a feed replayed from a captured graph;
and ASRModel / Transducer.stream_ctc_search on reduced streaming encoders."""
import pytest
import torch

from tests.conftest import load_golden
from tests.test_ctc_context import make_graph, same_results
from tests.test_ctc_context_gpu import planted_logp, synthetic_graph
from tests.test_ctc_stream import cuts_of, greedy_case, stream

pytestmark = pytest.mark.gpu
B, T, V = 8, 500, 5000


def case(tmp_path, beam):
    graph, phrases = synthetic_graph(tmp_path, 1000, V, seed=beam)
    logp = planted_logp(B, T, V, phrases, seed=100 + beam)
    lens = torch.randint(T // 3, T + 1, (B,), generator=torch.Generator().manual_seed(beam))
    lens[0] = T
    return graph, logp, lens


def run_stream(st, top_p, top_i, lens, cuts):
    """Feed the top-k lists (B, T, K) of whole utterances to a CtcBeamStream by `cuts`."""
    Bn, _, K = top_p.shape
    for width, rows in cuts:
        cp = torch.zeros(Bn, width, K, device="cuda")
        ci = torch.zeros(Bn, width, K, dtype=top_i.dtype, device="cuda")
        nf = []
        for b, (a, n) in enumerate(rows):
            n = max(0, min(a + n, int(lens[b])) - a)
            cp[b, :n], ci[b, :n] = top_p[b, a:a + n], top_i[b, a:a + n]
            nf.append(n)
        st.feed(cp, ci, nf)


def same_as_offline(d, off, beam, want_times):
    toks, ln, sc, tim = off
    ln_h = ln.tolist()
    assert d["len"] == ln_h
    assert torch.equal(torch.tensor(d["score"], dtype=torch.float64).view(torch.int64), sc.cpu().view(torch.int64))
    toks_h = toks.cpu()
    tim_h = tim.cpu() if want_times else None
    for b in range(len(ln_h)):
        assert d["count"][b] == sum(v >= 0 for v in ln_h[b])
        for n in range(beam):
            k = max(0, ln_h[b][n])
            assert d["tokens"][b][n] == toks_h[b, n, :k].tolist()
            if want_times:
                row = tim_h[b, n]
                assert d["times"][b][n] == row[row >= 0].tolist()


@pytest.mark.parametrize("beam", [4, 8, 16])
@pytest.mark.parametrize("with_graph", [False, True])
def test_stream_equals_offline_kernel_bit_for_bit(hip, tmp_path, beam, with_graph):
    """Chunks of 1, 16, 64 and a ragged cut, with and without frame lists: n-best tokens, lengths, times and the scores'
    bit patterns equal pafc_ctc_prefix_beam_search_ex on the whole sequence.  This is also the test that holds the two
    kernels' frame arithmetic together, in all four <CTX, TIMES> combinations."""
    from paper_accurate_fast_cheap_amd import hip_ops
    graph, logp, lens = case(tmp_path, beam)
    tables = graph.device_tables(torch.device("cuda", torch.cuda.current_device())) if with_graph else None
    top_p, top_i = logp.cuda().topk(beam, dim=-1)
    top_p, top_i = top_p.contiguous(), top_i.contiguous()
    lens_l = lens.tolist()
    for want_times in (True, False):
        off = hip_ops.ctc_prefix_beam(top_p, top_i, lens.cuda(), beam, 0, tables, want_times)
        torch.cuda.synchronize()
        for how in (1, 16, 64, "ragged"):
            st = hip_ops.CtcBeamStream(B, 64 if how == "ragged" else how, beam, beam, "cuda", 0, tables, T, want_times)
            run_stream(st, top_p, top_i, lens_l, cuts_of(T, how, B, seed=beam))
            d = st.drain(None, T, want_times)
            assert d["overflow"] == [0] * B
            same_as_offline(d, off, beam, want_times)
            # the same lists again through the `from` offset: the tail after the committed prefix
            d2 = st.drain(d["committed"], T, False)
            assert d2["committed"] == d["committed"] and d2["score"] == d["score"] and d2["len"] == d["len"]
            for b in range(B):
                assert all(d["tokens"][b][n][:d["committed"][b]] == d["tokens"][b][0][:d["committed"][b]]
                           for n in range(d["count"][b]))
                assert [t[d["committed"][b]:] for t in d["tokens"][b]] == d2["tokens"][b]


@pytest.mark.parametrize("beam", [4, 16])
@pytest.mark.parametrize("extras", [False, True])
def test_drain_from_the_committed_count_returns_the_same_lists(hip, tmp_path, beam, extras):
    """drain(counts, ld) against the matching slices of drain(0, 24) after each of three feeds of 8 frames, for counts = the
    previous `committed` and ld = 1 and the longest tail: tokens, len, count, overflow, the scores' bits and (extras: a context
    graph and frame lists) times.  committed is the common prefix of the live members' full lists.  Row 1 sits the middle
    feed out and row 2 is reset after the first.  A vocabulary of 12 keeps the prefixes few, so they leave the beam and are
    formed again; it also bounds the top-k, hence K = min(beam, 12)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer.search import _common_prefix_len
    Bn, Tmax, Tn, Vn = 3, 8, 24, 12
    K = min(beam, Vn)
    graph, phrases = synthetic_graph(tmp_path, 10, Vn, seed=beam, pool=8)
    top_p, top_i = planted_logp(Bn, Tn, Vn, phrases, seed=200 + beam).cuda().topk(K, dim=-1)
    assert bool((top_p[..., 1:] < top_p[..., :-1]).all())        # no ties in a frame's top-k
    tables = graph.device_tables(torch.device("cuda", torch.cuda.current_device())) if extras else None
    st = hip_ops.CtcBeamStream(Bn, Tmax, K, beam, "cuda", 0, tables, Tn, extras)
    bits = lambda rows: torch.tensor(rows, dtype=torch.float64).view(torch.int64).tolist()

    d = st.drain(None, Tn, extras)                            # before any feed: the empty prefix
    assert d["committed"] == [0] * Bn and d["count"] == [1] * Bn and d["len"] == [[0] + [-1] * (beam - 1)] * Bn
    assert d["tokens"] == [[[]] * beam] * Bn

    counts, grew = [0] * Bn, False
    for f, nf in enumerate(([8, 8, 8], [8, 0, 8], [8, 8, 8])):
        st.feed(top_p[:, 8 * f:8 * f + 8].contiguous(), top_i[:, 8 * f:8 * f + 8].contiguous(), nf)
        full = st.drain(None, Tn, extras)
        assert full["overflow"] == [0] * Bn
        live = [[full["tokens"][b][n] for n in range(full["count"][b])] for b in range(Bn)]
        assert all(len(live[b][n]) == full["len"][b][n] for b in range(Bn) for n in range(len(live[b])))
        assert full["committed"] == [_common_prefix_len(x) for x in live]
        tail = max(1, max(len(x) - counts[b] for b in range(Bn) for x in live[b]))
        for ld in (1, tail):
            part = st.drain(counts, ld, extras)
            for k in ("len", "count", "overflow", "committed"):
                assert part[k] == full[k], (k, ld)
            assert bits(part["score"]) == bits(full["score"])
            for b in range(Bn):
                assert part["tokens"][b] == [x[counts[b]:counts[b] + ld] for x in full["tokens"][b]]
            if extras:
                assert part["times"] == full["times"]
        grew = grew or any(c > 0 for c in full["committed"])
        counts = list(full["committed"])
        if f == 0:
            st.reset([2])
            counts[2] = 0
            d = st.drain(counts, Tn, False)
            assert d["len"][2] == [0] + [-1] * (beam - 1) and d["committed"] == counts and d["len"][:2] == full["len"][:2]
    assert grew                                               # the planted peaks commit a prefix in some row


@pytest.mark.parametrize("beam", [4, 8, 16])
@pytest.mark.parametrize("with_graph", [False, True])
def test_streamer_matches_the_host_loop(hip, tmp_path, beam, with_graph):
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_prefix_beam_search
    graph, logp, lens = case(tmp_path, beam)
    g = graph if with_graph else None
    want = ctc_prefix_beam_search(logp, lens, beam, g, 0)
    s = CtcStreamer(B, 16, "ctc_prefix_beam_search", beam, g, 0, max_total_frames=T)
    committed = []
    got = stream(s, logp.cuda(), lens.tolist(), cuts_of(T, 16, B), lambda p, fed: committed.append([list(c) for c in s.committed]))
    for w, r in zip(want, got):
        assert [tuple(n) for n in r.nbest] == [tuple(n) for n in w.nbest]
        assert r.times == w.times and r.nbest_times == w.nbest_times
        assert r.nbest_scores == pytest.approx(w.nbest_scores, rel=1e-12, abs=1e-9)
    for b in range(B):                                        # committed: grows only, ends as a prefix of the 1-best
        prev = []
        for h in committed:
            assert h[b][:len(prev)] == prev
            prev = h[b]
        assert list(got[b].tokens)[:len(prev)] == prev and len(prev) > 0


@pytest.mark.parametrize("beam", [4, 8])
@pytest.mark.parametrize("cs", [None, 6.0, 2.5])
def test_golden_on_the_device_streamed(hip, beam, cs):
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer
    gold = load_golden("ctc_context")
    graph = None if cs is None else make_graph("bpe", cs)
    logp, lens = gold["logp"].cuda(), gold["lens"].tolist()
    for how in (7, "ragged"):
        s = CtcStreamer(logp.shape[0], 16, "ctc_prefix_beam_search", beam, graph, 0, max_total_frames=80)
        got = stream(s, logp, lens, cuts_of(80, how, logp.shape[0], seed=beam))
        same_results(got, gold["beam"][(beam, cs)], atol=1e-9, rel=1e-12)


def test_partials_equal_the_offline_kernel_on_the_frames_so_far(hip, tmp_path):
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_prefix_beam_search
    graph, logp, lens = case(tmp_path, 8)
    logp = logp.cuda()
    s = CtcStreamer(B, 64, "ctc_prefix_beam_search", 8, graph, 0, max_total_frames=T)
    reads = []

    def check(partial, fed):
        want = ctc_prefix_beam_search(logp[:, :max(fed)], torch.tensor(fed).cuda(), 8, graph, 0)
        for p, w in zip(partial, want):
            assert [tuple(x) for x in p.nbest] == [tuple(x) for x in w.nbest]
            assert p.nbest_scores == w.nbest_scores and p.score == w.score       # the finalize value included
        reads.append(s.last_read_bytes)

    stream(s, logp, lens.tolist(), cuts_of(T, 64, B), check)
    print("bytes read per feed:", reads)


def test_reset_and_overflow_leave_the_guard_untouched(hip, tmp_path):
    """Rows 1 and 7 (the last row: its pools end the workspace) run past max_total_frames: their flag is set, nothing
    beyond the workspace is written, the other rows equal the offline search; a reset row equals the search of the frames
    fed after the reset."""
    from paper_accurate_fast_cheap_amd import hip_ops
    beam, total = 8, 96
    _, logp, _ = case(tmp_path, 8)
    top_p, top_i = logp[:, :160].cuda().topk(beam, dim=-1)
    st = hip_ops.CtcBeamStream(B, 32, beam, beam, "cuda", 0, None, total, True)
    guard = 1 << 16
    big = torch.full((st._nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    st._ws = big                                               # the same size is passed on: the tail is the guard
    st.reset()
    for a in (0, 32, 64):
        st.feed(top_p[:, a:a + 32], top_i[:, a:a + 32])
    st.reset([2])
    st.feed(top_p[:, 96:128], top_i[:, 96:128], [0, 32, 32, 0, 0, 0, 0, 1])     # rows 1 and 7 would pass 96
    d = st.drain(None, total, True)
    torch.cuda.synchronize()
    assert d["overflow"] == [0, 1, 0, 0, 0, 0, 0, 1]
    assert bool((big[st._nbytes:] == 0xA5).all())
    off = hip_ops.ctc_prefix_beam(top_p[:, :96].contiguous(), top_i[:, :96].contiguous(), None, beam, 0, None, True)
    late = hip_ops.ctc_prefix_beam(top_p[2:3, 96:128].contiguous(), top_i[2:3, 96:128].contiguous(), None, beam, 0, None, True)
    for b in range(B):
        o = late if b == 2 else off
        i = 0 if b == 2 else b
        assert d["len"][b] == o[1][i].tolist() and d["score"][b] == o[2][i].tolist()
        for n in range(beam):
            k = max(0, d["len"][b][n])
            assert d["tokens"][b][n] == o[0][i, n, :k].tolist()
            row = o[3][i, n]
            assert d["times"][b][n] == row[row >= 0].tolist()
    # a flagged row takes nothing until it is reset; the host layer names the row
    st.feed(top_p[:, :1].contiguous(), top_i[:, :1].contiguous(), [0, 1, 0, 0, 0, 0, 0, 0])
    assert st.drain(None, total, False)["len"][1] == d["len"][1]
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer
    s = CtcStreamer(2, 32, "ctc_prefix_beam_search", beam, None, 0, max_total_frames=40)
    s.feed(logp[:2, :32].cuda())
    with pytest.raises(PafcError, match=r"rows \[1\].*max_total_frames = 40"):
        s.feed(logp[:2, 32:64].cuda(), [8, 9])
    assert s._gpu.drain(None, 40, False)["overflow"] == [0, 1]


def test_feed_replayed_from_a_graph_equals_eager(hip, tmp_path):
    """One feed captured in a linear graph -- the kernel alone, on the object's fixed buffers -- replayed for the
    remaining chunks."""
    from paper_accurate_fast_cheap_amd import hip_ops
    beam = 8
    graph, logp, lens = case(tmp_path, beam)
    tables = graph.device_tables(torch.device("cuda", torch.cuda.current_device()))
    top_p, top_i = logp.cuda().topk(beam, dim=-1)
    eager = hip_ops.CtcBeamStream(B, 16, beam, beam, "cuda", 0, tables, T)
    run_stream(eager, top_p, top_i, lens.tolist(), cuts_of(T, 16, B))
    want = eager.drain(None, T, True)
    st = hip_ops.CtcBeamStream(B, 16, beam, beam, "cuda", 0, tables, T)
    cuts = cuts_of(T, 16, B)
    g = None
    for i, (width, rows) in enumerate(cuts):
        nf = [max(0, min(a + n, int(lens[b])) - a) for b, (a, n) in enumerate(rows)]
        a = rows[0][0]
        if i == 0:
            st.feed(top_p[:, a:a + width], top_i[:, a:a + width], nf)
            continue
        st.load(top_p[:, a:a + width], top_i[:, a:a + width], nf)
        if g is None:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                          # records the launch; nothing runs until the replay
                st.launch_feed()
        g.replay()
    torch.cuda.synchronize()
    assert st.drain(None, T, True) == want


def test_greedy_stream_equals_offline_kernel(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer, ctc_greedy_search
    logp, lens, _ = greedy_case()
    big = planted_logp(4, 300, 500, [[5, 6, 7]], seed=9)
    big_lens = torch.tensor([300, 211, 0, 97])
    for lp, ln, chunks in ((logp, lens, (1, 8, "ragged")), (big, big_lens, (16, 64, "ragged")), (big.bfloat16(), big_lens, (16,))):
        lp = lp.cuda()
        Bn, Tn = lp.shape[:2]
        toks, ntok, frames = hip_ops.ctc_greedy(lp, ln.cuda(), 0, want_frames=True)
        want_t = [toks[b, :int(ntok[b])].tolist() for b in range(Bn)]
        want_f = [frames[b, :int(ntok[b])].tolist() for b in range(Bn)]
        assert want_t == [r.tokens for r in ctc_greedy_search(lp, ln.cuda(), 0)]
        for how in chunks:
            s = CtcStreamer(Bn, 64 if how == "ragged" else how, "ctc_greedy_search")
            got = stream(s, lp, ln.tolist(), cuts_of(Tn, how, Bn, seed=3))
            assert [r.tokens for r in got] == want_t and [r.times for r in got] == want_f
    assert want_t[0] and sum(map(len, want_t)) > 50


def _stream_model(family, causal):
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from tests.test_rnnt_greedy import D, V as VOC, golden_model
    from tests.test_rnnt_greedy_stream_gpu import _stream_encoder
    if family == "asr":
        torch.manual_seed(3)
        return ASRModel(VOC, _stream_encoder(causal), CTC(VOC, D)).eval().cuda()
    model = golden_model(load_golden("rnnt_greedy_c5"), "cuda")
    model.encoder = _stream_encoder(causal)
    return model


@pytest.mark.parametrize("mode", ["ctc_prefix_beam_search", "ctc_greedy_search"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", ["asr", "transducer"])
def test_model_stream_ctc_search_equals_offline_on_the_same_encoder_steps(hip, tmp_path, family, causal, mode):
    """The streamed result equals the offline search of ctc_logprobs of the concatenated frames that the same streamed
    encoder steps produced.  The stream applies ctc_logprobs piece by piece; the test first asserts that the pieces' rows
    are bitwise those of the whole sequence, so that the comparison is about the decoder.  on_partial is called once per
    window."""
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_greedy_search, ctc_prefix_beam_search
    from tests.test_rnnt_greedy import V as VOC
    model = _stream_model(family, causal)
    chunk = 16
    speech = torch.randn(2, 4 * chunk * 6 + 3, 80, generator=torch.Generator().manual_seed(5)).cuda()
    graph, _ = synthetic_graph(tmp_path, 40, VOC, seed=11, context_score=2.0, pool=20)
    graph = graph if mode == "ctc_prefix_beam_search" else None
    seen = []
    with torch.no_grad():
        res = model.stream_ctc_search(speech, chunk, mode=mode, beam_size=4, context_graph=graph,
                                      on_partial=lambda i, part, com: seen.append((i, part, com)))
        enc = model.encoder
        sub, ctx = enc.embed.subsampling_rate, enc.embed.right_context + 1
        stride, window = sub * chunk, (chunk - 1) * sub + ctx
        Ts = speech.size(1)
        starts = list(range(0, Ts - ctx + 1, stride))
        pieces, ys, state = [], [], None
        for i, c in enumerate(starts):
            xs = speech[:, c:min(c + window, Ts)]
            if causal:
                y, state = enc.forward_chunk_carry(xs, 0, state)
            else:
                y, state = enc.forward_chunk_lookahead(xs, state, final=(i == len(starts) - 1))
            ys.append(y)
            pieces += [model.ctc_logprobs(y[:, a:a + chunk]) for a in range(0, y.size(1), chunk)]
        logp = torch.cat(pieces, 1)
        lens = torch.full((2,), logp.size(1), device="cuda")
        whole = model.ctc_logprobs(torch.cat(ys, 1))
        assert torch.equal(logp, whole)
        if mode == "ctc_greedy_search":
            ref = ctc_greedy_search(whole, lens, 0)
        else:
            ref = ctc_prefix_beam_search(whole, lens, 4, graph, 0)
    assert [i for i, _, _ in seen] == list(range(len(starts)))
    assert [list(r.tokens) for r in res] == [list(r.tokens) for r in ref]
    if mode == "ctc_prefix_beam_search":
        assert [r.nbest for r in res] == [r.nbest for r in ref] and [r.nbest_scores for r in res] == [r.nbest_scores for r in ref]
        assert [r.times for r in res] == [r.times for r in ref] and [r.nbest_times for r in res] == [r.nbest_times for r in ref]
    for b in range(2):                                        # what on_partial saw: committed tokens grow into the result
        prev = []
        for _, part, com in seen:
            assert com[b][:len(prev)] == prev
            prev = com[b]
        assert list(res[b].tokens)[:len(prev)] == prev
    assert sum(len(r.tokens) for r in res) > 0
