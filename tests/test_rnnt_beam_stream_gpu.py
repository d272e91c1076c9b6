"""Streaming CTC-fused RNN-T prefix beam search on the MI355X (hip_ops.RnntBeamStream, csrc/rnnt_beam_stream.hip:
pafc_rnnt_beam_stream_*, pafc_rnnt_beam_select_state; BeamStreamer; Transducer.stream_beam_search).

The kernels alone: synthetic candidates driven chunk by chunk against the offline kernels (hip_ops.RnntBeamState) on the
same inputs, bit for bit -- every frame's next_idx / last_tok, the drained token lists, lengths and float64 scores --,
overflow, drain with `from`, the state selection against the framework chain, bad arguments.  With the golden model: the
device path of BeamStreamer against PrefixBeamSearch._decode_batch_resident on the same GPU tensors, bit for bit (both run
the same frame body on the same B x beam slots, so every GEMM has the same shape), rows that start late and sit chunks
out, the host reads per feed, and Transducer.stream_beam_search on a reduced causal streaming encoder."""
import contextlib
import warnings

import pytest
import torch

from tests.conftest import load_golden
from tests.test_rnnt_beam_stream import cuts
from tests.test_search import _build

pytestmark = pytest.mark.gpu
B, T = 3, 37
LENS = (37, 20, 0)
CUTS = ["one", "sixteen", "irregular", "whole"]


# ---- the kernels alone -----------------------------------------------------------------------------------------------
def _candidates(beam, seed):
    """(B, T, beam, beam) top_val float32 / top_idx int64.  Ids: per slot a random permutation of a small vocabulary with
    blank 0 -- 6 tokens, or `beam` where a slot needs more distinct ids (top-k rows hold distinct ids) -- so merges and
    already-a-member hits are frequent.  Values: multiples of 1/4 over three units, sorted like a top-k row: many are
    exactly equal, which exercises both stable orders."""
    gen = torch.Generator().manual_seed(seed)
    V = max(6, beam)
    idx = torch.stack([torch.randperm(V, generator=gen)[:beam] for _ in range(B * T * beam)]).view(B, T, beam, beam)
    val = -torch.randint(0, 13, (B, T, beam, beam), generator=gen).float() / 4
    val = val.sort(dim=-1, descending=True).values
    return val.cuda().contiguous(), idx.cuda().contiguous()


_OFFLINE = {}


def _offline(beam):
    """RnntBeamState over all T frames: per frame (next_idx, last_tok), then (tokens, lengths, scores).  Computed once per beam."""
    if beam not in _OFFLINE:
        from paper_accurate_fast_cheap_amd import hip_ops
        tv, ti = _candidates(beam, 100 + beam)
        lens = torch.tensor(LENS, dtype=torch.int64, device="cuda")
        st = hip_ops.RnntBeamState(B, T, beam, 0, "cuda")
        frames = []
        for t in range(T):
            st.step(t, lens, tv[:, t].contiguous(), ti[:, t].contiguous())
            frames.append((st.next_idx.clone(), st.last_tok.clone()))
        toks, ln, sc = st.finish()
        _OFFLINE[beam] = (tv, ti, frames, toks.cpu(), ln.cpu(), sc.cpu())
    return _OFFLINE[beam]


def _lists(toks, ln):
    return [[toks[b, k, :ln[b, k]].tolist() if ln[b, k] >= 0 else None for k in range(ln.shape[1])] for b in range(ln.shape[0])]


@pytest.mark.parametrize("how", CUTS)
@pytest.mark.parametrize("beam", [1, 3, 8, 16])
def test_stream_kernels_equal_offline_kernels_bitwise(hip, beam, how):
    from paper_accurate_fast_cheap_amd import hip_ops
    tv, ti, frames, toks, ln, sc = _offline(beam)
    st = hip_ops.RnntBeamStream(B, 40, beam, 0, "cuda", max_total_frames=T)          # Tmax larger than every cut but "whole"
    for a, b in cuts(T, how):
        st.feed([max(0, min(L - a, b - a)) for L in LENS], b - a)
        for j in range(b - a):
            st.step(j, tv[:, a + j].contiguous(), ti[:, a + j].contiguous())
            assert torch.equal(st.next_idx, frames[a + j][0]), (a, j)
            assert torch.equal(st.last_tok, frames[a + j][1]), (a, j)
    d = st.drain(None, T)
    want = _lists(toks, ln)
    assert d["len"] == ln.tolist()
    assert d["count"] == [int((ln[b] >= 0).sum()) for b in range(B)]
    assert d["overflow"] == [0, 0, 0]
    for b in range(B):
        for k in range(beam):
            if want[b][k] is None:
                assert d["score"][b][k] == float("-inf")
            else:
                assert d["tokens"][b][k] == want[b][k]
                assert d["score"][b][k] == sc[b, k].item()                          # float64, bit for bit


def test_j_from_device_memory_equals_j_from_the_host(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    tv, ti, frames, toks, ln, sc = _offline(8)
    st = hip_ops.RnntBeamStream(B, 16, 8, 0, "cuda", max_total_frames=T)
    j_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    for a, b in cuts(T, "sixteen"):
        st.feed([max(0, min(L - a, b - a)) for L in LENS], b - a)
        j_dev.zero_()
        for j in range(16):                                    # always Tmax steps: those past a row's count are no-ops
            t = min(a + j, T - 1)
            st.step(0, tv[:, t].contiguous(), ti[:, t].contiguous(), j_dev=j_dev)
            j_dev.add_(1)
    d = st.drain(None, T)
    assert d["len"] == ln.tolist() and d["score"][0] == sc[0].tolist()
    assert d["tokens"][1][0] == toks[1, 0, :ln[1, 0]].tolist()


def test_overflow_consumes_nothing_and_holds_until_reset(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    tv, ti, *_ = _offline(3)
    st = hip_ops.RnntBeamStream(B, 16, 3, 0, "cuda", max_total_frames=20)
    st._ws.zero_()                                             # as if never reset
    st.reset([0, 1])

    def run(nf, a):
        st.feed(nf, 16)
        for j in range(16):
            st.step(j, tv[:, a + j].contiguous(), ti[:, a + j].contiguous())

    run([16, 10, 5], 0)
    d0 = st.drain(None, 40)
    assert d0["overflow"] == [0, 0, 2] and d0["count"][2] == 0          # the unreset row reports 2 and holds nothing
    run([5, 4, 1], 16)                                        # 16 + 5 > 20: row 0 takes nothing; row 1 goes on
    d1 = st.drain(None, 40)
    assert d1["overflow"] == [1, 0, 2]
    assert (d1["len"][0], d1["score"][0], d1["tokens"][0]) == (d0["len"][0], d0["score"][0], d0["tokens"][0])
    assert max(d1["len"][1]) >= max(d0["len"][1]) and d1["score"][1] != d0["score"][1]
    run([1, 0, 0], 16)                                        # the flag holds although one frame would fit
    d2 = st.drain(None, 40)
    assert d2["overflow"] == [1, 0, 2] and d2["score"][0] == d0["score"][0]
    st.reset([0, 2])
    run([4, 0, 4], 0)
    d3 = st.drain(None, 40)
    assert d3["overflow"] == [0, 0, 0] and d3["count"][2] >= 1 and max(d3["len"][0]) <= 4
    assert d3["score"][1] == d1["score"][1]                   # a row without frames is untouched


def test_drain_from_the_committed_count_returns_the_same_lists(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    tv, ti, *_ = _offline(3)
    # frames 0 .. 3: one token far ahead of the rest in every slot, so that the descendants of one hypothesis take the
    # beam over and a prefix is committed whatever the random frames behind them do
    tv, ti = tv.clone(), ti.clone()
    for t in range(4):
        for b in range(B):
            for m in range(3):
                rest = [int(v) for v in ti[b, t, m].tolist() if int(v) != 1 + t][:2]
                ti[b, t, m] = torch.tensor([1 + t] + rest, device="cuda")
        tv[:, t] = torch.tensor([0.0, -61.0, -62.0], device="cuda")
    st = hip_ops.RnntBeamStream(B, 16, 3, 0, "cuda", max_total_frames=T)
    counts = [0] * B
    grew = False
    for a, b in cuts(T, "sixteen"):
        st.feed([max(0, min(L - a, b - a)) for L in LENS], b - a)
        for j in range(b - a):
            st.step(j, tv[:, a + j].contiguous(), ti[:, a + j].contiguous())
        full = st.drain(None, T)
        part = st.drain(counts, T)
        for r in range(B):
            live = [full["tokens"][r][k] for k in range(full["count"][r])]
            lcp = min(len(x) for x in live)
            while any(x[:lcp] != live[0][:lcp] for x in live):
                lcp -= 1
            assert full["committed"][r] == lcp and part["committed"][r] == lcp
            assert part["len"][r] == full["len"][r] and part["score"][r] == full["score"][r]
            for k in range(full["count"][r]):
                assert live[k][:counts[r]] == live[0][:counts[r]]
                assert part["tokens"][r][k] == live[k][counts[r]:]
            short = st.drain(counts, 1)                       # ld bounds the copy, not the counts
            assert short["tokens"][r][0] == live[0][counts[r]:counts[r] + 1] and short["len"][r] == full["len"][r]
            grew = grew or lcp > 0
            counts[r] = lcp
    assert grew                                               # rows 0 and 1 commit behind the forced frames


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hidden", [640, 12])
def test_select_state_equals_the_framework_chain_bitwise(hip, dtype, hidden):
    from paper_accurate_fast_cheap_amd import hip_ops
    Bn, beam, L = 3, 8, 2
    n = Bn * beam
    gen = torch.Generator().manual_seed(hidden)
    h, c, hn, cn = (torch.randn(L, n, hidden, generator=gen).to(dtype).cuda() for _ in range(4))
    # within each utterance: a random slot of its own, old and new targets mixed
    own = torch.randint(0, beam, (n,), generator=gen) + torch.arange(n) // beam * beam
    idx = (own + torch.randint(0, 2, (n,), generator=gen) * n).cuda()
    assert bool((idx < n).any()) and bool((idx >= n).any())
    want_h = torch.cat([h, hn], dim=1).index_select(1, idx)
    want_c = torch.cat([c, cn], dim=1).index_select(1, idx)
    keep = (hn.clone(), cn.clone())
    hip_ops.rnnt_beam_select_state(h, c, hn, cn, idx, Bn, beam)
    assert torch.equal(h, want_h) and torch.equal(c, want_c)
    assert torch.equal(hn, keep[0]) and torch.equal(cn, keep[1])


def test_bad_arguments_are_rejected(hip):
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    with pytest.raises(_lib.PafcError):
        hip_ops.RnntBeamStream(B, 16, 17, 0, "cuda")
    st = hip_ops.RnntBeamStream(B, 16, 8, 0, "cuda", max_total_frames=40)
    L, p = _lib.lib(), _lib.ptr
    tv = torch.zeros(B, 8, 8, device="cuda")
    ti = torch.zeros(B, 8, 8, dtype=torch.int64, device="cuda")
    s = _lib.stream_of(tv)
    assert L.pafc_rnnt_beam_stream_step(B, 16, 40, 17, 0, 0, None, p(tv), p(ti), p(st._ws), st._nbytes, p(st.next_idx), p(st.last_tok), s) == -7
    assert L.pafc_rnnt_beam_stream_step(B, 16, 40, 8, 0, 0, None, p(tv), p(ti), p(st._ws), st._nbytes - 1, p(st.next_idx), p(st.last_tok), s) == -4
    assert L.pafc_rnnt_beam_stream_step(B, 16, 40, 8, 0, 0, None, None, p(ti), p(st._ws), st._nbytes, p(st.next_idx), p(st.last_tok), s) == -1
    assert L.pafc_rnnt_beam_stream_feed(B, 16, 40, 8, None, p(st._ws), st._nbytes, s) == -1
    assert L.pafc_rnnt_beam_stream_reset(B, 40, 8, 0, None, None, st._nbytes, p(st.next_idx), p(st.last_tok), s) == -1
    assert L.pafc_rnnt_beam_stream_drain(B, 40, 8, p(st._ws), st._nbytes, None, 4, None, None, None, None, None, None, s) == -1
    assert L.pafc_rnnt_beam_select_state(0, 2, B, 8, 64, None, None, None, None, None, s) == -1
    with pytest.raises(_lib.PafcError):
        st.step(0, tv.double(), ti)
    with pytest.raises(_lib.PafcError):
        hip_ops.rnnt_beam_select_state(tv, tv, tv, tv.bfloat16(), ti.view(-1)[:B * 8], B, 8)


# ---- with the golden model -------------------------------------------------------------------------------------------
_WORLD = {}


def _world():
    if not _WORLD:
        g = load_golden("search_c5")
        ctc, pred, joint, bs = _build(g, "cuda")
        with torch.no_grad():
            enc, lens = g["enc_out"].cuda(), g["enc_lens"].cuda()
            logp = ctc.log_softmax(enc)
        _WORLD.update(bs=bs, enc=enc, lens=lens, logp=logp, offline={})
    return _WORLD


def _offline_decode(beam):
    w = _world()
    if beam not in w["offline"]:
        with torch.no_grad():
            w["offline"][beam] = w["bs"]._decode_batch_resident(w["enc"], w["lens"], w["logp"], beam, 0.3, 0.7)
    return w["offline"][beam]


def _run(st, w, how):
    lens = w["lens"].tolist()
    hist = []
    for a, b in cuts(w["enc"].shape[1], how):
        st.feed(w["enc"][:, a:b], w["logp"][:, a:b], [max(0, min(L - a, b - a)) for L in lens])
        hist.append([list(c) for c in st.committed])
    return st.results(), hist


def _equal(res, ref):
    for r, o in zip(res, ref):
        assert [list(n) for n in r.nbest] == [list(n) for n in o.nbest]
        assert r.nbest_scores == o.nbest_scores and r.score == o.score and list(r.tokens) == list(o.tokens)


@pytest.mark.parametrize("how", CUTS)
@pytest.mark.parametrize("beam", [8, 3, 1])
def test_streamer_equals_offline_resident_decode_bitwise(hip, beam, how):
    from paper_accurate_fast_cheap_amd.transducer.search.prefix_beam_search import BeamStreamer
    w = _world()
    assert w["enc"].shape[1] >= 8                               # the offline body is the captured one
    st = BeamStreamer(w["bs"], 3, 37, beam, 0.3, 0.7, max_total_frames=64)
    res, hist = _run(st, w, how)
    _equal(res, _offline_decode(beam))
    for r in range(3):                                          # committed: final at every feed, never shrinking
        prev = []
        for h in hist:
            assert list(res[r].tokens[:len(h[r])]) == h[r] and h[r][:len(prev)] == prev
            prev = h[r]


def test_graph_replay_equals_eager_streamer_and_eager_offline(hip):
    from paper_accurate_fast_cheap_amd.transducer.search.prefix_beam_search import BeamStreamer
    w = _world()
    bs = w["bs"]
    graphed = BeamStreamer(bs, 3, 16, 8, 0.3, 0.7, max_total_frames=64)
    res_g, _ = _run(graphed, w, "irregular")
    eager = BeamStreamer(bs, 3, 16, 8, 0.3, 0.7, max_total_frames=64, use_graph=False)
    res_e, _ = _run(eager, w, "irregular")
    assert not eager.graphed
    _equal(res_g, res_e)
    bs.use_graph = False
    try:
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
            off = bs._decode_batch_resident(w["enc"], w["lens"], w["logp"], 8, 0.3, 0.7)
    finally:
        bs.use_graph = True
    _equal(res_e, off)
    _equal(res_g, _offline_decode(8))


def test_row_lifecycle_late_start_and_idle_chunk(hip):
    """Row 1 starts two chunks late (reset there), row 2 sits chunk 1 out.  Each row's tokens equal the offline decode of
    that utterance in the same row of a same-B batch; scores within 2e-3, test_search's bound for differently batched GEMMs."""
    from paper_accurate_fast_cheap_amd.transducer.search.prefix_beam_search import BeamStreamer
    w = _world()
    enc, logp, lens = w["enc"], w["logp"], w["lens"].tolist()
    C = 8
    st = BeamStreamer(w["bs"], 3, C, 8, 0.3, 0.7, max_total_frames=64)
    pos = [0, 0, 0]
    c = 0
    while any(pos[r] < lens[r] for r in range(3)):
        if c == 2:
            st.reset([1])
        e = torch.zeros(3, C, enc.shape[2], device="cuda")
        l = torch.zeros(3, C, logp.shape[2], device="cuda")
        nf = []
        for r in range(3):
            idle = (r == 1 and c < 2) or (r == 2 and c == 1)
            n = 0 if idle else min(C, lens[r] - pos[r])
            e[r, :n], l[r, :n] = enc[r, pos[r]:pos[r] + n], logp[r, pos[r]:pos[r] + n]
            pos[r] += n
            nf.append(n)
        before = [list(x) for x in st.committed]
        part = st.feed(e, l, nf)
        if c == 1:
            assert st.committed[2] == before[2] and part[2].nbest_scores == kept    # the idle row keeps its beam
        kept = part[2].nbest_scores
        c += 1
    for r, o in zip(st.results(), _offline_decode(8)):
        assert [list(n) for n in r.nbest] == [list(n) for n in o.nbest]
        assert r.nbest_scores == pytest.approx(o.nbest_scores, abs=2e-3)


_HOST = {}


def _short(T):
    """The first T frames of the golden batch with ragged lengths (T, T // 2, 1) -- rows that end inside the two warm-up
    frames included -- and the host loop's result on them, computed once per T."""
    w = _world()
    if T not in _HOST:
        enc, logp = w["enc"][:, :T].contiguous(), w["logp"][:, :T].contiguous()
        lens = torch.tensor([T, T // 2, 1], device="cuda")
        bs = w["bs"]
        bs.device_resident = False
        try:
            with torch.no_grad():
                host = bs.prefix_beam_search_decode(enc, lens, logp, beam_size=3, ctc_weight=0.3, transducer_weight=0.7)
        finally:
            bs.device_resident = True
        _HOST[T] = (enc, lens, logp, host)
    return _HOST[T]


@pytest.mark.parametrize("frame_body", ["framework", "kernels"])
def test_offline_warm_up_frames_are_counted_at_every_length(hip, frame_body):
    """The offline resident decode at the lengths around its `use_graph and T >= 8` rule: T = 1, 2, 7 run eagerly, T = 8 is the
    two warm-up frames plus six replays, T = 9 the graph path, and T = 9 again without the graph.  Each against the host loop
    on the same tensors: equal n-best token lists, scores within 2e-3 (test_search's bound for the two paths' differently
    batched GEMMs).  The graphed and the eager T = 9 results are equal bit for bit (the framework body runs the framework's
    own LSTM cell under the graph, so its eager run does too)."""
    bs = _world()["bs"]
    assert bs.use_graph
    got = {}
    try:
        for T, use_graph in ((1, True), (2, True), (7, True), (8, True), (9, True), (9, False)):
            enc, lens, logp, host = _short(T)
            bs.use_graph = use_graph
            with torch.no_grad(), contextlib.nullcontext() if use_graph else torch.backends.cudnn.flags(enabled=False):
                res = bs.prefix_beam_search_decode(enc, lens, logp, beam_size=3, ctc_weight=0.3, transducer_weight=0.7,
                                                   frame_body=frame_body)
            got[T, use_graph] = res
            print(frame_body, T, use_graph, [max((abs(a - b) for a, b in zip(r.nbest_scores, h.nbest_scores)), default=0.0)
                                             for r, h in zip(res, host)])
            for r, h in zip(res, host):
                assert [list(n) for n in r.nbest] == [list(n) for n in h.nbest], (T, use_graph)
                assert r.nbest_scores == pytest.approx(h.nbest_scores, abs=2e-3), (T, use_graph)
                assert list(r.tokens) == list(h.tokens)
    finally:
        bs.use_graph = True
    _equal(got[9, True], got[9, False])


@pytest.mark.parametrize("partials", [True, False])
def test_host_reads_per_feed_are_as_documented(hip, partials):
    """One synchronising call per feed, the drain's read; none with partials switched off."""
    from paper_accurate_fast_cheap_amd.transducer.search.prefix_beam_search import BeamStreamer
    w = _world()
    st = BeamStreamer(w["bs"], 3, 8, 8, 0.3, 0.7, max_total_frames=64, partials=partials)
    st.feed(w["enc"][:, :8], w["logp"][:, :8])                  # warm: binding, allocator, the captured body
    torch.cuda.synchronize()
    assert st.graphed
    for a in (8, 16):
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                st.feed(w["enc"][:, a:a + 8], w["logp"][:, a:a + 8], [8, 8, max(0, 11 - a)])
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        reads = [x for x in rec if "synchroniz" in str(x.message).lower()]
        assert len(reads) == (1 if partials else 0), [str(x.message)[:80] for x in reads]
    assert len(st.results()) == 3


def test_model_stream_beam_search_equals_offline_on_the_same_encoder_steps(hip):
    from tests.test_rnnt_greedy import golden_model
    from tests.test_rnnt_greedy_stream_gpu import _stream_encoder
    model = golden_model(load_golden("rnnt_greedy_c5"), "cuda")
    model.encoder = _stream_encoder(True)
    chunk = 16
    speech = torch.randn(2, 4 * chunk * 4 + 3, 80, generator=torch.Generator().manual_seed(5)).cuda()
    seen = []
    with torch.no_grad():
        res = model.stream_beam_search(speech, chunk, beam_size=8,
                                       on_partial=lambda i, part, com: seen.append((i, [list(p.tokens) for p in part], com)))
        enc = model.encoder                                     # the same encoder steps, concatenated
        sub, ctx = enc.embed.subsampling_rate, enc.embed.right_context + 1
        stride, window = sub * chunk, (chunk - 1) * sub + ctx
        Tn = speech.size(1)
        starts = list(range(0, Tn - ctx + 1, stride))
        ys, state = [], None
        for c in starts:
            y, state = enc.forward_chunk_carry(speech[:, c:min(c + window, Tn)], 0, state)
            ys.append(y)
        Y = torch.cat(ys, 1)
        ref = model.beam_search_decode(Y, torch.full((2,), Y.size(1), device="cuda"), model.ctc_logprobs(Y), beam_size=8,
                                       ctc_weight=0.3, transducer_weight=0.7)
    assert [i for i, _, _ in seen] == list(range(len(starts)))
    for b in range(2):
        # (the CTC head sees a chunk's rows here and all rows offline: its GEMM may round the last bits differently, so the
        # scores and the order far down the n-best are not pinned; the decoded tokens are)
        assert list(res[b].tokens) == list(ref[b].tokens)
        prev = []
        for _, part, com in seen:                               # committed lists: final and never shrinking
            assert com[b][:len(prev)] == prev and list(res[b].tokens[:len(com[b])]) == com[b]
            prev = com[b]
    assert sum(len(r.tokens) for r in res) > 0
