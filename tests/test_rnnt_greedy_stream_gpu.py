"""Streaming RNN-T greedy search on the MI355X (hip_ops.RnntGreedyStream, csrc/rnnt_greedy.hip: pafc_rnnt_greedy_stream_*):
the streamed decode of a chunked stream against the offline kernel decode of the concatenated frames, bit for bit (tokens,
absolute frames, float64 scores), rows that start late and sit chunks out, graph replay against eager, two streamers on two
streams, the host reads per feed, and Transducer.stream_greedy_search on reduced streaming encoders.

Exactness needs the same E = enc_ffn rows on both sides.  The streamer projects its fixed (B * Tmax)-row buffer, the offline
path its (B * T)-row input; the package GEMMs pick their kernel by the row count, and the fp32 few-rows kernel splits K over
the waves of a block, so the test shapes keep both calls in the staged-tile family (B * Tmax >= 512 rows at J = 640) and the
first test asserts that the rows are bitwise equal before anything relies on it."""
import math
import os
import sys
import warnings

import pytest
import torch

from tests.conftest import load_golden
from tests.test_rnnt_greedy import golden_model

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bench_rnnt_greedy as BG  # noqa: E402

pytestmark = pytest.mark.gpu
TMAX = {8: 64, 64: 16}            # streamer rows per B: B * Tmax >= 512


def _cuts(T, how):
    if how == "irregular":
        sizes, out, a, i = [3, 1, 9, 2, 16, 5, 11, 4], [], 0, 0
        while a < T:
            out.append((a, min(T, a + sizes[i % len(sizes)])))
            a, i = out[-1][1], i + 1
        return out
    step = {"one": 1, "sixteen": 16}[how]
    return [(a, min(T, a + step)) for a in range(0, T, step)]


def _stream(st, enc, lens, cuts):
    """Feed enc (B, T, D) chunk by chunk, row b getting the frames it has left; concatenated tokens and frames."""
    B = enc.shape[0]
    toks, frames = [[] for _ in range(B)], [[] for _ in range(B)]
    for a, b in cuts:
        nf = torch.tensor([max(0, min(b, int(L)) - a) for L in lens], dtype=torch.int64, device=enc.device)
        tk, fr = st.feed(enc[:, a:b], nf)
        for r in range(B):
            toks[r] += tk[r]
            frames[r] += fr[r]
    return toks, frames, st.score


def _row_state(st, b):
    """The bytes of row b's carried decoder state in a RnntGreedyStream's workspace: tok, need, k, slot, score, both LSTM
    slots (h and c, every layer), pred_out and P -- the layout of csrc/rnnt_greedy.hip (layout + stream_layout), mirrored
    here and checked against the workspace size."""
    al = lambda n: (n + 255) // 256 * 256
    n = st._net
    B, L, H, Pd, J, V = st.B, n.num_layers, n.hidden, n.pred_dim, n.join_dim, n.vocab
    ns, cap = (V + 31) // 32, st.Tmax * st.n_steps
    off, o = {}, 0
    for name, size in ([(f, B * 4) for f in ("Tb", "t", "tok", "need", "k", "ntok", "slot", "act", "live")]
                       + [("ctl", 8), ("score", B * 8), ("hs", 2 * L * B * H * 4), ("cs", 2 * L * B * H * 4),
                          ("pred", B * Pd * 4), ("P", B * J * 4), ("pmax", ns * B * 4), ("psum", ns * B * 4),
                          ("parg", ns * B * 4), ("otok", B * cap * 4), ("ofr", B * cap * 4), ("base", B * 8)]):
        off[name], o = o, o + al(size)
    assert o == st._nbytes
    ws = st._ws.cpu()
    parts = [ws[off[f] + 4 * b:off[f] + 4 * b + 4] for f in ("tok", "need", "k", "slot")]
    parts.append(ws[off["score"] + 8 * b:off["score"] + 8 * b + 8])
    for f in ("hs", "cs"):
        for sl in range(2):
            for l in range(L):
                q = off[f] + (((sl * L + l) * B + b) * H) * 4
                parts.append(ws[q:q + H * 4])
    parts.append(ws[off["pred"] + b * Pd * 4:off["pred"] + (b + 1) * Pd * 4])
    parts.append(ws[off["P"] + b * J * 4:off["P"] + (b + 1) * J * 4])
    return torch.cat(parts)


def _model(dtype, seed):
    return BG.to(BG.make_model(seed=seed, drive=0.5), "cuda", dtype)


@pytest.mark.parametrize("B", [8, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_chunk_projection_rows_equal_whole_batch_rows(hip, dtype, B):
    from paper_accurate_fast_cheap_amd import hip_ops
    model = _model(dtype, 11)
    enc, lens = BG.make_batch(B, 60, seed=11)
    enc = enc.to("cuda", dtype)
    Tm = TMAX[B]
    st = hip_ops.RnntGreedyStream(model.predictor, model.joint, B, Tm)
    ef = model.joint.enc_ffn
    gemm = hip_ops.gemm_f32 if dtype == torch.float32 else hip_ops.gemm_bf16
    with torch.no_grad():
        whole = gemm(enc.reshape(-1, enc.shape[2]).contiguous(), ef.weight.detach().contiguous(),
                     ef.bias.detach().contiguous()).view(B, 60, -1)
        for a, b in ((0, 16), (16, 17), (17, 60 if Tm >= 43 else 33)):
            st.feed(enc[:, a:b])
            E = st._E.view(B, Tm, -1)[:, :b - a]
            assert torch.equal(E, whole[:, a:b]), (a, b)


@pytest.mark.parametrize("how", ["one", "sixteen", "irregular"])
@pytest.mark.parametrize("B", [8, 64])
@pytest.mark.parametrize("n_steps", [64, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_streamed_decode_equals_offline_kernel_decode_bitwise(hip, dtype, n_steps, B, how):
    from paper_accurate_fast_cheap_amd import hip_ops
    model = _model(dtype, 12)
    enc, lens = BG.make_batch(B, 60, seed=12, zero_row=True)
    enc = enc.to("cuda", dtype)
    with torch.no_grad():
        ref_t, ref_f, ref_s = hip_ops.rnnt_greedy_search(model.predictor, model.joint, enc, lens.cuda(), 0, n_steps)
        st = hip_ops.RnntGreedyStream(model.predictor, model.joint, B, TMAX[B], n_steps)
        toks, frames, scores = _stream(st, enc, lens.tolist(), _cuts(60, how))
    assert toks == ref_t
    assert frames == ref_f
    assert scores == ref_s                       # float64, ==
    assert sum(len(t) for t in toks) > 0


def test_golden_tokens_on_the_streamer(hip):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import GreedyStreamer
    g = load_golden("rnnt_greedy_c5")
    for n_steps in (64, 2):
        model = golden_model(g, "cuda")
        s = GreedyStreamer(model, 3, 7, n_steps)
        enc, lens = g["enc_out"].cuda(), g["enc_lens"].tolist()
        with torch.no_grad():
            for a in range(0, enc.shape[1], 7):
                s.feed(enc[:, a:a + 7], [max(0, min(a + 7, L) - a) for L in lens])
        assert [r.tokens for r in s.results()] == g["tokens"][n_steps]


def test_row_lifecycle_late_starts_and_idle_chunks(hip):
    """Rows restarted by reset at different chunks, sitting some chunks out: each equals the offline decode of its own
    frames (in an offline batch of the same B, so E comes from the same GEMM family), and a row that sits a chunk out emits
    nothing and keeps its carried state (LSTM slots, tok, need, k, slot, pred_out, P, score) byte for byte."""
    from paper_accurate_fast_cheap_amd import hip_ops
    B, Tm, C = 8, 64, 10
    model = _model(torch.float32, 13)
    enc, _ = BG.make_batch(B, 120, seed=13)
    enc = enc.cuda()
    start = [0, 1, 2, 3, 0, 2, 4, 1]                      # chunk at which row b is reset
    idle = {(1, 3), (1, 5), (4, 1), (4, 2), (6, 6), (7, 3)}     # (row, chunk) with no frames
    st = hip_ops.RnntGreedyStream(model.predictor, model.joint, B, Tm)
    pos = [0] * B
    own = [[] for _ in range(B)]                          # the frames each row has decoded since its reset
    toks, frames = [[] for _ in range(B)], [[] for _ in range(B)]
    with torch.no_grad():
        for c in range(9):
            rs = [b for b in range(B) if start[b] == c and c > 0]
            if rs:
                st.reset(rs)
                for b in rs:
                    toks[b], frames[b], pos[b], own[b] = [], [], 0, []
            before = st.score
            idle_now = [b for b in range(B) if c >= start[b] and (b, c) in idle]
            snap = {b: _row_state(st, b) for b in idle_now}
            chunk = torch.zeros(B, C, enc.shape[2], device="cuda")
            nf = []
            for b in range(B):
                n = 0 if (c < start[b] or (b, c) in idle) else C
                chunk[b, :n] = enc[b, pos[b]:pos[b] + n]
                own[b].append(enc[b, pos[b]:pos[b] + n])
                pos[b] += n
                nf.append(n)
            tk, fr = st.feed(chunk, torch.tensor(nf, device="cuda"))
            for b in range(B):
                toks[b] += tk[b]
                frames[b] += fr[b]
                if nf[b] == 0:
                    assert tk[b] == [] and st.score[b] == before[b]
            for b in idle_now:                              # an idle row's carried state, byte for byte
                assert torch.equal(_row_state(st, b), snap[b]), (b, c)
    T = max(pos)
    whole = torch.zeros(B, T, enc.shape[2], device="cuda")
    for b in range(B):
        whole[b, :pos[b]] = torch.cat(own[b])
    with torch.no_grad():
        ref_t, ref_f, ref_s = hip_ops.rnnt_greedy_search(model.predictor, model.joint, whole, torch.tensor(pos).cuda())
    assert toks == ref_t and frames == ref_f and st.score == ref_s


def test_graph_replay_equals_eager_and_two_streams_equal_sequential(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    model = _model(torch.float32, 14)
    enc, lens = BG.make_batch(8, 60, seed=14)
    enc = enc.cuda()
    cuts = _cuts(60, "irregular")
    with torch.no_grad():
        eager = _stream(hip_ops.RnntGreedyStream(model.predictor, model.joint, 8, 64, use_graph=False), enc, lens.tolist(), cuts)
        gs = hip_ops.RnntGreedyStream(model.predictor, model.joint, 8, 64)
        graphed = _stream(gs, enc, lens.tolist(), cuts)
        assert gs.graphed
    assert graphed == eager
    enc2, lens2 = BG.make_batch(8, 60, seed=15)
    enc2 = enc2.cuda()
    with torch.no_grad():
        seq2 = _stream(hip_ops.RnntGreedyStream(model.predictor, model.joint, 8, 64), enc2, lens2.tolist(), cuts)
        a = hip_ops.RnntGreedyStream(model.predictor, model.joint, 8, 64)
        b = hip_ops.RnntGreedyStream(model.predictor, model.joint, 8, 64)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        sa.wait_stream(torch.cuda.current_stream())
        sb.wait_stream(torch.cuda.current_stream())
        out = [[[[] for _ in range(8)], [[] for _ in range(8)]] for _ in range(2)]
        for x, y in cuts:                                      # the two streamers interleaved, each on its own stream
            for i, (s, e, L, strm) in enumerate(((a, enc, lens, sa), (b, enc2, lens2, sb))):
                with torch.cuda.stream(strm):
                    nf = torch.tensor([max(0, min(y, int(l)) - x) for l in L], device="cuda")
                    tk, fr = s.feed(e[:, x:y], nf)
                for r in range(8):
                    out[i][0][r] += tk[r]
                    out[i][1][r] += fr[r]
        torch.cuda.synchronize()
    assert (out[0][0], out[0][1], a.score) == eager
    assert (out[1][0], out[1][1], b.score) == seq2


def test_host_reads_per_feed_are_as_documented(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    model = _model(torch.float32, 16)
    enc, _ = BG.make_batch(8, 48, seed=16)
    enc = enc.cuda()
    st = hip_ops.RnntGreedyStream(model.predictor, model.joint, 8, 16)
    with torch.no_grad():
        st.feed(enc[:, :16])                             # warm: binding, allocator, the graph for n = 16
        torch.cuda.synchronize()
        for a in (16, 32):
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as w:
                    warnings.simplefilter("always")
                    toks, frames = st.feed(enc[:, a:a + 16])
            finally:
                torch.cuda.set_sync_debug_mode(prev)
            reads = [x for x in w if "synchroniz" in str(x.message).lower()]
            S = BG.count_steps(toks, [[f - a for f in fr] for fr in frames], [16] * 8, 64)
            expect = 2 + math.ceil(max(0, S - 16) / hip_ops.RNNT_GREEDY_CHUNK)
            assert len(reads) == expect, ([str(x.message)[:80] for x in reads], S)


def _stream_encoder(causal):
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = dict(output_size=128, attention_heads=2, linear_units=256, num_blocks=2, input_layer="conv2d", normalize_before=True,
                cnn_module_kernel=15 if causal else 31, causal=causal, use_cnn_module=True, cnn_module_norm="layer_norm",
                activation_type="swish", pos_enc_layer_type="rel_pos", selfattention_layer_type="rwkv_tmix60",
                rnn_att_version="rwkv", rnn_att_direction="uni", rwkv_ctx_len=2048, rwkv_do_bfloat16=False)
    torch.manual_seed(21 if causal else 22)
    return ConformerEncoder(80, **conf).cuda().eval()


@pytest.mark.parametrize("causal", [True, False])
def test_model_stream_greedy_search_equals_offline_on_the_same_encoder_steps(hip, causal):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import batch_greedy_search
    g = load_golden("rnnt_greedy_c5")
    model = golden_model(g, "cuda")
    model.encoder = _stream_encoder(causal)
    chunk = 16
    speech = torch.randn(2, 4 * chunk * 6 + 3, 80, generator=torch.Generator().manual_seed(5)).cuda()
    seen = []
    with torch.no_grad():
        res = model.stream_greedy_search(speech, chunk, on_tokens=lambda i, new: seen.append((i, new)))
        enc = model.encoder                                     # the same encoder steps, concatenated
        sub, ctx = enc.embed.subsampling_rate, enc.embed.right_context + 1
        stride, window = sub * chunk, (chunk - 1) * sub + ctx
        T = speech.size(1)
        starts = list(range(0, T - ctx + 1, stride))
        ys, state = [], None
        for i, c in enumerate(starts):
            xs = speech[:, c:min(c + window, T)]
            if causal:
                y, state = enc.forward_chunk_carry(xs, 0, state)
            else:
                y, state = enc.forward_chunk_lookahead(xs, state, final=(i == len(starts) - 1))
            ys.append(y)
        Y = torch.cat(ys, 1)
        ref = batch_greedy_search(model, Y, torch.full((2,), Y.size(1), device="cuda"), 64)
        whole = model.greedy_search(speech, torch.full((2,), T, device="cuda"))
    assert [i for i, _ in seen] == list(range(len(starts)))
    for b in range(2):
        assert sum((new[b] for _, new in seen), []) == res[b].tokens
    assert [r.tokens for r in res] == [r.tokens for r in ref]
    assert [r.times for r in res] == [r.times for r in ref]
    assert [r.score for r in res] == [r.score for r in ref]
    assert sum(len(r.tokens) for r in res) > 0
    agree = sum(int(r.tokens == w) for r, w in zip(res, whole))
    print(f"stream_greedy_search ({'causal' if causal else 'look-ahead'}) vs whole-utterance greedy_search: "
          f"{agree} / 2 streams with identical tokens")
