"""utils.stream_pool.StreamPool on the reduced streaming models: independent streams that open, bring irregular packets and
close at different moments, through fewer slots than streams.
(a) one row per step: every stream's result equals AudioStreamer(model, 1, ...) of that stream alone, with ==;
(b) any batching: a driver made of public pieces replays pool.step_log -- slices of fbank_batch, carries joined and split by
    torch indexing, zero rows for padding, the same forward_chunk_carry call -- and gets bitwise the step outputs and results;
(c) against the stream alone: only the GEMM tile a row lands in differs, bounded as the lock-step path bounds it."""
import random

import pytest
import torch

from tests import parity_log
from tests.conftest import load_golden
from tests.test_audio_stream_gpu import AUDIO, _bitwise, _model, _same
from tests.test_ctc_context_gpu import synthetic_graph
from tests.test_fbank_gpu import _wave

pytestmark = pytest.mark.gpu
SLOTS = 3
BSLOTS = 5                            # the batched runs: a step of three rows is padded to four
# five streams through three slots: the three lengths of test_audio_stream_gpu (last window full / short last window / no
# window at all) and two more
LENGTHS = dict(AUDIO, **{"141 frames": 400 + 160 * 140 + 33, "200 frames": 400 + 160 * 199})
ORDER = ["short last window", "fewer frames than ctx", "141 frames", "last window full", "200 frames"]
_cache = {}


def _audio(names):
    return {name: _wave(LENGTHS[name], 40 + i).cuda() for i, name in enumerate(names)}


def _bf16_model():
    """The bf16 causal encoder of test_fused_state_carry_step_serves_concurrent_streams (the fused chunk step) under a CTC head."""
    if "bf16" not in _cache:
        from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
        from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
        from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
        from tests.test_rnnt_greedy import V as VOC
        g = load_golden("encoder_reduced_uni_bf16model")
        conf = dict(g["conf"], causal=True, cnn_module_kernel=15)
        torch.manual_seed(6)
        enc = ConformerEncoder(80, **conf)
        with torch.no_grad():
            for n, p in enc.named_parameters():
                if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                    p.normal_(0, 0.05)
        torch.manual_seed(7)
        model = ASRModel(VOC, enc, CTC(VOC, conf["output_size"])).to(torch.bfloat16).cuda().eval()
        model.encoder.fused_inference = True
        _cache["bf16"] = model
    return _cache["bf16"]


def _serve(pool, audio, order, seed, lo=1, hi=9000):
    """Streams open at different feeds, bring irregular packets (some feeds skip a stream, some bring it nothing), and close
    one at a time while the others go on.  -> ({name: result}, {sid: name})"""
    rng = random.Random(seed)
    pending, live, results, names, committed = list(order), {}, {}, {}, {}
    tick = 0
    while pending or live:
        want = 2 if tick < 2 else len(live) + 1
        while pending and len(live) < min(want, pool.S):
            sid = pool.open()
            names[sid] = pending.pop(0)
            live[sid], committed[sid] = 0, []
        sids = [s for s in live if rng.random() < 0.85]
        rng.shuffle(sids)
        if sids:
            ns = [min(rng.randint(lo, hi), audio[names[s]].size(1) - live[s]) for s in sids]
            buf = torch.zeros(len(sids), max(ns) + 5, device=next(iter(audio.values())).device)
            for i, (s, n) in enumerate(zip(sids, ns)):
                buf[i, :n] = audio[names[s]][0, live[s]:live[s] + n]
                live[s] += n
            part = pool.feed(sids, buf, ns)
            assert set(part) == set(sids)
            for s in live:                                       # .committed only grows
                now = pool.committed(s)
                assert now[:len(committed[s])] == committed[s]
                committed[s] = now
        for s in [s for s in live if live[s] == audio[names[s]].size(1)][:1]:
            res = pool.close(s)
            assert list(res.tokens)[:len(committed[s])] == committed[s]
            results[names[s]] = res
            del live[s]
            assert s not in pool.active
        tick += 1
    assert pool.active == []
    return results, names


def _kwargs(mode, tmp_path):
    from tests.test_rnnt_greedy import V as VOC
    if mode == "ctc_prefix_beam_search":
        return dict(beam_size=4, context_graph=synthetic_graph(tmp_path, 40, VOC, seed=11, context_score=2.0, pool=20)[0])
    return {}


@pytest.mark.parametrize("mode", ["ctc_prefix_beam_search", "ctc_greedy_search", "rnnt_greedy_search"])
def test_one_row_per_step_equals_the_audio_streamer_of_each_stream_alone(hip, tmp_path, mode):
    from paper_accurate_fast_cheap_amd.utils.audio_stream import AudioStreamer
    from paper_accurate_fast_cheap_amd.utils.stream_pool import StreamPool
    model = _model("transducer" if mode == "rnnt_greedy_search" else "asr", True)
    kwargs = _kwargs(mode, tmp_path)
    audio = _audio(ORDER)
    pool = StreamPool(model, SLOTS, 16, mode, use_graph=False, max_step_rows=1, **kwargs)
    results, names = _serve(pool, audio, ORDER, 3)
    assert len(names) == 5 > SLOTS and set(results) == set(ORDER)             # slots were reused
    assert all(len(r["rows"]) == 1 and r["batch"] == 1 and not r["in_place"] and not r["replayed"] for r in pool.step_log)
    finals = {names[r["rows"][0][0]]: r["rows"][0][2] for r in pool.step_log if r["rows"][0][3]}
    assert finals == {"short last window": 30, "141 frames": 13, "last window full": 67, "200 frames": 8}   # (none for < ctx)
    alone = AudioStreamer(model, 1, 16, mode, **kwargs)
    tokens = 0
    for name in ORDER:
        alone.feed(audio[name])
        ref = alone.finish()
        alone.reset()
        assert _same([results[name]], ref), name
        tokens += len(ref[0].tokens)
    assert list(results["fewer frames than ctx"].tokens) == [] and tokens > 0


def _replay(model, mode, kwargs, chunk, log, feats, names):
    """pool.step_log replayed with public pieces only -> (the step outputs, {name: final result})."""
    from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer
    enc = model.encoder
    dec = CtcStreamer(BSLOTS, chunk, mode, kwargs.get("beam_size", 10), kwargs.get("context_graph"), 0, 4096)
    carries, ys, results, buf = {}, [], {}, None
    for rec in log:
        sids = [r[0] for r in rec["rows"]]
        m, batch = len(sids), rec["batch"]
        xs = torch.cat([feats[names[sid]][:, start:start + length] for sid, start, length, _ in rec["rows"]])
        xs = torch.cat([xs, xs.new_zeros(batch - m, xs.size(1), xs.size(2))])
        if rec["first"]:
            y, new = enc.forward_chunk_carry(xs, 0, None)
            dec.reset(rec["slots"])
        else:
            state = []
            for i in range(len(carries[sids[0]])):
                state.append({k: torch.cat([carries[sid][i][k] for sid in sids]
                                           + [v.new_zeros((batch - m,) + tuple(v.shape[1:]))])
                              for k, v in carries[sids[0]][i].items()})
            y, new = enc.forward_chunk_carry(xs, 0, state, in_place=rec["in_place"])
        for j, sid in enumerate(sids):
            carries[sid] = [{k: v[j:j + 1].clone() for k, v in st.items()} for st in new]
        ys.append(y[:m].clone())
        lp = model.ctc_logprobs(y)[:m]                           # (of the step's whole output, padding rows included)
        if buf is None:
            buf = lp.new_zeros(BSLOTS, chunk, lp.size(2))
        nf = [0] * BSLOTS
        for j, slot in enumerate(rec["slots"]):
            buf[slot, :lp.size(1)] = lp[j]
            nf[slot] = lp.size(1)
        dec.feed(buf, nf)
        res = dec.results()
        for (sid, _, _, final), slot in zip(rec["rows"], rec["slots"]):
            if final:
                results[names[sid]] = res[slot]
    return ys, results


BATCHED = ["short last window", "141 frames", "last window full", "200 frames"]


def _batched_run(which, use_graph, tmp_path):
    """One pool run per (model, use_graph), shared by the tests below, and its replay."""
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch
    from paper_accurate_fast_cheap_amd.utils.stream_pool import StreamPool
    key = (which, use_graph)
    if key not in _cache:
        model, chunk = (_model("asr", True), 16) if which == "fp32" else (_bf16_model(), 8)
        mode, kwargs = "ctc_prefix_beam_search", _kwargs("ctc_prefix_beam_search", tmp_path)
        audio = _audio(BATCHED)
        seen = []
        pool = StreamPool(model, BSLOTS, chunk, mode, use_graph=use_graph, on_encoder_out=lambda rec, y: seen.append(y.clone()),
                          **kwargs)
        results, names = _serve(pool, audio, BATCHED, 2)
        dt = next(model.parameters()).dtype
        feats = {name: fbank_batch(w, out_dtype=dt)[0] for name, w in audio.items()}
        with torch.no_grad():
            ys, replayed = _replay(model, mode, kwargs, chunk, pool.step_log, feats, names)
        _cache[key] = dict(model=model, chunk=chunk, log=pool.step_log, seen=seen, results=results, names=names, feats=feats,
                           ys=ys, replayed=replayed)
    return _cache[key]


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_any_batching_is_bitwise_the_replay_of_the_step_log(hip, tmp_path, which):
    run = _batched_run(which, False, tmp_path)
    log = run["log"]
    assert max(len(r["rows"]) for r in log) > 1 and any(r["batch"] > len(r["rows"]) for r in log)      # batched, and padded
    assert all(not r["in_place"] and not r["replayed"] for r in log)
    assert all(len({row[0] for row in r["rows"]}) == len(r["rows"]) for r in log)
    assert all(all(row[1] == 0 for row in r["rows"]) == r["first"] for r in log)                       # first windows apart
    if which == "bf16":
        assert run["model"].encoder._carry_last_fused                                                  # the fused chunk step
    assert len(run["seen"]) == len(run["ys"]) == len(log)
    for i, (got, want) in enumerate(zip(run["seen"], run["ys"])):
        assert _bitwise(got, want), (i, log[i])
    assert set(run["results"]) == set(run["replayed"]) == set(BATCHED)
    for name in BATCHED:
        assert _same([run["results"][name]], [run["replayed"][name]]), name
    assert sum(len(r.tokens) for r in run["results"].values()) > 0


def _lockstep_inputs(run):
    """Three equal-length streams for the lock-step stream_chunks of the same model, long enough for it to capture its graph
    (420 frames: six full windows at chunk 16): pieces of the streams' features, end to end."""
    base = torch.cat([run["feats"][name] for name in BATCHED], 1)
    return torch.cat([base[:, o:o + 420] for o in (0, 150, 300)]).contiguous()


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_replayed_steps_against_the_eager_replay_of_the_step_log(hip, tmp_path, which):
    """use_graph: the steps run in place over fixed buffers and are replayed from a captured graph from the second use of a
    batch size on.  Bitwise against the eager replay of the same log, or within twice the lock-step path's own
    replayed-against-eager difference on this model (batch compositions differ per step); both go to the parity log."""
    run = _batched_run(which, True, tmp_path)
    log = run["log"]
    assert any(r["replayed"] for r in log) and all(r["in_place"] for r in log if r["replayed"])
    window = max(r["rows"][0][2] for r in log)
    assert all(r["in_place"] == (not r["first"] and r["rows"][0][2] == window) for r in log)      # own shapes stay eager
    pool_diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(run["seen"], run["ys"]))
    bitwise = all(_bitwise(a, b) for a, b in zip(run["seen"], run["ys"]))
    enc = run["model"].encoder
    xs = _lockstep_inputs(run)
    with torch.no_grad():
        lock = float((enc.stream_chunks(xs, run["chunk"], use_graph=True).float()
                      - enc.stream_chunks(xs, run["chunk"], use_graph=False).float()).abs().max())
    print(f"stream pool {which}: replayed vs eager replay max |d| = {pool_diff:g} (bitwise: {bitwise}); lock-step stream_chunks "
          f"replayed vs eager max |d| = {lock:g}")
    parity_log.record(f"stream_pool_replayed_{which}", pool_replayed_vs_eager_max=pool_diff, bitwise=bool(bitwise),
                      lockstep_replayed_vs_eager_max=lock, bound=2.0 * lock)
    if not bitwise:
        assert pool_diff <= 2.0 * lock, (pool_diff, lock)
    else:
        for name in BATCHED:
            assert _same([run["results"][name]], [run["replayed"][name]]), name


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_every_stream_against_itself_alone(hip, tmp_path, which):
    """Under mixed batching only the GEMM tile a row lands in differs from the stream run alone: bf16 within the bounds
    test_fused_state_carry_step_serves_concurrent_streams sets (mean < 5e-3, max < 0.15); fp32 within twice the lock-step
    path's own batched-against-alone difference on this model.  Tokens are not asserted: a near tie may flip."""
    run = _batched_run(which, False, tmp_path)
    enc, chunk = run["model"].encoder, run["chunk"]
    per = {}
    for rec, y in zip(run["log"], run["seen"]):
        for j, row in enumerate(rec["rows"]):
            per.setdefault(run["names"][row[0]], []).append(y[j:j + 1])
    worst_max = worst_mean = 0.0
    with torch.no_grad():
        for name, parts in per.items():
            alone = enc.stream_chunks(run["feats"][name], chunk, use_graph=False)
            got = torch.cat(parts, 1)
            assert got.shape == alone.shape, name
            d = (got.float() - alone.float()).abs()
            worst_max, worst_mean = max(worst_max, float(d.max())), max(worst_mean, float(d.mean()))
        xs = _lockstep_inputs(run)
        both = enc.stream_chunks(xs, chunk, use_graph=False)
        lock = max(float((both[b:b + 1].float() - enc.stream_chunks(xs[b:b + 1].contiguous(), chunk, use_graph=False).float())
                         .abs().max()) for b in range(3))
    print(f"stream pool {which}: pool vs alone max |d| = {worst_max:g}, mean |d| = {worst_mean:g}; lock-step batched vs alone "
          f"max |d| = {lock:g}")
    parity_log.record(f"stream_pool_vs_alone_{which}", pool_vs_alone_max=worst_max, pool_vs_alone_mean=worst_mean,
                      lockstep_batched_vs_alone_max=lock)
    if which == "bf16":
        assert worst_mean < 5e-3 and worst_max < 0.15, (worst_mean, worst_max)
    else:
        assert worst_max <= 2.0 * lock, (worst_max, lock)


def test_errors_name_the_stream_and_the_pool_keeps_serving(hip, tmp_path):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.utils.audio_stream import AudioStreamer
    from paper_accurate_fast_cheap_amd.utils.stream_pool import StreamPool
    model = _model("asr", True)
    kwargs = _kwargs("ctc_prefix_beam_search", tmp_path)
    audio = _audio(["last window full", "141 frames"])
    pool = StreamPool(model, 2, 16, "ctc_prefix_beam_search", use_graph=False, max_step_rows=1, max_total_frames=32, **kwargs)
    a, b = pool.open(), pool.open()
    with pytest.raises(PafcError, match="pool full"):
        pool.open()
    with pytest.raises(PafcError, match="sid 9 is unknown"):
        pool.feed([9], torch.zeros(1, 10, device="cuda"))
    with pytest.raises(ValueError, match="once per feed"):
        pool.feed([a, a], torch.zeros(2, 10, device="cuda"))
    # a passes max_total_frames = 32 encoder frames with its third window; b (100 frames: 16 + 8 encoder frames) is served by
    # the same feed and by the ones after
    long, short = audio["last window full"], audio["141 frames"][:, :400 + 160 * 99].contiguous()
    half = short.size(1) // 2
    buf = torch.zeros(2, long.size(1), device="cuda")
    buf[0], buf[1, :half] = long[0], short[0, :half]
    with pytest.raises(PafcError, match=rf"sid {a} \(slot 0\).*max_total_frames = 32"):
        pool.feed([a, b], buf, [long.size(1), half])
    assert pool.active == [a, b]
    pool.feed([b], short[:, half:].contiguous())
    res_b = pool.close(b)
    alone = AudioStreamer(model, 1, 16, "ctc_prefix_beam_search", max_total_frames=32, **kwargs)
    alone.feed(short)
    assert _same([res_b], alone.finish()) and pool.truncated == []
    assert pool.active == [a]
    pool.close(a)                                                # what it had taken; the sid is listed
    assert pool.truncated == [a] and pool.active == []
    with pytest.raises(PafcError, match=rf"sid {a} was closed"):
        pool.feed([a], torch.zeros(1, 10, device="cuda"))
    with pytest.raises(PafcError, match=rf"sid {b} was closed"):
        pool.close(b)
    # the slots serve new streams as if nothing had been there
    c = pool.open()
    pool.feed([c], short[:, :half].contiguous())
    pool.feed([c], short[:, half:].contiguous())
    alone.reset()
    alone.feed(short)
    assert _same([pool.close(c)], alone.finish())


def test_a_packet_larger_than_the_ring_is_cut_and_changes_nothing(hip, tmp_path):
    """The smallest ring the scheduler takes (window + stride = 131 frames) and whole streams in one packet each: the pool cuts
    the packets against the ring, the windows wrap inside it, and the results are those of each stream alone."""
    from paper_accurate_fast_cheap_amd.utils.audio_stream import AudioStreamer
    from paper_accurate_fast_cheap_amd.utils.stream_pool import StreamPool
    model = _model("asr", True)
    kwargs = _kwargs("ctc_prefix_beam_search", tmp_path)
    names = ["short last window", "last window full"]
    audio = _audio(names)
    pool = StreamPool(model, 2, 16, "ctc_prefix_beam_search", use_graph=False, max_step_rows=1, ring_frames=131, **kwargs)
    sids = [pool.open(), pool.open()]
    width = max(w.size(1) for w in audio.values())
    buf = torch.zeros(2, width, device="cuda")
    for i, name in enumerate(names):
        buf[i, :audio[name].size(1)] = audio[name][0]
    pool.feed(sids, buf, [audio[name].size(1) for name in names])
    assert pool.fbank.frames_emitted == [286, 259] and max(pool.fbank.frames_emitted) > 2 * pool.sched.ring_frames
    got = pool.close(sids)
    alone = AudioStreamer(model, 1, 16, "ctc_prefix_beam_search", **kwargs)
    for name, res in zip(names, got):
        alone.feed(audio[name])
        assert _same([res], alone.finish()), name
        alone.reset()
