"""The resampler on the GPU (include/pafc_resample.h, dataset/resample.py) against the float64 restatement tests/resample_ref.py.

Accuracy bound, derived and not measured: an output is one chain of K = span fused multiply-adds from 0.0f over float32
coefficients k_j and samples x_j, so against the float64 sum over the SAME float32 coefficients it is off by at most
gamma_K sum_j |k_j x_j| <= (K + 1) 2^-24 sum_j |k_j x_j|.

Streams: outputs are compared with resample_batch of the whole audio as integers, bit for bit.  Every operand is a slice of
a NaN-filled buffer with NaN guard rows before and after it, as tests/test_mha_band_gpu.py does, and a row's samples behind its
own length are NaN as well: a finite output proves that nothing outside the operands was read, untouched guards that nothing
outside the output was written."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import resample_ref as ref

pytestmark = pytest.mark.gpu

RATES = sorted(ref.RATES)
GUARD, PAD = 2, 8
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _signal(S, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S, dtype=torch.float32)
    return (torch.randn(S, generator=g) * 2500.0 + 600.0 * torch.sin(t * 0.05) + 37.0).round().clamp(-32768, 32767)


def _guarded(rows, width):
    """A NaN-filled (GUARD + rows + GUARD, PAD + width + PAD) buffer on the GPU and its operand slice."""
    buf = torch.full((GUARD + rows + GUARD, PAD + width + PAD), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + rows, PAD:PAD + width]


def _guards_untouched(buf, rows, width):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[GUARD:GUARD + rows, PAD:PAD + width] = False
    return bool(torch.isnan(buf[mask]).all())


def _dense_of(plan):
    """The product's compact float32 table as a dense (new, taps) float32 array."""
    dense = np.zeros((plan.new, plan.taps), dtype=np.float32)
    first, coef = plan.first.numpy(), plan.coef.numpy()
    for i in range(plan.new):
        dense[i, first[i]:first[i] + plan.span] = coef[i]
    return dense


@functools.lru_cache(maxsize=None)
def _batch_case(rate):
    """Inputs and the float64 results of one rate, computed once: (lengths, waves (B, S_max) float32 CPU with NaN behind a
    row's length, [float64 want per row], [float64 sum |k x| per row])."""
    from paper_accurate_fast_cheap_amd.dataset.resample import resample_plan
    orig, new, W, taps, _ = ref.RATES[rate]
    plan = resample_plan(rate, 16000)
    lengths = [0, 1, W, W + orig - 1, W + orig, 2 * W + orig, 4001, 3000]
    S_max = max(lengths)
    waves = torch.full((len(lengths), S_max), NAN, dtype=torch.float32)
    dense = _dense_of(plan)
    want, scale = [], []
    for b, S in enumerate(lengths):
        x = _signal(S, 100 * rate + b)
        waves[b, :S] = x
        want.append(ref.resample(x.numpy(), orig, new, dense))
        scale.append(ref.abs_sum(x.numpy(), orig, new, dense))
    return lengths, waves, want, scale


@pytest.mark.parametrize("rate", RATES)
def test_resample_batch_against_float64(hip, rate):
    from paper_accurate_fast_cheap_amd.dataset.resample import resample_batch, resample_plan
    orig, new, W, taps, span = ref.RATES[rate]
    plan = resample_plan(rate, 16000)
    lengths, waves, want, scale = _batch_case(rate)
    B, S_max = waves.shape
    N_max = ref.num_out(S_max, orig, new)
    wbuf, wop = _guarded(B, S_max)
    wop.copy_(waves)
    obuf, oop = _guarded(B, N_max)
    lbuf = torch.full((GUARD + B + GUARD,), -7, dtype=torch.int64, device="cuda")
    lens = torch.tensor(lengths, dtype=torch.int64, device="cuda")
    before = wbuf.clone()
    out, out_len = resample_batch(wop, lens, rate, 16000, out=oop, out_lengths=lbuf[GUARD:GUARD + B])
    torch.cuda.synchronize()
    assert out.data_ptr() == oop.data_ptr()
    assert torch.equal(_bits(wbuf), _bits(before))
    assert _guards_untouched(obuf, B, N_max)
    assert lbuf.cpu().tolist() == [-7] * GUARD + [ref.num_out(S, orig, new) for S in lengths] + [-7] * GUARD
    got = oop.cpu().double().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for b, S in enumerate(lengths):
        N = ref.num_out(S, orig, new)
        bound = (span + 1) * 2.0 ** -24 * scale[b]
        err = np.abs(got[b, :N] - want[b])
        if N:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (rate, S, float(err.max()))
        assert np.all(got[b, N:] == 0.0), (rate, S)               # zeros behind the row's own N
    print(f"resample_batch {rate} -> 16000 Hz: worst error / bound {worst:.3f}")
    # lengths None: every row is S_max long, and a length outside [0, S_max] is clamped
    full = waves.clone()
    full[:, :] = _signal(S_max, 7).unsqueeze(0)
    a, a_len = resample_batch(full.cuda(), None, rate, 16000)
    b_, b_len = resample_batch(full.cuda(), torch.tensor([S_max + 5] * (B - 1) + [-3], dtype=torch.int64, device="cuda"), rate, 16000)
    assert a_len.tolist() == [N_max] * B and b_len.tolist() == [N_max] * (B - 1) + [0]
    assert torch.equal(_bits(a[:-1]), _bits(b_[:-1])) and not b_[-1].any()


def _cuts(S, rng, big):
    out, pos = [], 0
    while pos < S:
        n = min(S - pos, rng.choice((0, 1, 1, 2, rng.randint(1, 60), rng.randint(1, big), rng.randint(1, big))))
        out.append(n)
        pos += n
    return out


@pytest.mark.parametrize("rate", RATES)
def test_lock_step_stream_has_the_bits_of_the_batch_for_any_cut(hip, rate):
    from paper_accurate_fast_cheap_amd.dataset.resample import ResampleStreamer, resample_batch
    orig, new, W, taps, _ = ref.RATES[rate]
    B, S = 2, 3 * taps + 2500
    audio = torch.stack([_signal(S, rate + b) for b in range(B)]).cuda()
    whole, whole_len = resample_batch(audio, None, rate, 16000)
    N = ref.num_out(S, orig, new)
    assert whole_len.tolist() == [N] * B
    st = ResampleStreamer(B, rate, 16000)
    runs = []
    for seed in (1, 1, 2):                                      # the same cut twice, then another one
        rng = random.Random(1000 * rate + seed)
        parts, pos = [], 0
        for n in _cuts(S, rng, 1500):
            buf, op = _guarded(B, n)
            op.copy_(audio[:, pos:pos + n])
            want_out = st.plan.stream_plan(st.carry_len, n)[0]
            parts.append(st.feed(op))
            assert parts[-1].shape == (B, want_out)
            assert _guards_untouched(buf, B, n)
            pos += n
            assert st.received == pos and st.emitted == sum(p.size(1) for p in parts) <= ref.num_out(pos, orig, new)
        parts.append(st.flush())                                # (flush starts new streams)
        assert (st.received, st.emitted, st.carry_len) == (0, 0, W)
        runs.append(torch.cat(parts, dim=1))
    torch.cuda.synchronize()
    for got in runs:
        assert got.shape == (B, N) and torch.equal(_bits(got), _bits(whole[:, :N]))


@pytest.mark.parametrize("rate", RATES)
def test_slot_streams_have_the_bits_of_the_batch_in_any_interleaving(hip, rate):
    from paper_accurate_fast_cheap_amd.dataset.resample import ResampleSlotStreamer, resample_batch
    orig, new, W, taps, _ = ref.RATES[rate]
    SLOTS = 4
    lens = [2 * taps + 1800, taps + 700, W + 1, 2 * taps + 1801, 5]          # five streams through three of the four slots
    S_max = max(lens)
    audio = torch.zeros(len(lens), S_max)
    for i, S in enumerate(lens):
        audio[i, :S] = _signal(S, 31 * rate + i)
    audio = audio.cuda()
    whole, whole_len = resample_batch(audio, lens, rate, 16000)
    Ns = [ref.num_out(S, orig, new) for S in lens]
    assert whole_len.tolist() == Ns

    def serve(seed):
        rng = random.Random(seed)
        st = ResampleSlotStreamer(SLOTS, rate, 16000)
        idle = 2                                                  # never named: its carry must stay as it is
        st._carry[idle] = torch.arange(st._carry.size(1), dtype=torch.float32, device="cuda") + 0.5
        idle_before = st._carry[idle].clone()
        free, pending, live, got = [3, 0, 1], list(range(len(lens))), {}, {i: [] for i in range(len(lens))}
        while pending or live:
            while pending and free:
                live[pending.pop(0)] = [free.pop(0), 0]
            names = [i for i in live if rng.random() < 0.8]
            rng.shuffle(names)                                    # any slot order
            if not names:
                continue
            ns = [min(lens[i] - live[i][1], rng.choice((0, 1, rng.randint(1, 50), rng.randint(1, 1200)))) for i in names]
            # the last samples of a stream come with final, or final comes alone in a later call, with no sample at all
            fin = [live[i][1] + n == lens[i] and (n == 0 or rng.random() < 0.5) for i, n in zip(names, ns)]
            n_max = max(ns) + 3
            buf, op = _guarded(len(names), n_max)
            for r, (i, n) in enumerate(zip(names, ns)):
                op[r, :n] = audio[i, live[i][1]:live[i][1] + n]
            out, counts = st.feed_rows([live[i][0] for i in names], op, ns, fin)
            assert _guards_untouched(buf, len(names), n_max)
            assert out.shape == (len(names), max(counts))
            for r, (i, n, f) in enumerate(zip(names, ns, fin)):
                got[i].append(out[r, :counts[r]].clone())
                live[i][1] += n
                slot = live[i][0]
                if f:
                    assert (st.received[slot], st.emitted[slot], st.carry_len[slot]) == (0, 0, W)
                    free.append(slot)                             # the slot starts a new stream without a reset() call
                    del live[i]
                else:
                    assert st.received[slot] == live[i][1] and st.carry_len[slot] <= orig + 2 * W
        torch.cuda.synchronize()
        assert torch.equal(_bits(st._carry[idle]), _bits(idle_before))
        return [torch.cat(got[i]) for i in range(len(lens))]

    a, b, c = serve(rate), serve(rate), serve(rate + 1)
    for i, N in enumerate(Ns):
        want = _bits(whole[i, :N])
        assert a[i].shape == (N,) and torch.isfinite(a[i]).all()
        assert torch.equal(_bits(a[i]), want) and torch.equal(_bits(b[i]), want) and torch.equal(_bits(c[i]), want), (rate, i)


def test_fbank_frames_of_resampled_slot_streams_are_those_of_the_batch(hip):
    """FbankSlotStreamer fed from ResampleSlotStreamer holds, per slot, the bits of fbank_batch(resample_batch(whole))."""
    from paper_accurate_fast_cheap_amd.dataset.fbank import FbankSlotStreamer, fbank_batch
    from paper_accurate_fast_cheap_amd.dataset.resample import ResampleSlotStreamer, resample_batch
    rate, SLOTS, RING = 44100, 3, 64
    lens = [26000, 9000, 17777]                                   # 0.59, 0.20 and 0.40 s: fewer frames than the ring has rows
    audio = torch.zeros(3, max(lens))
    for i, S in enumerate(lens):
        audio[i, :S] = _signal(S, 900 + i)
    audio = audio.cuda()
    feats, flens = fbank_batch(*resample_batch(audio, lens, rate, 16000))
    rs, fb = ResampleSlotStreamer(SLOTS, rate, 16000), FbankSlotStreamer(SLOTS, RING)
    slot_of, pos, rng = [2, 0, 1], [0, 0, 0], random.Random(5)
    while any(p < S for p, S in zip(pos, lens)):
        names = [i for i in range(3) if pos[i] < lens[i] and rng.random() < 0.8]
        rng.shuffle(names)
        if not names:
            continue
        ns = [min(lens[i] - pos[i], rng.randint(1, 9000)) for i in names]
        chunk = torch.zeros(len(names), max(ns), device="cuda")
        for r, (i, n) in enumerate(zip(names, ns)):
            chunk[r, :n] = audio[i, pos[i]:pos[i] + n]
            pos[i] += n
        slots = [slot_of[i] for i in names]
        out, counts = rs.feed_rows(slots, chunk, ns, [pos[i] == lens[i] for i in names])
        fb.feed_rows(slots, out, counts)
    torch.cuda.synchronize()
    want_frames = [1 + (ref.num_out(S, 441, 160) - 400) // 160 for S in lens]
    assert flens.tolist() == want_frames and max(want_frames) <= RING and min(want_frames) > 0
    assert [fb.frames_emitted[slot_of[i]] for i in range(3)] == want_frames
    for i in range(3):
        T = int(flens[i])
        assert torch.equal(_bits(fb.ring[slot_of[i], :T]), _bits(feats[i, :T])), i


class _Spy:
    """Counts ResampleStreamer / ResampleSlotStreamer constructions and pafc_resample_* calls while installed."""

    def __init__(self, monkeypatch):
        from paper_accurate_fast_cheap_amd import _lib
        from paper_accurate_fast_cheap_amd.dataset import resample
        self.seen = []
        L = _lib.lib()
        for name in ("ResampleStreamer", "ResampleSlotStreamer"):
            monkeypatch.setattr(resample, name, self._wrap(name, getattr(resample, name)))
        for name in ("pafc_resample_num_out", "pafc_resample_stream_plan", "pafc_resample_batch", "pafc_resample_rows"):
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _wrap(self, name, fn):
        def wrapped(*a, **k):
            self.seen.append(name)
            return fn(*a, **k)
        return wrapped


def _packets(S, seed, hi):
    rng, out, pos = random.Random(seed), [], 0
    while pos < S:
        out.append(min(rng.randint(1, hi), S - pos))
        pos += out[-1]
    return out


def test_audio_streamer_at_44100_equals_the_streamer_fed_the_resampled_audio(hip, monkeypatch):
    from paper_accurate_fast_cheap_amd.dataset.resample import resample_batch
    from paper_accurate_fast_cheap_amd.utils.audio_stream import AudioStreamer
    from tests.test_audio_stream_gpu import _model, _same
    model = _model("asr", True)
    B, S = 2, 127000                                              # 2.88 s: 286 frames, a short last window
    audio = torch.stack([_signal(S, 60 + b) for b in range(B)]).cuda()
    audio16, n16 = resample_batch(audio, None, 44100, 16000)
    N = int(n16[0])
    assert N == ref.num_out(S, 441, 160)
    spy = _Spy(monkeypatch)
    plain = AudioStreamer(model, B, 16, "ctc_prefix_beam_search", beam_size=4)
    assert plain.resampler is None
    plain.feed(audio16[:, :N])
    want = plain.finish()
    assert spy.seen == []                                         # at 16 kHz the resampler is not entered
    st = AudioStreamer(model, B, 16, "ctc_prefix_beam_search", beam_size=4, sample_rate=44100)
    assert "ResampleStreamer" in spy.seen
    for how in (1, 2):
        pos = 0
        for n in ([S] if how == 1 else _packets(S, 3, 30000)):
            st.feed(audio[:, pos:pos + n])
            pos += n
        got = st.finish()
        st.reset()
        assert _same(got, want), how
    assert "pafc_resample_rows" in spy.seen
    assert sum(len(r.tokens) for r in want) > 0


def test_stream_pool_at_8000_equals_the_pool_fed_the_resampled_audio(hip, monkeypatch):
    from paper_accurate_fast_cheap_amd.dataset.resample import resample_batch
    from paper_accurate_fast_cheap_amd.utils.stream_pool import StreamPool
    from tests.test_audio_stream_gpu import _model, _same
    model = _model("asr", True)
    SLOTS = 2
    lens = [23040, 11003, 17000]                                  # three streams through two slots, 8 kHz
    audio = [_signal(S, 80 + i).cuda().unsqueeze(0) for i, S in enumerate(lens)]
    audio16 = [resample_batch(a, None, 8000, 16000)[0] for a in audio]
    assert [a.size(1) for a in audio16] == [2 * S for S in lens]

    def serve(pool, streams, hi, seed):
        """Streams open as slots free up, bring irregular packets in a shuffled order and close when their audio ends."""
        rng = random.Random(seed)
        pending, live, results = list(range(len(streams))), {}, {}
        while pending or live:
            while pending and len(live) < pool.S:
                i = pending.pop(0)
                live[pool.open()] = [i, 0]
            sids = [s for s in live if rng.random() < 0.85]
            rng.shuffle(sids)
            if sids:
                ns = [min(rng.randint(1, hi), streams[live[s][0]].size(1) - live[s][1]) for s in sids]
                buf = torch.zeros(len(sids), max(ns) + 5, device="cuda")
                for r, (s, n) in enumerate(zip(sids, ns)):
                    buf[r, :n] = streams[live[s][0]][0, live[s][1]:live[s][1] + n]
                    live[s][1] += n
                pool.feed(sids, buf, ns)
            for s in [s for s in live if live[s][1] == streams[live[s][0]].size(1)][:1]:
                results[live[s][0]] = pool.close(s)
                del live[s]
        return results

    spy = _Spy(monkeypatch)
    plain = StreamPool(model, SLOTS, 16, "ctc_prefix_beam_search", beam_size=4, max_step_rows=1)
    assert plain.resampler is None
    want = serve(plain, audio16, 9000, 1)
    assert spy.seen == []                                         # at 16 kHz the resampler is not entered
    pool = StreamPool(model, SLOTS, 16, "ctc_prefix_beam_search", beam_size=4, max_step_rows=1, sample_rate=8000)
    assert "ResampleSlotStreamer" in spy.seen
    got = serve(pool, audio, 4500, 2)
    assert "pafc_resample_rows" in spy.seen
    for i in range(len(lens)):
        assert _same([got[i]], [want[i]]), i
    assert sum(len(r.tokens) for r in want.values()) > 0


def test_wrappers_name_what_is_unmet_before_any_launch(hip, monkeypatch):
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.dataset.resample import (ResampleSlotStreamer, ResampleStreamer, resample, resample_batch)
    st = ResampleSlotStreamer(3, 8000, 16000)
    ls = ResampleStreamer(2, 8000, 16000)
    launches = []
    L = _lib.lib()
    for name in ("pafc_resample_batch", "pafc_resample_rows"):
        monkeypatch.setattr(L, name, lambda *a, _n=name: launches.append(_n) or 0)
    x = torch.zeros(2, 100, device="cuda")
    wide = torch.zeros(1, 300, device="cuda")
    overlapping = wide.as_strided((2, 100), (50, 1))
    with pytest.raises(PafcError, match="MI355X only"):
        resample_batch(x.cpu(), None, 8000, 16000)
    with pytest.raises(PafcError, match="float32"):
        resample_batch(x.double(), None, 8000, 16000)
    with pytest.raises(PafcError, match="overlap"):
        resample_batch(overlapping, None, 8000, 16000)
    with pytest.raises(PafcError, match="lengths"):
        resample_batch(x, torch.zeros(2, dtype=torch.int32, device="cuda"), 8000, 16000)
    with pytest.raises(PafcError, match="unsupported ratio"):
        resample_batch(x, None, 15999, 16000)
    with pytest.raises(PafcError, match="unsupported ratio"):
        resample_batch(x, None, 400000, 16000)
    with pytest.raises(PafcError, match="MI355X only"):
        st.feed_rows([0, 1], x.cpu())
    with pytest.raises(PafcError, match="float32"):
        st.feed_rows([0, 1], x.double())
    with pytest.raises(PafcError, match="overlap"):
        st.feed_rows([0, 1], overlapping)
    with pytest.raises(PafcError, match="distinct slots"):
        st.feed_rows([1, 1], x)
    with pytest.raises(PafcError, match="distinct slots"):
        st.feed_rows([0, 3], x)
    for bad in (-1, 101):
        with pytest.raises(PafcError, match=r"outside \[0, 100\]"):
            st.feed_rows([0, 1], x, [5, bad])
    with pytest.raises(PafcError, match="float32"):
        ls.feed(x.double())
    with pytest.raises(PafcError):
        ls.feed(x[:1])
    with pytest.raises(PafcError, match="unsupported ratio"):
        ResampleStreamer(2, 15999, 16000)
    with pytest.raises(PafcError, match="nothing to resample"):
        ResampleSlotStreamer(2, 16000, 16000)
    assert launches == []
    assert st.received == [0, 0, 0] and st.emitted == [0, 0, 0]   # a refused feed changes nothing
    # the reference's processor: a no-op when the rates agree
    sample = {"key": "k", "wav": x, "sample_rate": 16000}
    assert resample(sample)["wav"] is x and launches == []
    monkeypatch.undo()
    sample = {"key": "k", "wav": x, "sample_rate": 8000}
    out = resample(sample)
    assert out["sample_rate"] == 16000 and out["wav"].shape == (2, 200) and not out["wav"].any()
    # the library's own answer to a ratio outside its limits and to rows shorter than their samples: an error code, no launch
    first, coef = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, 13, device="cuda")
    o = torch.zeros(2, 200, device="cuda")
    p = _lib.ptr
    assert L.pafc_resample_batch(p(x), 100, None, 2, 100, 5000, 1, 7, p(first), p(coef), 13, p(o), 200, None, None) == -7
    assert L.pafc_resample_batch(p(x), 100, None, 2, 100, 25, 1, 152, p(first), p(coef), 303, p(o), 200, None, None) == -7
    assert L.pafc_resample_batch(p(x), 50, None, 2, 100, 1, 2, 7, p(first), p(coef), 13, p(o), 200, None, None) == -2
    torch.cuda.synchronize()
