"""Streaming decode driven by audio (utils.audio_stream.AudioStreamer) on the reduced streaming models of
test_ctc_stream_gpu: for any cut of the audio into packets the encoder sees bitwise the windows that the model's stream_*
function cuts out of fbank_batch of the whole audio, with the same final flags, and the results are those of that function
bit for bit."""
import random

import pytest
import torch

from tests.test_ctc_context_gpu import synthetic_graph
from tests.test_ctc_stream_gpu import _stream_model
from tests.test_fbank_gpu import _wave

pytestmark = pytest.mark.gpu
CHUNK, B = 16, 2                      # subsampling 4, right context 6: windows of 67 frames every 64
# frames -> samples: 259 = 3 * 64 + 67 frames (the last window is full), 286 frames (a last window of 30), 5 frames (< ctx)
AUDIO = {"last window full": 400 + 160 * 258, "short last window": 400 + 160 * 285 + 77, "fewer frames than ctx": 400 + 160 * 4 + 50}
_models = {}


def _model(family, causal):
    if (family, causal) not in _models:
        _models[family, causal] = _stream_model(family, causal)
    return _models[family, causal]


def _cuts(S, how):
    if how == "one feed":
        return [S]
    if how == "10240":
        return [10240] * (S // 10240) + ([S % 10240] if S % 10240 else [])
    rng, out, pos = random.Random(S), [], 0
    while pos < S:
        out.append(min(rng.randint(1, 5000), S - pos))
        pos += out[-1]
    return out


class Spy:
    """Records (input window, final flag) of every encoder step while it is installed."""

    def __init__(self, monkeypatch, enc):
        self.calls = []
        carry, look = enc.forward_chunk_carry, enc.forward_chunk_lookahead

        def spy_carry(xs, offset=0, state=None, in_place=False):
            self.calls.append((xs.clone(), None))
            return carry(xs, offset, state, in_place)

        def spy_look(xs, state=None, final=False):
            self.calls.append((xs.clone(), final))
            return look(xs, state, final=final)
        monkeypatch.setattr(enc, "forward_chunk_carry", spy_carry, raising=False)
        monkeypatch.setattr(enc, "forward_chunk_lookahead", spy_look, raising=False)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _bitwise(x, w):
    return x.shape == w.shape and x.dtype == w.dtype and torch.equal(x.contiguous().view(torch.int32), w.contiguous().view(torch.int32))


def _same(a, b):
    keys = ("tokens", "score", "times", "nbest", "nbest_scores", "nbest_times")
    return len(a) == len(b) and all([getattr(x, k) if k != "tokens" else list(x.tokens) for k in keys] ==
                                    [getattr(y, k) if k != "tokens" else list(y.tokens) for k in keys] for x, y in zip(a, b))


@pytest.mark.parametrize("mode", ["ctc_prefix_beam_search", "ctc_greedy_search", "rnnt_greedy_search"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", ["asr", "transducer"])
def test_audio_streamer_equals_the_stream_search_of_the_whole_feature_tensor(hip, tmp_path, monkeypatch, family, causal, mode):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch
    from paper_accurate_fast_cheap_amd.utils.audio_stream import AudioStreamer
    from paper_accurate_fast_cheap_amd.utils.graph_step import chunk_windows
    from tests.test_rnnt_greedy import V as VOC
    if family == "asr" and mode == "rnnt_greedy_search":
        with pytest.raises(ValueError):
            AudioStreamer(_model(family, causal), B, CHUNK, mode)
        return
    model = _model(family, causal)
    kwargs = {}
    if mode == "ctc_prefix_beam_search":
        kwargs = dict(beam_size=4, context_graph=synthetic_graph(tmp_path, 40, VOC, seed=11, context_score=2.0, pool=20)[0])
    spy = Spy(monkeypatch, model.encoder)
    tokens = 0
    for name, S in AUDIO.items():
        audio = torch.cat([_wave(S, 70 + b) for b in range(B)]).cuda()
        feats, flens = fbank_batch(audio)
        T = feats.size(1)
        starts, window, _ = chunk_windows(model.encoder.embed, CHUNK, T)
        if name == "last window full":
            assert starts[-1] + window == T
        elif name == "short last window":
            assert 0 < T - starts[-1] < window
        else:
            assert starts == []
        with torch.no_grad():
            if mode == "rnnt_greedy_search":
                ref = model.stream_greedy_search(feats, CHUNK)
            else:
                ref = model.stream_ctc_search(feats, CHUNK, mode=mode, **kwargs)
        offline = spy.take()
        want = [(feats[:, c:min(c + window, T)], None if causal else i == len(starts) - 1) for i, c in enumerate(starts)]
        assert len(offline) == len(want) and all(_bitwise(x, w) and f == g for (x, f), (w, g) in zip(offline, want))
        tokens += sum(len(r.tokens) for r in ref)
        streamer = AudioStreamer(model, B, CHUNK, mode, **kwargs)
        for how in ("one feed", "10240", "irregular"):
            committed = [[] for _ in range(B)]
            pos, ran = 0, 0
            for n in _cuts(S, how):
                part = streamer.feed(audio[:, pos:pos + n])
                pos += n
                calls = len(spy.calls)
                assert (part is None) == (calls == ran), "feed returns None exactly when no window ran"
                ran = calls
                if part is not None:
                    assert len(part) == B
                for b in range(B):                           # .committed only grows
                    now = list(streamer.committed[b])
                    assert now[:len(committed[b])] == committed[b]
                    committed[b] = now
            res = streamer.finish()
            seen = spy.take()
            # the plumbing: bitwise the offline windows, with the same final flags
            assert len(seen) == len(want), (name, how, len(seen), len(want))
            for i, ((x, f), (w, g)) in enumerate(zip(seen, want)):
                assert _bitwise(x, w) and f == g, (name, how, i)
            assert _same(res, ref), (name, how)
            for b in range(B):
                assert list(res[b].tokens)[:len(committed[b])] == committed[b]
            with pytest.raises(ValueError):
                streamer.feed(audio[:, :10])                 # finished: reset first
            streamer.reset()
    assert tokens > 0                                        # (the comparison was about something)
