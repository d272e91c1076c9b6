"""Streaming decode driven by AUDIO: packets of samples for B lock-step streams in, tokens out.

FbankStreamer turns the packets into feature frames appended to a device buffer, WindowRelease decides which encoder windows
of forward_chunk_by_chunk those frames complete, each window goes through the encoder with carried state and its output
frames into the search's streamer -- the same sequence of encoder and decoder calls that ASRModel.stream_ctc_search /
Transducer.stream_greedy_search make on the finished feature tensor of the whole stream, for any cut of the audio."""
from typing import Callable, List, Optional, Tuple

import torch

from .graph_step import chunk_windows

MODES = ("ctc_greedy_search", "ctc_prefix_beam_search", "rnnt_greedy_search")


class WindowRelease:
    """Which windows of forward_chunk_by_chunk can run as the frames of a stream arrive (pure host arithmetic).

    Window i starts at frame i * stride.  push(frames) releases it, as (start, window, False), once
    T >= i * stride + stride + ctx frames exist: it is full, and the next window has its first output frame, so this one is
    not the last.  That waits `sub` frames longer than the window itself needs.  finish() releases what is left, with
    final=True: the held full window or a shorter last one of ctx <= T - start < window frames; nothing when T < ctx.  Over a
    stream the released list equals the windows of chunk_windows(embed, chunk, T) on the whole, final on the last."""

    def __init__(self, embed, decoding_chunk_size: int):
        if decoding_chunk_size <= 0:
            raise ValueError("WindowRelease: decoding_chunk_size must be > 0 (a chunked stream)")
        _, self.window, self.stride = chunk_windows(embed, decoding_chunk_size, 0)
        self.ctx = embed.right_context + 1
        self.reset()

    def reset(self):
        self.T = 0            # frames so far
        self.start = 0        # first frame of the next window to release
        self.finished = False

    def push(self, frames: int) -> List[Tuple[int, int, bool]]:
        assert frames >= 0 and not self.finished
        self.T += frames
        out = []
        while self.T >= self.start + self.stride + self.ctx:
            out.append((self.start, self.window, False))
            self.start += self.stride
        return out

    def finish(self) -> List[Tuple[int, int, bool]]:
        assert not self.finished
        self.finished = True
        left = self.T - self.start
        if left < self.ctx:
            return []
        out = [(self.start, min(left, self.window), True)]
        self.start += self.stride
        return out


class AudioStreamer:
    """Streaming search of `batch_size` lock-step audio streams.  mode: ctc_greedy_search / ctc_prefix_beam_search (any
    ASRModel with a streamable encoder) or rnnt_greedy_search (a Transducer); the keyword arguments are those
    stream_ctc_search (beam_size, context_graph, blank_id, blank_penalty, on_partial, max_total_frames) and stream_greedy_search
    (n_steps, on_tokens) take.  max_total_frames defaults to 4096 encoder frames per stream between resets (the length of a
    stream is not known in advance).

    feed(samples (B, n) float32 in int16 range, on the model's device) runs every window the samples complete and returns the
    latest partial result -- CTC: the partial DecodeResults of CtcStreamer.feed, as on_partial sees them; RNN-T: the new tokens
    per row of the windows this feed ran -- or None if no window ran.  finish() runs the last window and returns the final
    List[DecodeResult]: exactly what the model's stream_* function returns for fbank_batch of the whole audio.  `.committed`:
    per row the tokens that can no longer change (it only grows).  reset() starts new streams.

    sample_rate: the rate of the samples feed() takes.  At another rate than 16 000 Hz a dataset.resample.ResampleStreamer turns
    every packet into 16 kHz samples on the device first and finish() flushes it into the fbank before the last window: the
    results are exactly those of an AudioStreamer fed resample_batch of the whole audio.  At 16 000 none is constructed."""

    def __init__(self, model: torch.nn.Module, batch_size: int, decoding_chunk_size: int, mode: str = "ctc_prefix_beam_search",
                 beam_size: int = 10, context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0,
                 on_partial: Optional[Callable] = None, max_total_frames: int = 4096, n_steps: int = 64,
                 on_tokens: Optional[Callable] = None, num_mel_bins: int = 80, sample_rate: int = 16000):
        from ..dataset.fbank import FbankStreamer
        if mode not in MODES:
            raise ValueError(f"AudioStreamer: mode must be one of {MODES}, got {mode!r}")
        # the checks of the window walk itself (chunk size, streamable pre-norm uni-directional encoder), on an empty stream
        p = next(model.parameters())
        list(model._stream_windows(torch.empty(batch_size, 0, num_mel_bins, device=p.device, dtype=p.dtype), decoding_chunk_size,
                                   "AudioStreamer"))
        self.model, self.B, self.chunk, self.mode = model, batch_size, decoding_chunk_size, mode
        enc = model.encoder
        self._lookahead = any(l.conv_module is not None and l.conv_module.lorder == 0 for l in enc.encoders)
        self.plan = WindowRelease(enc.embed, decoding_chunk_size)
        self.fbank = FbankStreamer(batch_size, num_mel_bins, p.dtype, p.device)
        self.sample_rate = sample_rate
        self.resampler = None
        if sample_rate != 16000:
            from ..dataset import resample as _resample
            self.resampler = _resample.ResampleStreamer(batch_size, sample_rate, 16000, p.device)
        self._buf = torch.empty(batch_size, 2 * (self.plan.window + self.plan.stride), num_mel_bins, dtype=p.dtype, device=p.device)
        self._base = 0                  # absolute frame of _buf[:, 0]
        self._held = 0                  # frames in _buf
        self._state = None
        self._windows = 0
        self._blank_id, self._blank_penalty = blank_id, blank_penalty
        self._on_partial, self._on_tokens = on_partial, on_tokens
        if mode == "rnnt_greedy_search":
            from ..transducer.search.greedy_search import GreedyStreamer
            if not hasattr(model, "predictor") or not hasattr(model, "joint"):
                raise ValueError("AudioStreamer: rnnt_greedy_search needs a Transducer")
            self.decoder = GreedyStreamer(model, batch_size, decoding_chunk_size, n_steps)
        else:
            from ..transformer.search import CtcStreamer
            self.decoder = CtcStreamer(batch_size, decoding_chunk_size, mode, beam_size, context_graph, blank_id, max_total_frames)

    @property
    def committed(self) -> List[List[int]]:
        if self.mode == "rnnt_greedy_search":       # a greedy token is final when it is emitted
            return [list(h) for h in self.decoder._hyps]
        return self.decoder.committed

    def reset(self):
        self.fbank.reset()
        if self.resampler is not None:
            self.resampler.reset()
        self.plan.reset()
        self.decoder.reset()
        self._base = self._held = self._windows = 0
        self._state = None

    def _run(self, windows):
        enc, last = self.model.encoder, None
        for start, length, final in windows:
            xs = self._buf[:, start - self._base:start - self._base + length]
            if self._lookahead:
                y, self._state = enc.forward_chunk_lookahead(xs, self._state, final=final)
            else:
                y, self._state = enc.forward_chunk_carry(xs, 0, self._state)
            i, self._windows = self._windows, self._windows + 1
            if self.mode == "rnnt_greedy_search":
                new: List[List[int]] = [[] for _ in range(self.B)]
                for a in range(0, y.size(1), self.chunk):       # (the final drain of the look-ahead emits more frames)
                    for b, tk in enumerate(self.decoder.feed(y[:, a:a + self.chunk])):
                        new[b] += tk
                if self._on_tokens is not None:
                    self._on_tokens(i, new)
                last = new if last is None else [o + n for o, n in zip(last, new)]
            else:
                partial = None                                  # (a window may come without output frames)
                for a in range(0, y.size(1), self.chunk):
                    partial = self.decoder.feed(self.model.ctc_logprobs(y[:, a:a + self.chunk], self._blank_penalty,
                                                                        self._blank_id))
                last = partial if partial is not None else self.decoder.partials()
                if self._on_partial is not None:
                    self._on_partial(i, last, [list(c) for c in self.decoder.committed])
        return last

    def _drop_consumed(self):
        """Frames before the next window's start are done with: move the tail (< window + subsampling frames) to the front."""
        off = min(self.plan.start - self._base, self._held)
        if off <= 0:
            return
        keep = self._held - off
        if keep > 0:
            tail = self._buf[:, off:self._held].clone()         # source and destination may overlap: through a temporary
            self._buf[:, :keep] = tail
        self._base, self._held = self._base + off, keep

    @torch.no_grad()
    def feed(self, samples: torch.Tensor):
        if self.plan.finished:
            raise ValueError("AudioStreamer.feed: the streams were finished; reset() starts new ones")
        if self.resampler is not None:
            samples = self.resampler.feed(samples)
        return self._feed_16k(samples)

    def _feed_16k(self, samples: torch.Tensor):
        from ..dataset.fbank import stream_plan
        frames, _ = stream_plan(self.fbank.carry_len, samples.size(1) if samples.dim() == 2 else 0)
        need = self._held + frames
        if need > self._buf.size(1):                            # one packet may bring any number of frames
            grown = self._buf.new_empty(self.B, max(need, 2 * self._buf.size(1)), self._buf.size(2))
            grown[:, :self._held] = self._buf[:, :self._held]
            self._buf = grown
        got = self.fbank.feed_into(samples, self._buf, self._held)
        self._held += got
        last = self._run(self.plan.push(got))
        self._drop_consumed()
        return last

    @torch.no_grad()
    def finish(self):
        if self.resampler is not None and not self.plan.finished:
            self._feed_16k(self.resampler.flush())          # the outputs that were waiting for samples behind the last one
        self._run(self.plan.finish())
        self._drop_consumed()
        return self.decoder.results()
