"""Sample-rate conversion on the MI355X, in front of the fbank: any rate in, 16 kHz out, for batches and for streams.

Reference call site: the `resample` processor, wenet/dataset/processor.py:294-313, which runs
torchaudio.transforms.Resample(orig_freq, new_freq) -- sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99 -- before
compute_fbank.  The filter is restated here from that definition (torchaudio is not a dependency): with g = gcd(f_in, f_out),
orig = f_in / g, new = f_out / g, base = min(orig, new) * 0.99 and W = ceil(6 orig / base) it has `new` phases of 2 W + orig
taps, built in float64 and rounded once to float32.  Every tap the definition clamps is exactly zero in float32, so the kernel
gets a compact table: per phase the first kept tap and `span` taps from there.

An output sample is one fma chain over those taps in one device function, whatever the entry point, so resample_batch of a
whole recording, ResampleStreamer fed any cut of it and ResampleSlotStreamer fed it raggedly among other streams give the
same bits.  A stream releases outputs in whole frames of `new` samples, frame m once m orig + W + orig samples have arrived
(latency W + orig input samples), and keeps the samples a later frame still needs in a carry on the device; the plan is host
integer arithmetic (pafc_resample_stream_plan), nothing is read back."""
import math
from ctypes import byref, c_int, c_long
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import _lib
from .fbank import _ld, _rows

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
# The library's limits (include/pafc_resample.h, csrc/resample_host.h), restated so that a ratio outside them is named before
# its table is built -- 15 999 -> 16 000 Hz would be 16 000 phases of 48 000 taps; the entry points check them again.
MAX_CARRY = 4096            # PAFC_RESAMPLE_MAX_CARRY
_TILE, _LDS_CAP = 1024, 64 * 1024
_plans: Dict[Tuple[int, int], "ResamplePlan"] = {}


class ResamplePlan:
    """The conversion orig_freq -> new_freq: orig, new, W, taps = 2 W + orig, span, and the compact float32 table on the
    host (`first` (new) int32, `coef` (new, span)); on_device(device) -> (first, coef) there, uploaded once per device."""

    def __init__(self, orig_freq: int, new_freq: int):
        for name, f in (("orig_freq", orig_freq), ("new_freq", new_freq)):
            if isinstance(f, bool) or int(f) != f or f <= 0:
                raise _lib.PafcError(f"resample: {name} must be a positive whole number of Hz, got {f!r}")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        g = math.gcd(self.orig_freq, self.new_freq)
        self.orig, self.new = self.orig_freq // g, self.new_freq // g
        base = min(self.orig, self.new) * ROLLOFF
        self.W = int(math.ceil(LOWPASS_FILTER_WIDTH * self.orig / base))
        self.taps = 2 * self.W + self.orig
        what = f"resample {self.orig_freq} -> {self.new_freq} Hz (ratio {self.orig} / {self.new})"
        if self.taps > MAX_CARRY or self.new * self.taps > (1 << 24):
            raise _lib.PafcError(f"{what}: unsupported ratio, a stream's carry of orig + 2 W = {self.taps} samples must be <= "
                                 f"{MAX_CARRY} and the filter of {self.new} x {self.taps} taps <= 2^24")
        dense = self.dense_table(self.orig, self.new, self.W).to(torch.float32)
        idx = torch.arange(self.taps).unsqueeze(0).expand_as(dense)
        nz = dense != 0
        lo = torch.where(nz, idx, torch.full_like(idx, self.taps)).min(dim=1).values
        hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).max(dim=1).values
        self.span = int((hi - lo).max())
        first = torch.minimum(lo, torch.full_like(lo, self.taps - self.span))
        self.first = first.to(torch.int32).contiguous()
        self.coef = torch.gather(dense, 1, first.unsqueeze(1) + torch.arange(self.span).unsqueeze(0)).contiguous()
        rows = min(self.new, _TILE)
        in_span = ((self.new + _TILE - 2) // self.new) * self.orig + self.taps
        if 4 * rows * (self.span | 1) > _LDS_CAP or 4 * in_span > _LDS_CAP:
            raise _lib.PafcError(f"{what}: unsupported ratio, a block's share of the table ({4 * rows * (self.span | 1)} bytes) "
                                 f"and its input span ({4 * in_span} bytes) must each fit {_LDS_CAP} bytes of LDS")
        self._dev: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}

    @staticmethod
    def dense_table(orig: int, new: int, W: int) -> torch.Tensor:
        """(new, 2 W + orig) float64: k[i][j] = sinc(t) cos^2(pi t / 2 L) base / orig, t = clamp((-i / new + (j - W) / orig) base)."""
        L = LOWPASS_FILTER_WIDTH
        base = min(orig, new) * ROLLOFF
        i = torch.arange(new, dtype=torch.float64).unsqueeze(1)
        j = torch.arange(2 * W + orig, dtype=torch.float64).unsqueeze(0)
        t = ((-i / new + (j - W) / orig) * base).clamp(-L, L)
        pt = math.pi * t
        sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(pt) / torch.where(t == 0, torch.ones_like(t), pt))
        return sinc * torch.cos(pt / (2 * L)) ** 2 * (base / orig)

    def on_device(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        key = str(torch.device(device))
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = (self.first.to(device), self.coef.to(device))
        return t

    def num_out(self, n_in: int) -> int:
        return _lib.lib().pafc_resample_num_out(int(n_in), self.orig, self.new)

    def stream_plan(self, carry_len: int, n: int) -> Tuple[int, int]:
        """(outputs released, samples carried on) when n samples arrive behind carry_len carried ones."""
        n_out, c_next = c_long(0), c_int(0)
        _lib.check(_lib.lib().pafc_resample_stream_plan(self.orig, self.new, self.W, int(carry_len), int(n), byref(n_out),
                                                        byref(c_next)), "pafc_resample_stream_plan")
        return n_out.value, c_next.value


def resample_plan(orig_freq: int, new_freq: int = 16000) -> ResamplePlan:
    """The cached plan of a conversion (tables are built once per pair of rates and uploaded once per device)."""
    key = (orig_freq, new_freq)
    p = _plans.get(key)
    if p is None:
        p = _plans[key] = ResamplePlan(orig_freq, new_freq)
    return p


def resample_batch(waveforms: torch.Tensor, lengths: Union[None, torch.Tensor, Sequence[int]] = None, orig_freq: int = 16000,
                   new_freq: int = 16000, out: Optional[torch.Tensor] = None,
                   out_lengths: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """B utterances from orig_freq to new_freq in ONE launch.  waveforms: (B, S_max) float32 on the GPU, row b holding its
    utterance in its first lengths[b] samples (rows may be a view with unit inner stride); lengths: int64 device tensor (B) or a
    Python list (copied to the device once), None = every row is S_max long.  Returns (out (B, N_max) float32, out_lengths (B)
    int64 on the device): row b's first out_lengths[b] = ceil(new S_b / orig) samples are its resampled utterance, zeros behind
    them -- what fbank_batch(out, out_lengths) takes, with no host read in between.  `out` / `out_lengths`: write there instead
    ((B, >= N_max) float32 with unit inner stride; (B) int64).  Equal rates return the arguments as they are, as torchaudio
    does.  Nothing here waits for the device."""
    wave = _rows(waveforms, "waveforms")
    B, S = wave.shape
    dev = wave.device
    if lengths is not None:
        if not torch.is_tensor(lengths):
            lengths = torch.tensor([int(v) for v in lengths], dtype=torch.int64).to(dev)
        if lengths.dtype != torch.int64 or lengths.shape != (B,):
            raise _lib.PafcError(f"lengths must be int64 ({B},), got {lengths.dtype} {tuple(lengths.shape)}")
        _lib.require_gpu(lengths)
    if orig_freq == new_freq:
        if lengths is None:
            lengths = torch.full((B,), S, dtype=torch.int64, device=dev)
        return wave, lengths
    plan = resample_plan(orig_freq, new_freq)
    L = _lib.lib()
    N = plan.num_out(S)
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=dev)
    else:
        out = _rows(out, "out")
        if out.size(0) != B or out.size(1) < N or out.device != dev:
            raise _lib.PafcError(f"out must be float32 ({B}, >= {N}) on {dev}")
    if out_lengths is None:
        out_lengths = torch.empty((B,), dtype=torch.int64, device=dev)
    else:
        _lib.require_gpu(out_lengths)
        if out_lengths.dtype != torch.int64 or out_lengths.shape != (B,) or out_lengths.device != dev:
            raise _lib.PafcError(f"out_lengths must be int64 ({B},) on {dev}")
    if B == 0 or N == 0:
        return out, out_lengths.zero_()
    first, coef = plan.on_device(dev)
    rc = L.pafc_resample_batch(_lib.ptr(wave), _ld(wave), _lib.ptr(lengths), B, S, plan.orig, plan.new, plan.W, _lib.ptr(first),
                               _lib.ptr(coef), plan.span, _lib.ptr(out), _ld(out), _lib.ptr(out_lengths), _lib.stream_of(wave))
    _lib.check(rc, "pafc_resample_batch")
    return out, out_lengths


class ResampleSlotStreamer:
    """Resampling of `slots` INDEPENDENT streams fed raggedly.  feed_rows(slot_ids, chunk (R, n_max), lengths, final) ->
    (out (R, width) float32, counts): row i brings chunk[i, :lengths[i]] (input rate) to slot slot_ids[i] (distinct slots;
    lengths None = n_max each) and out[i, :counts[i]] are the output samples that completes; what lies behind counts[i] in a
    row is not defined.  final (one bool, or one per row) ends the row's stream with this packet: the outputs that were
    waiting for later samples are computed with zeros behind the last one, so that the stream has produced ceil(new S / orig)
    in all, and the slot starts a new stream.  chunk None is an empty packet for every row (a pure flush).  One launch pair and
    one small upload of the row descriptors, no wait.  `carry_len[slot]`, `received[slot]`, `emitted[slot]` mirror the device
    state on the host; reset(slot) starts a new stream in a slot.  For any cut of a stream into feeds, interleaved with other
    streams in any slot order, its outputs are bit for bit resample_batch of its whole audio."""

    def __init__(self, slots: int, orig_freq: int, new_freq: int = 16000, device="cuda"):
        if slots < 1:
            raise _lib.PafcError("ResampleSlotStreamer: slots must be >= 1")
        if orig_freq == new_freq:
            raise _lib.PafcError("ResampleSlotStreamer: the rates agree, there is nothing to resample")
        self.plan = resample_plan(orig_freq, new_freq)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PafcError("this op runs on the MI355X only (device is %s); there is no CPU fallback" % self.device)
        self.S = slots
        self._L = _lib.lib()
        self._first, self._coef = self.plan.on_device(self.device)
        self._carry = torch.zeros((slots, self.plan.taps), dtype=torch.float32, device=self.device)
        self.carry_len = [self.plan.W] * slots
        self.received = [0] * slots
        self.emitted = [0] * slots

    def reset(self, slot: int):
        """A new stream in `slot`: its carry is the left padding, W zeros."""
        self._carry[slot, :self.plan.W].zero_()
        self.carry_len[slot] = self.plan.W
        self.received[slot] = 0
        self.emitted[slot] = 0

    def plan_rows(self, slot_ids: Sequence[int], lengths: Sequence[int], final) -> List[Tuple[int, int]]:
        """[(outputs, samples carried on)] the rows of a feed would give; changes nothing."""
        out = []
        for s, n, fin in zip(slot_ids, lengths, final):
            if fin:
                out.append((self.plan.num_out(self.received[s] + n) - self.emitted[s], 0))
            else:
                out.append(self.plan.stream_plan(self.carry_len[s], n))
        return out

    def feed_rows(self, slot_ids: Sequence[int], chunk: Optional[torch.Tensor], lengths: Optional[Sequence[int]] = None,
                  final: Union[bool, Sequence[bool]] = False) -> Tuple[torch.Tensor, List[int]]:
        who = "ResampleSlotStreamer.feed_rows"
        slot_ids = [int(s) for s in slot_ids]
        R = len(slot_ids)
        if chunk is not None:
            chunk = _rows(chunk, "chunk")
            if chunk.size(0) != R or chunk.device != self._carry.device:
                raise _lib.PafcError(f"{who}: the chunk must be ({R}, n_max) on {self._carry.device}")
        n_max = chunk.size(1) if chunk is not None else 0
        lengths = [n_max] * R if lengths is None else [int(v) for v in lengths]
        final = [bool(final)] * R if isinstance(final, bool) else [bool(f) for f in final]
        if len(lengths) != R or len(final) != R or any(not 0 <= s < self.S for s in slot_ids) or len(set(slot_ids)) != R:
            raise _lib.PafcError(f"{who}: {R} distinct slots in [0, {self.S}), {R} lengths and {R} final flags")
        for s, n in zip(slot_ids, lengths):
            if not 0 <= n <= n_max:
                raise _lib.PafcError(f"{who}: slot {s}: length {n} is outside [0, {n_max}]")
        plans = self.plan_rows(slot_ids, lengths, final)
        width = max([p[0] for p in plans], default=0)
        out = torch.empty((R, width), dtype=torch.float32, device=self._carry.device)
        if any(n > 0 or p[0] > 0 for n, p in zip(lengths, plans)):
            desc = []
            for s, n, (n_out, c_next) in zip(slot_ids, lengths, plans):
                desc += [s, self.carry_len[s], n, n_out, c_next]
            host = (c_int * len(desc))(*desc)
            dev = torch.tensor(desc, dtype=torch.int32).to(self._carry.device)
            rc = self._L.pafc_resample_rows(_lib.ptr(self._carry), self._carry.stride(0), self.S, host, _lib.ptr(dev), R,
                                            _lib.ptr(chunk), _ld(chunk) if chunk is not None else 0, n_max, self.plan.orig,
                                            self.plan.new, self.plan.W, _lib.ptr(self._first), _lib.ptr(self._coef), self.plan.span,
                                            _lib.ptr(out), max(width, 1), _lib.stream_of(self._carry))
            _lib.check(rc, "pafc_resample_rows")
        for s, n, fin, (n_out, c_next) in zip(slot_ids, lengths, final, plans):
            if fin:
                self.reset(s)
            else:
                self.carry_len[s] = c_next
                self.received[s] += n
                self.emitted[s] += n_out
        return out, [p[0] for p in plans]


class ResampleStreamer:
    """Resampling of `batch_size` lock-step streams fed packet by packet: feed(chunk (B, n) at orig_freq) returns the
    (B, n_out) samples at new_freq this packet completes (n_out may be 0), flush() the last ones of the streams -- computed
    with zeros behind the last sample -- and starts new streams, reset() starts new streams and drops what was held.  For any
    cut of a stream into feeds, the outputs followed by flush() are bit for bit resample_batch of the whole.  A feed is two
    launches and one small upload, no wait.  `received`, `emitted`: samples in and out since the streams began."""

    def __init__(self, batch_size: int, orig_freq: int, new_freq: int = 16000, device="cuda"):
        if batch_size < 1:
            raise _lib.PafcError("ResampleStreamer: batch_size must be >= 1")
        if orig_freq == new_freq:
            raise _lib.PafcError("ResampleStreamer: the rates agree, there is nothing to resample")
        self.B = batch_size
        self._rows = ResampleSlotStreamer(batch_size, orig_freq, new_freq, device)
        self.plan = self._rows.plan
        self._ids = list(range(batch_size))

    @property
    def carry_len(self) -> int:
        return self._rows.carry_len[0]

    @property
    def received(self) -> int:
        return self._rows.received[0]

    @property
    def emitted(self) -> int:
        return self._rows.emitted[0]

    def reset(self):
        self._rows._carry[:, :self.plan.W].zero_()
        for b in self._ids:
            self._rows.carry_len[b], self._rows.received[b], self._rows.emitted[b] = self.plan.W, 0, 0

    def feed(self, chunk: torch.Tensor) -> torch.Tensor:
        if chunk.dim() != 2 or chunk.size(0) != self.B:
            raise _lib.PafcError(f"ResampleStreamer.feed: the chunk must be ({self.B}, n)")
        return self._rows.feed_rows(self._ids, chunk)[0]

    def flush(self) -> torch.Tensor:
        return self._rows.feed_rows(self._ids, None, None, final=True)[0]


def resample(sample: dict, resample_rate: int = 16000) -> dict:
    """wenet/dataset/processor.py:294-313: {key, wav (channels, S) float32 on the GPU, sample_rate} -> wav at resample_rate.
    In place; nothing happens when the rates agree."""
    assert "sample_rate" in sample and "wav" in sample
    sample_rate = sample["sample_rate"]
    if sample_rate != resample_rate:
        sample["sample_rate"] = resample_rate
        sample["wav"] = resample_batch(sample["wav"], None, sample_rate, resample_rate)[0]
    return sample
