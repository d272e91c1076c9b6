"""80-bin Kaldi log-mel fbank on the MI355X, behind the call the reference makes.

Reference call sites: `compute_fbank(sample, num_mel_bins, frame_length, frame_shift, dither)`
wenet/dataset/processor.py:343-371 and `compute_feats` wenet/bin/encoder-rtf.py:558-585, both of which call
torchaudio.compliance.kaldi.fbank(waveform, num_mel_bins=..., frame_length=25, frame_shift=10, dither=...,
energy_floor=0.0, sample_frequency=16000).  `fbank()` below takes the same arguments with the same meaning and
returns the same (frames, num_mel_bins) float32 tensor -- on the device the waveform lives on.

The constant tables (povey window, DFT matrix, mel filters) are built once per device in float64 / float32 on
the host exactly as torchaudio builds them and handed to the kernel; the library itself keeps no state."""
import math
from ctypes import byref, c_int, c_long
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import _lib

_tables: Dict[Tuple[str, int], dict] = {}
_FIXED = ("fbank kernel is built for the reference's configuration: 25 ms / 10 ms frames at 16 kHz, energy_floor 0 "
          "(processor.py:363-369)")
CARRY = 560          # row length of a stream's carry (a row never holds more than 400 + 160 - 1 samples)


def mel_banks(num_bins: int, padded: int = 512, sample_freq: float = 16000.0, low_freq: float = 20.0) -> torch.Tensor:
    """(num_bins, padded/2 + 1) triangular filters in mel space, float32 arithmetic as torchaudio's get_mel_banks
    (+ its zero column for the Nyquist bin)."""
    nfft_bins = padded // 2
    high_freq = 0.5 * sample_freq
    width = sample_freq / padded
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    lo, hi = mel(low_freq), mel(high_freq)
    delta = (hi - lo) / (num_bins + 1)
    b = torch.arange(num_bins, dtype=torch.float32).unsqueeze(1)
    left, center, right = lo + b * delta, lo + (b + 1.0) * delta, lo + (b + 2.0) * delta
    melf = (1127.0 * (1.0 + width * torch.arange(nfft_bins, dtype=torch.float32) / 700.0).log()).unsqueeze(0)
    up = (melf - left) / (center - left)
    down = (right - melf) / (right - center)
    w = torch.clamp_min(torch.min(up, down), 0.0)
    return torch.nn.functional.pad(w, (0, 1))


def _get_tables(device: torch.device, num_mel_bins: int) -> dict:
    key = (str(device), num_mel_bins)
    t = _tables.get(key)
    if t is not None:
        return t
    cols = _lib.lib().pafc_fbank_tables_cols()
    n = torch.arange(400, dtype=torch.float64).unsqueeze(1)
    k = torch.arange(257, dtype=torch.float64).unsqueeze(0)
    ang = 2.0 * math.pi * n * k / 512.0
    dft = torch.zeros(400, cols, dtype=torch.float64)
    dft[:, 0:514:2] = torch.cos(ang)
    dft[:, 1:514:2] = -torch.sin(ang)
    melw = mel_banks(num_mel_bins)
    nz = melw > 0
    idx = torch.arange(257).unsqueeze(0).expand_as(melw)
    lo = torch.where(nz, idx, torch.full_like(idx, 257)).min(dim=1).values
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).max(dim=1).values
    t = dict(window=torch.hann_window(400, periodic=False, dtype=torch.float32).pow(0.85).to(device),
             dft=dft.to(torch.float32).to(device).contiguous(), melw=melw.to(device).contiguous(),
             lo=lo.to(torch.int32).to(device), hi=hi.to(torch.int32).to(device))
    _tables[key] = t
    return t


def fbank(waveform: torch.Tensor, num_mel_bins: int = 23, frame_length: float = 25.0, frame_shift: float = 10.0,
          dither: float = 0.0, energy_floor: float = 0.0, sample_frequency: float = 16000.0,
          noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """waveform: (channels, S) float tensor in int16 range ON THE GPU (channel 0 is used, as torchaudio's default
    channel=-1 -> first channel); returns (frames, num_mel_bins) float32.  dither != 0 draws standard-normal noise
    per frame sample on the device (or uses `noise` (frames, 400) if given)."""
    if (frame_length, frame_shift, sample_frequency, energy_floor) != (25.0, 10.0, 16000.0, 0.0):
        raise _lib.PafcError(_FIXED)
    if waveform.dim() != 2:
        raise _lib.PafcError("waveform must be (channels, samples)")
    _lib.require_gpu(waveform)
    L = _lib.lib()
    wave = waveform[0].to(torch.float32).contiguous()
    S = wave.numel()
    m = L.pafc_fbank_num_frames(S)
    out = torch.empty((m, num_mel_bins), dtype=torch.float32, device=wave.device)
    if m == 0:
        return out
    t = _get_tables(wave.device, num_mel_bins)
    if dither != 0.0 and noise is None:
        noise = torch.randn((m, 400), dtype=torch.float32, device=wave.device)
    if noise is not None:
        _lib.require_gpu(noise)
        if noise.shape != (m, 400) or noise.dtype != torch.float32:
            raise _lib.PafcError("noise must be float32 (frames, 400)")
    rc = L.pafc_fbank_f32(_lib.ptr(wave), S, _lib.ptr(t["window"]), _lib.ptr(t["dft"]), _lib.ptr(t["melw"]),
                          _lib.ptr(t["lo"]), _lib.ptr(t["hi"]), num_mel_bins,
                          _lib.ptr(noise if dither != 0.0 else None), float(dither), 0.97, _lib.ptr(out),
                          _lib.stream_of(wave))
    _lib.check(rc, "pafc_fbank_f32")
    return out


def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    """A (B, n) float32 GPU tensor whose rows the kernel can read where they lie: unit inner stride, any row stride >= n."""
    if x.dim() != 2:
        raise _lib.PafcError(f"{what} must be (batch, samples)")
    if not x.is_cuda:
        raise _lib.PafcError("this op runs on the MI355X only (tensor is on %s); there is no CPU fallback" % x.device)
    if x.dtype != torch.float32:
        raise _lib.PafcError(f"{what} must be float32, got {x.dtype}")
    if x.size(1) > 1 and x.stride(1) != 1 or x.size(0) > 1 and x.stride(0) < x.size(1):
        raise _lib.PafcError(f"{what}: rows must have unit inner stride and must not overlap (strides {tuple(x.stride())})")
    return x


def _ld(x: torch.Tensor) -> int:
    return x.stride(0) if x.size(0) > 1 else max(x.size(1), 1)


def fbank_batch(waveforms: torch.Tensor, lengths: Union[None, torch.Tensor, Sequence[int]] = None, num_mel_bins: int = 80,
                dither: float = 0.0, noise: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32,
                frame_length: float = 25.0, frame_shift: float = 10.0, energy_floor: float = 0.0,
                sample_frequency: float = 16000.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """fbank() of B utterances in ONE launch.  waveforms: (B, S_max) float32 in int16 range on the GPU, row b holding its
    utterance in its first lengths[b] samples (rows may be a view with unit inner stride: a slice of a wider buffer);
    lengths: int64 device tensor (B) or a Python list (copied to the device once), None = every row is S_max long.
    Returns (feats (B, T_max, num_mel_bins) in out_dtype -- float32 or bfloat16 = the float32 value rounded to nearest even --,
    feat_lengths (B) int32 on the device): row b's first feat_lengths[b] frames are bit for bit fbank() of its utterance, every
    frame behind them is 0.  dither != 0 draws (or takes as `noise`) standard-normal noise (B, T_max, 400).  Nothing here waits
    for the device."""
    if (frame_length, frame_shift, sample_frequency, energy_floor) != (25.0, 10.0, 16000.0, 0.0):
        raise _lib.PafcError(_FIXED)
    wave = _rows(waveforms, "waveforms")
    code = _lib.dtype_code(out_dtype)
    L = _lib.lib()
    B, S = wave.shape
    dev = wave.device
    T = L.pafc_fbank_num_frames(S)
    if lengths is not None:
        if not torch.is_tensor(lengths):
            lengths = torch.tensor([int(v) for v in lengths], dtype=torch.int64).to(dev)
        if lengths.dtype != torch.int64 or lengths.shape != (B,):
            raise _lib.PafcError(f"lengths must be int64 ({B},), got {lengths.dtype} {tuple(lengths.shape)}")
        _lib.require_gpu(lengths)
    out = torch.empty((B, T, num_mel_bins), dtype=out_dtype, device=dev)
    out_len = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0 or T == 0:
        return out, out_len.zero_()
    if dither != 0.0 and noise is None:
        noise = torch.randn((B, T, 400), dtype=torch.float32, device=dev)
    if noise is not None:
        _lib.require_gpu(noise)
        if noise.shape != (B, T, 400) or noise.dtype != torch.float32:
            raise _lib.PafcError(f"noise must be float32 ({B}, {T}, 400)")
    t = _get_tables(dev, num_mel_bins)
    rc = L.pafc_fbank_batch(_lib.ptr(wave), _ld(wave), _lib.ptr(lengths), B, S, _lib.ptr(t["window"]), _lib.ptr(t["dft"]),
                            _lib.ptr(t["melw"]), _lib.ptr(t["lo"]), _lib.ptr(t["hi"]), num_mel_bins,
                            _lib.ptr(noise if dither != 0.0 else None), float(dither), 0.97, _lib.ptr(out), code,
                            _lib.ptr(out_len), _lib.stream_of(wave))
    _lib.check(rc, "pafc_fbank_batch")
    return out, out_len


def stream_plan(carry_len: int, n: int) -> Tuple[int, int]:
    """(frames completed, samples carried on) when n samples arrive behind carry_len carried ones: pafc_fbank_stream_plan."""
    frames, c_next = c_long(0), c_int(0)
    _lib.check(_lib.lib().pafc_fbank_stream_plan(int(carry_len), int(n), byref(frames), byref(c_next)), "pafc_fbank_stream_plan")
    return frames.value, c_next.value


class FbankStreamer:
    """fbank of `batch_size` lock-step streams fed packet by packet.  feed(chunk (B, n)) returns the (B, f, num_mel_bins) frames
    this packet completed (f may be 0) and keeps, on the device, the samples a later frame still needs (`carry_len` of them,
    < 560).  For any cut of a stream into feeds the concatenated frames are bit for bit fbank_batch of the whole stream.
    feed_into(chunk, out, first_frame) writes the frames at out[:, first_frame:first_frame + f] instead (out: (B, >= first_frame
    + f, num_mel_bins) in out_dtype with contiguous frames; rows may be strided) and returns f.  A feed is two launches and no
    wait, and can be captured.  reset() starts new streams.  Dither is not offered on a stream."""

    def __init__(self, batch_size: int, num_mel_bins: int = 80, out_dtype: torch.dtype = torch.float32, device="cuda",
                 dither: float = 0.0):
        if dither != 0.0:
            raise _lib.PafcError("FbankStreamer: dither is not offered on a stream (dither must be 0)")
        if batch_size < 1:
            raise _lib.PafcError("FbankStreamer: batch_size must be >= 1")
        self.B, self.nmel, self.out_dtype = batch_size, num_mel_bins, out_dtype
        self._code = _lib.dtype_code(out_dtype)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PafcError("this op runs on the MI355X only (device is %s); there is no CPU fallback" % self.device)
        self._L = _lib.lib()
        self._t = _get_tables(self.device, num_mel_bins)
        self._carry = torch.zeros((batch_size, CARRY), dtype=torch.float32, device=self.device)
        self.carry_len = 0
        self.frames_emitted = 0

    def reset(self):
        self.carry_len = 0
        self.frames_emitted = 0

    def _check(self, chunk: torch.Tensor) -> Tuple[int, int]:
        chunk = _rows(chunk, "chunk")
        if chunk.size(0) != self.B or chunk.device != self._carry.device:
            raise _lib.PafcError(f"FbankStreamer.feed: the chunk must be ({self.B}, n) on {self._carry.device}")
        return stream_plan(self.carry_len, chunk.size(1))

    def feed_into(self, chunk: torch.Tensor, out: Optional[torch.Tensor], first_frame: int = 0, _plan=None) -> int:
        frames, c_next = _plan or self._check(chunk)
        n = chunk.size(1)
        if n == 0:
            return 0
        stride = 0
        if frames > 0:
            if (out is None or out.dim() != 3 or out.size(0) != self.B or out.size(2) != self.nmel or out.dtype != self.out_dtype
                    or out.device != chunk.device or first_frame < 0 or out.size(1) < first_frame + frames):
                raise _lib.PafcError(f"FbankStreamer.feed_into: out must be {self.out_dtype} ({self.B}, >= {first_frame + frames}, "
                                     f"{self.nmel}) on {chunk.device}")
            if out.stride(2) != 1 or out.stride(1) != self.nmel or (self.B > 1 and out.stride(0) < out.size(1) * self.nmel):
                raise _lib.PafcError("FbankStreamer.feed_into: the frames of a row of out must be contiguous")
            stride = out.stride(0) if self.B > 1 else out.size(1) * self.nmel
        t = self._t
        rc = self._L.pafc_fbank_stream(_lib.ptr(self._carry), self.carry_len, _lib.ptr(chunk), _ld(chunk), n, self.B,
                                       _lib.ptr(t["window"]), _lib.ptr(t["dft"]), _lib.ptr(t["melw"]), _lib.ptr(t["lo"]),
                                       _lib.ptr(t["hi"]), self.nmel, 0.0, 0.97, _lib.ptr(out if frames > 0 else None), self._code,
                                       stride, first_frame, _lib.stream_of(chunk))
        _lib.check(rc, "pafc_fbank_stream")
        self.carry_len = c_next
        self.frames_emitted += frames
        return frames

    def feed(self, chunk: torch.Tensor) -> torch.Tensor:
        plan = self._check(chunk)
        out = torch.empty((self.B, plan[0], self.nmel), dtype=self.out_dtype, device=self._carry.device)
        self.feed_into(chunk, out, 0, plan)
        return out


class FbankSlotStreamer:
    """fbank of `slots` INDEPENDENT streams fed raggedly: a call names any subset of the slots, each with its own number of new
    samples, and the frames go into a per-slot ring `ring` (slots, ring_frames, num_mel_bins): frame f of a slot's stream lies at
    ring[slot, f mod ring_frames].  feed_rows(slot_ids, chunk (R, n_max), lengths) -> frames completed per row; row i brings
    chunk[i, :lengths[i]] to slot slot_ids[i] (distinct slots; lengths None = n_max each).  One launch pair and one small upload
    of the row descriptors, no wait.  `carry_len[slot]` / `frames_emitted[slot]` mirror the device state on the host (the plan
    is pure arithmetic), reset(slot) starts a new stream in a slot.  A row may complete at most ring_frames frames per call, and
    the caller has to have consumed a ring row before the stream comes round to it again.  For any cut of a stream into feeds,
    interleaved with other streams in any slot order, its frames are bit for bit fbank_batch of its whole audio."""

    def __init__(self, slots: int, ring_frames: int, num_mel_bins: int = 80, out_dtype: torch.dtype = torch.float32, device="cuda",
                 dither: float = 0.0):
        if dither != 0.0:
            raise _lib.PafcError("FbankSlotStreamer: dither is not offered on a stream (dither must be 0)")
        if slots < 1 or ring_frames < 1:
            raise _lib.PafcError("FbankSlotStreamer: slots and ring_frames must be >= 1")
        self.S, self.ring_frames, self.nmel, self.out_dtype = slots, ring_frames, num_mel_bins, out_dtype
        self._code = _lib.dtype_code(out_dtype)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PafcError("this op runs on the MI355X only (device is %s); there is no CPU fallback" % self.device)
        self._L = _lib.lib()
        self._t = _get_tables(self.device, num_mel_bins)
        self._carry = torch.zeros((slots, CARRY), dtype=torch.float32, device=self.device)
        self.ring = torch.zeros((slots, ring_frames, num_mel_bins), dtype=out_dtype, device=self.device)
        self.carry_len = [0] * slots
        self.frames_emitted = [0] * slots

    def reset(self, slot: int):
        self.carry_len[slot] = 0
        self.frames_emitted[slot] = 0

    def feed_rows(self, slot_ids: Sequence[int], chunk: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> List[int]:
        chunk = _rows(chunk, "chunk")
        slot_ids = [int(s) for s in slot_ids]
        R, n_max = len(slot_ids), chunk.size(1)
        if R == 0:
            return []
        if chunk.size(0) != R or chunk.device != self._carry.device:
            raise _lib.PafcError(f"FbankSlotStreamer.feed_rows: the chunk must be ({R}, n_max) on {self._carry.device}")
        lengths = [n_max] * R if lengths is None else [int(v) for v in lengths]
        if len(lengths) != R or any(not 0 <= s < self.S for s in slot_ids) or len(set(slot_ids)) != R:
            raise _lib.PafcError(f"FbankSlotStreamer.feed_rows: {R} distinct slots in [0, {self.S}) and {R} lengths")
        desc, plans = [], []
        for s, n in zip(slot_ids, lengths):
            if not 0 <= n <= n_max:
                raise _lib.PafcError(f"FbankSlotStreamer.feed_rows: slot {s}: length {n} is outside [0, {n_max}]")
            frames, c_next = stream_plan(self.carry_len[s], n)
            if frames > self.ring_frames:
                raise _lib.PafcError(f"FbankSlotStreamer.feed_rows: slot {s}: {frames} frames in one call, the ring holds "
                                     f"{self.ring_frames} (cut the packet)")
            desc += [s, self.carry_len[s], n, self.frames_emitted[s]]
            plans.append((frames, c_next))
        if not any(lengths):
            return [0] * R
        host = (c_int * len(desc))(*desc)
        dev = torch.tensor(desc, dtype=torch.int32).to(self._carry.device)
        t = self._t
        rc = self._L.pafc_fbank_stream_rows(_lib.ptr(self._carry), self.S, host, _lib.ptr(dev), R, _lib.ptr(chunk), _ld(chunk), n_max,
                                            _lib.ptr(t["window"]), _lib.ptr(t["dft"]), _lib.ptr(t["melw"]), _lib.ptr(t["lo"]),
                                            _lib.ptr(t["hi"]), self.nmel, 0.0, 0.97, _lib.ptr(self.ring), self._code,
                                            self.ring_frames, _lib.stream_of(chunk))
        _lib.check(rc, "pafc_fbank_stream_rows")
        for s, n, (frames, c_next) in zip(slot_ids, lengths, plans):
            if n > 0:
                self.carry_len[s] = c_next
                self.frames_emitted[s] += frames
        return [f if n > 0 else 0 for n, (f, _) in zip(lengths, plans)]


def compute_fbank(sample: dict, num_mel_bins: int = 23, frame_length: int = 25, frame_shift: int = 10,
                  dither: float = 0.0) -> dict:
    """wenet/dataset/processor.py:343-371: {key, wav (float in [-1, 1)), sample_rate} -> adds 'feat'."""
    assert "sample_rate" in sample and "wav" in sample and "key" in sample
    waveform = sample["wav"] * (1 << 15)
    sample["feat"] = fbank(waveform, num_mel_bins=num_mel_bins, frame_length=float(frame_length),
                           frame_shift=float(frame_shift), dither=dither, energy_floor=0.0,
                           sample_frequency=float(sample["sample_rate"]))
    return sample
