"""Streaming decode of INDEPENDENT audio streams out of a pool of slots: sessions open and close at any moment and bring
packets of any size, and every step batches the streams that happen to have an encoder window ready.

The pieces are the lock-step ones, composed: FbankSlotStreamer turns a ragged feed into frames in a per-slot ring, a
WindowRelease per slot decides which windows of forward_chunk_by_chunk those frames complete, the carried encoder state of
the streams of a step is gathered out of per-slot storage into a dense batch and scattered back by one launch each
(hip_ops.RowsTable), the step is the same forward_chunk_carry call the lock-step paths make, and its output rows go into ONE
CtcStreamer / GreedyStreamer of `slots` rows, in which a stream that sat the step out takes nframes = 0.

PoolScheduler is the host part -- slots, packet cuts against the ring, rounds, steps, buckets -- and runs without a GPU."""
from collections import deque, namedtuple
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import graph_step
from .audio_stream import MODES, WindowRelease

WIN, SHIFT = 400, 160        # fbank frame geometry (include/pafc_fbank.h)

Row = namedtuple("Row", "sid slot start length final")
Step = namedtuple("Step", "rows first batch")     # batch: rows after padding; first: the rows' streams start here (no state)


def _frames(c: int, n: int) -> Tuple[int, int]:
    """pafc_fbank_stream_plan: c carried samples + n new -> (frames completed, samples carried on)."""
    f = 0 if c + n < WIN else 1 + (c + n - WIN) // SHIFT
    return f, c + n - SHIFT * f


def _pool_error(msg: str):
    from .._lib import PafcError
    return PafcError(msg)


class _Slot:
    def __init__(self, embed, chunk):
        self.plan = WindowRelease(embed, chunk)
        self.sid: Optional[int] = None
        self.clear()

    def clear(self):
        self.plan.reset()
        self.carry_len = 0          # samples the fbank carries
        self.frames = 0             # frames the fbank has written
        self.consumed = 0           # frames before this one are no longer needed
        self.queue = deque()        # released windows that have not run
        self.closing = False


class PoolScheduler:
    """The host side of StreamPool (pure arithmetic, as WindowRelease).

    open() -> sid (sids count up and are never reused; the lowest free slot is taken) or PafcError("pool full");
    cut(left) takes, for every stream with samples left, as many as its slot's ring has room for the frames of -- a packet
    larger than the free ring is split, the rest waits for the rounds that consume frames --, pushes the frames into the slot's
    WindowRelease and returns the pieces [(sid, slot, offset, n, carried, first_frame)];
    next_round() -> the steps that run at most ONE released window per slot (the windows of a stream are sequential): first
    windows of streams (they run without state) apart from the others, a shorter last window with those of its own length,
    each group cut into steps of at most max_step_rows rows; a step of full windows is padded to the next bucket (the powers
    of two up to `slots`, and `slots`).  close(sids) releases what is left of those streams into their queues, release(sid)
    frees the slot."""

    def __init__(self, embed, slots: int, decoding_chunk_size: int, ring_frames: Optional[int] = None,
                 max_step_rows: Optional[int] = None):
        if slots < 1:
            raise ValueError("PoolScheduler: slots must be >= 1")
        self.S = slots
        self.slots = [_Slot(embed, decoding_chunk_size) for _ in range(slots)]
        self.window, self.stride, self.ctx = self.slots[0].plan.window, self.slots[0].plan.stride, self.slots[0].plan.ctx
        self.ring_frames = 2 * (self.window + self.stride) if ring_frames is None else int(ring_frames)
        if self.ring_frames < self.window + self.stride:
            # after its released windows ran a stream holds < stride + ctx <= window unconsumed frames: there is always room
            raise ValueError(f"PoolScheduler: ring_frames must be >= window + stride = {self.window + self.stride}")
        self.max_rows = slots if max_step_rows is None else int(max_step_rows)
        if not 1 <= self.max_rows <= slots:
            raise ValueError(f"PoolScheduler: max_step_rows must be in [1, {slots}]")
        self.buckets = sorted({min(1 << k, slots) for k in range(slots.bit_length() + 1)})
        self._slot_of: Dict[int, int] = {}
        self._next_sid = 0

    # ---- slots ---------------------------------------------------------------------------------------------------
    def open(self) -> int:
        for i, s in enumerate(self.slots):
            if s.sid is None:
                s.clear()
                s.sid = self._next_sid
                self._slot_of[s.sid] = i
                self._next_sid += 1
                return s.sid
        raise _pool_error(f"StreamPool.open: pool full (all {self.S} slots hold open streams)")

    def slot_of(self, sid: int, who: str = "StreamPool") -> int:
        slot = self._slot_of.get(sid) if isinstance(sid, int) else None
        if slot is None:
            state = "was closed" if isinstance(sid, int) and 0 <= sid < self._next_sid else "is unknown"
            raise _pool_error(f"{who}: stream sid {sid!r} {state}")
        return slot

    @property
    def active(self) -> List[int]:
        return sorted(self._slot_of)

    def release(self, sid: int):
        slot = self._slot_of.pop(sid)
        self.slots[slot].sid = None
        self.slots[slot].clear()

    def bucket(self, rows: int) -> int:
        return next(b for b in self.buckets if b >= rows)

    # ---- packets -------------------------------------------------------------------------------------------------
    def free_frames(self, slot: int) -> int:
        s = self.slots[slot]
        return self.ring_frames - (s.frames - s.consumed)

    def cut(self, left: Dict[int, List[int]]) -> List[Tuple[int, int, int, int, int, int]]:
        """left: {sid: [offset into its packet, samples left]}, updated in place."""
        pieces = []
        for sid, ol in left.items():
            if ol[1] <= 0:
                continue
            slot = self.slot_of(sid)
            s = self.slots[slot]
            if s.closing:
                raise _pool_error(f"StreamPool.feed: stream sid {sid} is closing")
            room = max(0, (WIN - 1) + SHIFT * self.free_frames(slot) - s.carry_len)   # frames(c + n) <= free
            n = min(ol[1], room)
            if n <= 0:
                continue
            f, c_next = _frames(s.carry_len, n)
            pieces.append((sid, slot, ol[0], n, s.carry_len, s.frames))
            s.carry_len, s.frames = c_next, s.frames + f
            s.queue.extend(s.plan.push(f))
            ol[0], ol[1] = ol[0] + n, ol[1] - n
        return pieces

    def close(self, sids: Sequence[int]):
        for sid in sids:
            s = self.slots[self.slot_of(sid, "StreamPool.close")]
            if not s.closing:
                s.closing = True
                s.queue.extend(s.plan.finish())

    # ---- rounds --------------------------------------------------------------------------------------------------
    def pending(self) -> bool:
        return any(s.queue for s in self.slots)

    def next_round(self) -> List[Step]:
        groups: Dict[Tuple[int, int], List[Row]] = {}
        for i, s in enumerate(self.slots):
            if not s.queue:
                continue
            start, length, final = s.queue.popleft()
            first = start == 0
            short = length < self.window
            # order: first windows (longest first), the full windows, the shorter last ones
            key = (0, -length) if first else ((2, -length) if short else (1, 0))
            groups.setdefault(key, []).append(Row(s.sid, i, start, length, final))
            s.consumed = min(start + self.stride, s.frames)
        steps = []
        for key in sorted(groups):
            rows = groups[key]
            for a in range(0, len(rows), self.max_rows):
                part = rows[a:a + self.max_rows]
                steps.append(Step(part, key[0] == 0, self.bucket(len(part)) if key[0] == 1 else len(part)))
        return steps


class _Bucket:
    """The fixed buffers of the steps of one padded batch size: compact state, the windows, idx / offsets, the output rows."""

    def __init__(self, pool: "StreamPool", batch: int):
        from ..hip_ops import RowsTable
        dev = pool.device
        self.batch = batch
        self.state = [{k: v.new_zeros((batch,) + tuple(v.shape[1:])) for k, v in st.items()} for st in pool._state]
        self.xs = pool.fbank.ring.new_zeros(batch, pool.sched.window, pool.fbank.nmel)
        self.io = torch.zeros((2, batch), dtype=torch.int32, device=dev)     # idx and the ring offsets: one upload per step
        self.io[0].fill_(-1)
        self.idx, self.offs = self.io[0], self.io[1]
        pairs = [(pool._state[i][k], self.state[i][k]) for i in range(len(self.state)) for k in self.state[i]]
        self.t_state = RowsTable(pairs)
        self.t_full = RowsTable(pairs, [(pool.fbank.ring, self.xs)])
        self.rows_out = None        # (batch, chunk, V | D), made by the first step
        self.t_out = None
        self.uses = 0
        self.graph = None
        self.y = None
        self.refused = False


class StreamPool:
    """Streaming search of up to `slots` independent audio streams.  mode: ctc_greedy_search / ctc_prefix_beam_search (an
    ASRModel with a streamable encoder) or rnnt_greedy_search (a Transducer); beam_size, context_graph, blank_id, blank_penalty,
    max_total_frames, n_steps as AudioStreamer.

    sid = open() takes a free slot (PafcError "pool full" when there is none).  feed(sids, samples (R, n_max) float32 in int16
    range on the model's device, lengths=None): row i brings samples[i, :lengths[i]] to stream sids[i]; every window the
    samples complete runs, batched with the windows of the other streams of this feed, and the call returns {sid: partial}
    -- CTC: the stream's partial DecodeResult as of its last window, RNN-T: its new tokens -- or None for a stream none of whose
    windows ran.  close(sid or list) runs what is left of the stream(s), returns the final DecodeResult(s) -- what
    AudioStreamer.finish returns for the same audio -- and frees the slot(s).  committed(sid): the tokens that can no longer
    change; active: the open sids; step_log: per step {"rows": [(sid, window start, length, final)], "slots": the rows'
    slots, "batch": the padded batch size, "first": run without state, "in_place": the carries were fixed buffers updated
    where they lie, "replayed": a captured graph ran}.  on_encoder_out(step_log entry, y (rows, n, D)) sees every step's
    encoder output (a replayed step's is the graph's own buffer: copy what is to be kept).

    A step is: gather the carried state and the feature windows of its rows (one launch), forward_chunk_carry, scatter the
    state back (one launch), ctc_logprobs, scatter the output rows into the decoder's `slots`-wide chunk (one launch),
    decoder.feed with nframes = 0 for every stream that sat out.  The first window of a stream runs with state=None among first
    windows only, and its carries overwrite whatever the slot held; a shorter last window runs with those of its length.  With
    use_graph every padded batch size keeps fixed buffers, runs its steps in place, is captured into a hipGraph the second
    time it is used and replayed from then on after one small upload of idx and the offsets; a refused capture leaves that
    batch size eager.  A stream that passes max_total_frames raises PafcError naming its sid after the feed has served the
    others; it takes no more frames, close() returns what it had taken and lists its sid in `truncated`.

    sample_rate: the rate of the samples feed() takes.  At another rate than 16 000 Hz a dataset.resample.ResampleSlotStreamer
    turns the rows of a feed into 16 kHz samples on the device first (one more launch pair; the counts are host arithmetic), the
    resampled rows are cut against the ring as a 16 kHz packet is, and close() flushes the stream's resampler into the fbank
    before its last window: the results are exactly those of a pool fed resample_batch of every stream's whole audio.  At
    16 000 none is constructed.

    Not offered, with a ValueError: rnnt_beam_search (its streaming bench ended in a device exception whose cause is open),
    encoders that cannot stream, and the look-ahead model (non-causal conv module): its layers emit a number of frames that
    depends on the age of the stream, so streams of different ages cannot share a dense batch."""

    def __init__(self, model: torch.nn.Module, slots: int, decoding_chunk_size: int, mode: str = "ctc_prefix_beam_search",
                 beam_size: int = 10, context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0,
                 max_total_frames: int = 4096, n_steps: int = 64, max_step_rows: Optional[int] = None, use_graph: bool = True,
                 on_encoder_out: Optional[Callable] = None, num_mel_bins: int = 80, ring_frames: Optional[int] = None,
                 sample_rate: int = 16000):
        if mode == "rnnt_beam_search":
            raise ValueError("StreamPool: rnnt_beam_search is not offered in the pool: its streaming bench ended in a device "
                             "exception whose cause is still open, and the pool adds no new way to reach it")
        if mode not in MODES:
            raise ValueError(f"StreamPool: mode must be one of {MODES}, got {mode!r}")
        p = next(model.parameters())
        # the checks of the window walk itself (chunk size, streamable pre-norm uni-directional encoder), on an empty stream
        list(model._stream_windows(torch.empty(1, 0, num_mel_bins, device=p.device, dtype=p.dtype), decoding_chunk_size,
                                   "StreamPool"))
        enc = model.encoder
        if any(l.conv_module is not None and l.conv_module.lorder == 0 for l in enc.encoders):
            raise ValueError("StreamPool: the look-ahead model (non-causal conv module) is not offered in the pool: its layers "
                             "emit a number of frames that depends on the age of the stream, so streams of different ages "
                             "cannot share a dense batch (AudioStreamer serves it in lock step)")
        if mode == "rnnt_greedy_search" and not (hasattr(model, "predictor") and hasattr(model, "joint")):
            raise ValueError("StreamPool: rnnt_greedy_search needs a Transducer")
        self.sched = PoolScheduler(enc.embed, slots, decoding_chunk_size, ring_frames, max_step_rows)
        self.model, self.S, self.chunk, self.mode = model, slots, decoding_chunk_size, mode
        self.device = p.device
        self.use_graph = bool(use_graph)
        self._blank_id, self._blank_penalty = blank_id, blank_penalty
        self._on_encoder_out = on_encoder_out
        self.step_log: List[dict] = []
        from ..dataset.fbank import FbankSlotStreamer
        self.fbank = FbankSlotStreamer(slots, self.sched.ring_frames, num_mel_bins, p.dtype, p.device)
        self._frame_bytes = num_mel_bins * self.fbank.ring.element_size()
        self.sample_rate = sample_rate
        self.resampler = None
        if sample_rate != 16000:
            from ..dataset import resample as _resample
            self.resampler = _resample.ResampleSlotStreamer(slots, sample_rate, 16000, p.device)
        if mode == "rnnt_greedy_search":
            from ..transducer.search.greedy_search import GreedyStreamer
            self.decoder = GreedyStreamer(model, slots, decoding_chunk_size, n_steps)
        else:
            from ..transformer.search import CtcStreamer
            self.decoder = CtcStreamer(slots, decoding_chunk_size, mode, beam_size, context_graph, blank_id, max_total_frames)
        self._state: Optional[List[Dict[str, torch.Tensor]]] = None      # per layer {name: (slots, ...)}
        self._dec_buf: Optional[torch.Tensor] = None                      # (slots, chunk, V | D): the decoder's chunk
        self._buckets: Dict[int, _Bucket] = {}
        self._partial: List = [None] * slots
        self._ran: List[bool] = [False] * slots
        self._over: List[Tuple[int, int]] = []
        self.truncated: List[int] = []      # sids closed after the decoder had refused them frames (max_total_frames)

    # ---- the public surface --------------------------------------------------------------------------------------
    def open(self) -> int:
        sid = self.sched.open()
        slot = self.sched.slot_of(sid)
        self.fbank.reset(slot)
        if self.resampler is not None:
            self.resampler.reset(slot)
        self.decoder.reset([slot])       # (a slot is reset when it is freed as well: nothing of an earlier stream is left)
        self._partial[slot] = None
        return sid

    @property
    def active(self) -> List[int]:
        return self.sched.active

    def committed(self, sid: int) -> List[int]:
        slot = self.sched.slot_of(sid, "StreamPool.committed")
        if self.mode == "rnnt_greedy_search":       # a greedy token is final when it is emitted
            return list(self.decoder._hyps[slot])
        return list(self.decoder.committed[slot])

    @torch.no_grad()
    def feed(self, sids: Sequence[int], samples: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> dict:
        sids = [sids] if isinstance(sids, int) else list(sids)
        if samples.dim() != 2 or samples.size(0) != len(sids):
            raise ValueError(f"StreamPool.feed: samples must be ({len(sids)}, n_max), one row per sid")
        slots = [self.sched.slot_of(sid, "StreamPool.feed") for sid in sids]      # (raises before anything changes)
        if len(set(sids)) != len(sids):
            raise ValueError("StreamPool.feed: a stream may be named once per feed")
        for sid, slot in zip(sids, slots):
            if self.sched.slots[slot].closing:
                raise _pool_error(f"StreamPool.feed: stream sid {sid} is closing")
        n_max = samples.size(1)
        lengths = [n_max] * len(sids) if lengths is None else [int(v) for v in lengths]
        if len(lengths) != len(sids) or any(not 0 <= n <= n_max for n in lengths):
            raise ValueError(f"StreamPool.feed: lengths must be {len(sids)} values in [0, {n_max}]")
        for slot in slots:
            self._ran[slot] = False
        self._over = []
        if self.resampler is not None:
            samples, lengths = self.resampler.feed_rows(slots, samples, lengths)
        self._feed_16k(sids, samples, lengths)
        out = {}
        for sid, slot in zip(sids, slots):
            out[sid] = self._partial[slot] if self._ran[slot] else None
            if self.mode == "rnnt_greedy_search":
                self._partial[slot] = None
        self._raise_over()
        return out

    def _feed_16k(self, sids: List[int], samples: torch.Tensor, lengths: List[int]):
        """Rows of 16 kHz samples into the fbank, cut against the rings, and every window they complete."""
        row_of = {sid: i for i, sid in enumerate(sids)}
        left = {sid: [0, n] for sid, n in zip(sids, lengths)}
        while any(ol[1] > 0 for ol in left.values()):
            pieces = self.sched.cut(left)
            if not pieces:
                raise _pool_error("StreamPool.feed: no room in any ring and no window to run")      # (cannot happen)
            whole = len(pieces) == len(sids) and all(off == 0 for _, _, off, _, _, _ in pieces) and \
                [sid for sid, *_ in pieces] == sids
            if whole:
                chunk = samples
            else:                           # a cut packet, or rows that wait: the pieces as rows of their own
                width = max(n for _, _, _, n, _, _ in pieces)
                chunk = samples.new_zeros(len(pieces), width)
                for j, (sid, _, off, n, _, _) in enumerate(pieces):
                    chunk[j, :n] = samples[row_of[sid], off:off + n]
            got = self.fbank.feed_rows([slot for _, slot, *_ in pieces], chunk, [n for _, _, _, n, _, _ in pieces])
            for (sid, slot, _, n, c, first), f in zip(pieces, got):
                assert (f, self.fbank.frames_emitted[slot]) == (_frames(c, n)[0], self.sched.slots[slot].frames)
            self._run_rounds()

    @torch.no_grad()
    def close(self, sids):
        many = not isinstance(sids, int)
        sids = list(sids) if many else [sids]
        slots = [self.sched.slot_of(sid, "StreamPool.close") for sid in sids]
        if len(set(sids)) != len(sids):
            raise ValueError("StreamPool.close: a stream may be named once")
        self._over = []
        if self.resampler is not None:      # the outputs that were waiting for samples behind the last one
            live = [(sid, slot) for sid, slot in zip(sids, slots) if not self.sched.slots[slot].closing]
            if live:
                tail, counts = self.resampler.feed_rows([slot for _, slot in live], None, None, final=True)
                self._feed_16k([sid for sid, _ in live], tail, counts)
        self.sched.close(sids)
        self._run_rounds()                  # (only the closing streams have windows left)
        results = self.decoder.results()
        out = [results[slot] for slot in slots]
        full = getattr(self.decoder, "_full", None)
        for sid, slot in zip(sids, slots):
            if full is not None and full[slot]:
                self.truncated.append(sid)
            self.sched.release(sid)
            self.fbank.reset(slot)
            self.decoder.reset([slot])
            self._partial[slot] = None
        self._over = []
        return out if many else out[0]

    # ---- steps -----------------------------------------------------------------------------------------------------
    def _raise_over(self):
        if self._over:
            over, self._over = self._over, []
            names = ", ".join(f"sid {sid} (slot {slot})" for sid, slot in over)
            raise _pool_error(f"StreamPool: stream {names} would pass max_total_frames = {self.decoder.max_total} and takes no "
                              "more frames; close it (the other streams were served)")

    def _run_rounds(self):
        while self.sched.pending():
            for step in self.sched.next_round():
                self._run_step(step)

    def _upload(self, step: Step):
        """idx and the ring offsets (bytes) of a step's rows, padded to its batch, as ONE host tensor."""
        pad = step.batch - len(step.rows)
        ring = self.sched.ring_frames
        idx = [r.slot for r in step.rows] + [-1] * pad
        offs = [(r.start % ring) * self._frame_bytes for r in step.rows] + [0] * pad
        return torch.tensor([idx, offs], dtype=torch.int32)

    def _bucket(self, batch: int) -> _Bucket:
        b = self._buckets.get(batch)
        if b is None:
            b = self._buckets[batch] = _Bucket(self, batch)
        return b

    def _decoder_rows(self, y: torch.Tensor) -> torch.Tensor:
        if self.mode == "rnnt_greedy_search":
            return y
        return self.model.ctc_logprobs(y, self._blank_penalty, self._blank_id)

    def _as_chunk_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """(m, n <= chunk, V) -> contiguous (m, chunk, V), the row shape of the decoder's chunk."""
        if self._dec_buf is None:
            self._dec_buf = rows.new_zeros(self.S, self.chunk, rows.size(2))
        if rows.size(1) == self.chunk and rows.is_contiguous():
            return rows
        full = rows.new_zeros(rows.size(0), self.chunk, rows.size(2))
        full[:, :rows.size(1)] = rows
        return full

    def _scatter_state(self, new_state: list, idx: torch.Tensor, m: int):
        from ..hip_ops import RowsTable
        if self._state is None:            # the carries of a first window are full-shape: they size the per-slot storage
            self._state = [{k: v.new_zeros((self.S,) + tuple(v.shape[1:])) for k, v in st.items()} for st in new_state]
        pairs = [(self._state[i][k], v.contiguous()) for i, st in enumerate(new_state) for k, v in st.items()]
        RowsTable(pairs).scatter(idx, m)

    def _run_step(self, step: Step):
        from ..hip_ops import RowsTable
        enc = self.model.encoder
        rows, m, batch = step.rows, len(step.rows), step.batch
        length = rows[0].length
        full = not step.first and length == self.sched.window
        host = self._upload(step)
        rec = {"rows": [(r.sid, r.start, r.length, r.final) for r in rows], "slots": [r.slot for r in rows], "batch": batch,
               "first": step.first, "in_place": False, "replayed": False}
        if not full:
            # a first window (no state) or a shorter last one: its own shape, eagerly
            dev = host.to(self.device)
            idx, offs = dev[0], dev[1]
            xs = self.fbank.ring.new_empty(batch, length, self.fbank.nmel)
            if step.first:
                RowsTable([], [(self.fbank.ring, xs)]).gather(idx, batch, offs)
                y, new_state = enc.forward_chunk_carry(xs, 0, None)
            else:
                b = self._bucket(batch)
                b.t_state.gather(idx, batch)
                RowsTable([], [(self.fbank.ring, xs)]).gather(idx, batch, offs)
                y, new_state = enc.forward_chunk_carry(xs, 0, b.state)
            self._scatter_state(new_state, idx, batch)
            out_rows = self._as_chunk_rows(self._decoder_rows(y))
            RowsTable([(self._dec_buf, out_rows)]).scatter(idx, batch)
        else:
            b = self._bucket(batch)
            b.uses += 1
            if not self.use_graph:
                dev = host.to(self.device)
                idx, offs = dev[0], dev[1]
                b.t_full.gather(idx, batch, offs)
                y, new_state = enc.forward_chunk_carry(b.xs, 0, b.state)
                self._scatter_state(new_state, idx, batch)
                out_rows = self._as_chunk_rows(self._decoder_rows(y))
                RowsTable([(self._dec_buf, out_rows)]).scatter(idx, batch)
            else:
                b.io.copy_(host)
                rec["in_place"] = True
                if b.graph is None and b.uses == 2 and not b.refused:
                    b.graph, b.y = graph_step.capture(lambda: self._in_place_step(b), self.device)
                    b.refused = b.graph is None
                if b.graph is not None:
                    b.graph.replay()
                    y, rec["replayed"] = b.y, True
                elif b.uses == 1:           # off the default stream, as the capture that follows wants its warm-up
                    y = graph_step.on_side_stream(self.device, lambda: self._in_place_step(b))
                else:
                    y = self._in_place_step(b)
        n_out = y.size(1)
        self.step_log.append(rec)
        if self._on_encoder_out is not None:
            self._on_encoder_out(rec, y[:m])
        self._feed_decoder(rows, n_out)

    def _in_place_step(self, b: _Bucket) -> torch.Tensor:
        """The whole step of a padded batch size over its fixed buffers: what a captured graph holds."""
        from ..hip_ops import RowsTable
        b.t_full.gather(b.idx, b.batch, b.offs)
        y, new_state = self.model.encoder.forward_chunk_carry(b.xs, 0, b.state, in_place=True)
        for st, nw in zip(b.state, new_state):
            if nw is not st:                    # (the fused step updates its carries where they lie)
                for k in st:
                    st[k].copy_(nw[k])
        b.t_state.scatter(b.idx, b.batch)
        out = self._decoder_rows(y)
        if b.rows_out is None:
            b.rows_out = self._as_chunk_rows(out).clone()
            b.t_out = RowsTable([(self._dec_buf, b.rows_out)])
        else:
            b.rows_out[:, :out.size(1)].copy_(out)
        b.t_out.scatter(b.idx, b.batch)
        return y

    def _feed_decoder(self, rows: List[Row], n_out: int):
        nf = [0] * self.S
        for r in rows:
            nf[r.slot] = n_out
        if n_out == 0:
            return
        from .._lib import PafcError
        if self.mode == "rnnt_greedy_search":
            toks = self.decoder.feed(self._dec_buf, nf)
            for r in rows:
                self._partial[r.slot] = (self._partial[r.slot] or []) + list(toks[r.slot])
                self._ran[r.slot] = True
            return
        try:
            part = self.decoder.feed(self._dec_buf, nf)
        except PafcError:
            newly = [r for r in rows if self.decoder._full[r.slot]]
            if not newly:
                raise
            self._over += [(r.sid, r.slot) for r in newly if (r.sid, r.slot) not in self._over]
            part = self.decoder.partials()
        for r in rows:
            self._partial[r.slot] = part[r.slot]
            self._ran[r.slot] = True
