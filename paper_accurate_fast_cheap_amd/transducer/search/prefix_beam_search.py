"""CTC-fused RNN-T prefix beam search (reference: wenet/transducer/search/prefix_beam_search.py:428-574, the
`prefix_beam_search_decode_batch` that `Transducer.beam_search_decode` reaches through :219-220).

Per frame t and utterance: one predictor step + joint for every live beam, log_softmax, shallow fusion
log(w_rnnt e^{rnnt} + w_ctc e^{ctc}), top-`beam` tokens per beam, candidates visited in descending score order,
equal hypotheses merged with log_add, stop once `beam` distinct hypotheses are collected, keep the best `beam`;
at most one symbol per frame.  Token ids are the bit-exact parity bar, so the candidate walk below follows the
reference statement by statement -- including its rounding points (beam scores go through float32 every frame)
and its early stop (later duplicates of an already-collected hypothesis are NOT merged once the beam is full).

What changed for the GPU: the reference reads every candidate with `.item()` (beam^2 x 3 host syncs per utterance
and frame) and concatenates per-beam LSTM states with torch.cat every frame.  Here the LSTM states of all beams
of all utterances stay in two batched device tensors that are re-indexed once per frame, and the host receives
ONE packed (scores, indices) block per frame for the whole batch."""
import contextlib
from typing import List, Optional

import torch

from ...transformer.search import DecodeResult, _common_prefix_len, log_add
from ...utils import graph_step


FRAME_BODIES = ("framework", "kernels")


def check_frame_body(value: str) -> str:
    """The per-frame body of the device-resident search: "framework" (predictor step, joint, fusion and top-k as framework
    ops) or "kernels" (hip_ops.RnntBeamBody: the same frame as the library's own kernels, never a fallback)."""
    if value not in FRAME_BODIES:
        raise ValueError(f"frame_body must be one of {FRAME_BODIES}, got {value!r}")
    return value


class Sequence:
    __slots__ = ("hyp", "score", "cache")

    def __init__(self, hyp: List[int], score: float, cache: int):
        self.hyp = hyp
        self.score = score
        self.cache = cache   # column of the batched state tensors that holds this beam's LSTM state


def _result(nbest: List[List[int]], scores: List[float]) -> DecodeResult:
    """The DecodeResult of an n-best list in descending score order (empty: a row that holds no hypothesis yet)."""
    if not nbest:
        return DecodeResult(tokens=[], score=0.0, nbest=[], nbest_scores=[])
    return DecodeResult(tokens=nbest[0], score=scores[0], nbest=nbest, nbest_scores=scores)


class _ResidentFrames:
    """The frame of the device-resident search over B x beam fixed slots, with its warm-up, capture and replay: what the
    offline decode (over the caller's tensors) and BeamStreamer (over its staging buffers) both run.  Every tensor a frame
    touches has a fixed address and shape and the frame index lives on the device (t_dev), so the frame is captured once and
    replayed.  slots: hip_ops.RnntBeamState or RnntBeamStream; step(top_val, top_idx, t_dev): the caller's bound step call;
    src (B, T, D): the encoder rows -- with `body` (hip_ops.RnntBeamBody: the frame as the library's kernels) E = enc_ffn
    rows (B, T, J) --, ctc (B, T, V); a frame reads row min(t_dev, T - 1) of both.  cache: the LSTM state [h, c], updated in
    place.  chain_select: the framework body selects the state with the framework chain, not pafc_rnnt_beam_select_state.
    The object is in no reference cycle (it stores no bound method of its own), so it dies -- and its hipGraph with it -- when
    its owner drops it, never in a later garbage collection, which could run inside somebody else's stream capture."""

    def __init__(self, bs, slots, step, src, ctc, cache, w_rnnt: float, w_ctc: float, body=None, chain_select: bool = False):
        from ...hip_ops import rnnt_beam_select_state
        self.bs, self.slots, self.step, self.src, self.ctc, self.cache, self.body = bs, slots, step, src, ctc, cache, body
        self.w_rnnt, self.w_ctc, self.chain_select, self._select = w_rnnt, w_ctc, chain_select, rnnt_beam_select_state
        self.device = src.device
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.graph = False                                 # False: no capture tried; None: the capture was refused

    def frame(self):
        """One frame for all slots: the kernels body when the engine was given one, else the framework body."""
        if self.body is None:
            return self._frame_framework()
        st, body, (h, c), t_dev = self.slots, self.body, self.cache, self.t_dev
        body.frame(self.src, self.ctc, self.w_rnnt, self.w_ctc, st.last_tok, h, c, t_dev=t_dev)
        self.step(body.top_val, body.top_idx, t_dev)
        self._select(h, c, body.h_new, body.c_new, st.next_idx, st.B, st.beam)
        body.advance(t_dev)

    def _frame_framework(self):
        st, cache, t_dev, beam, last = self.slots, self.cache, self.t_dev, self.slots.beam, self.src.shape[1] - 1
        enc = self.src.index_select(1, t_dev.clamp(max=last)).squeeze(1)
        enc = enc.repeat_interleave(beam, dim=0).unsqueeze(1)                                    # (n, 1, D)
        logp, new_cache = self.bs.forward_decoder_one_step(enc, st.last_tok, cache)
        logp = logp.squeeze(1).squeeze(1)                                                        # (n, V)
        ctc_t = self.ctc.index_select(1, t_dev.clamp(max=last)).squeeze(1).repeat_interleave(beam, dim=0)
        logp = torch.log(torch.add(self.w_rnnt * torch.exp(logp), self.w_ctc * torch.exp(ctc_t)))
        top_val, top_idx = logp.topk(beam)
        self.step(top_val.float().contiguous(), top_idx.contiguous(), t_dev)
        if self.chain_select:
            cache[0].copy_(torch.cat([cache[0], new_cache[0]], dim=1).index_select(1, st.next_idx))
            cache[1].copy_(torch.cat([cache[1], new_cache[1]], dim=1).index_select(1, st.next_idx))
        else:
            self._select(cache[0], cache[1], new_cache[0].contiguous(), new_cache[1].contiguous(), st.next_idx, st.B, st.beam)
        t_dev.add_(1)

    def capture(self):
        """Two eager frames on the side stream (they warm every library handle), then the frame captured into a hipGraph.
        Only a REFUSED capture (an operation the stream capture does not permit in this build) leaves None -- nothing ran
        during it, so t_dev stands behind the two warm-up frames and run() goes on eagerly; a failing launch or a PafcError
        inside the frame is a real error and surfaces."""
        graph_step.on_side_stream(self.device, lambda: (self.frame(), self.frame()))
        self.graph = graph_step.capture(self.frame, self.device)[0]

    def run(self, k: int):
        """k frames: replays of the captured graph (their errors are genuine kernel / launch errors: not swallowed), else eager."""
        for _ in range(k):
            if self.graph:
                self.graph.replay()
            else:
                self.frame()


class PrefixBeamSearch:
    def __init__(self, encoder, predictor, joint, ctc, blank):
        self.encoder = encoder
        self.predictor = predictor
        self.joint = joint
        self.ctc = ctc
        self.blank = blank
        self.device_resident = True   # GPU tensors: keep the beams on the device (False: host bookkeeping, one copy per frame)
        self.use_graph = True         # device-resident path: replay the frame body from a captured hipGraph
        self.frame_body = "framework"  # device-resident path: the frame as framework ops, or "kernels" (check_frame_body)

    @property
    def frame_body(self) -> str:
        return self._frame_body

    @frame_body.setter
    def frame_body(self, value: str):
        self._frame_body = check_frame_body(value)

    def forward_decoder_one_step(self, encoder_x: torch.Tensor, pre_t: torch.Tensor, cache: List[torch.Tensor]):
        padding = torch.zeros(pre_t.size(0), 1, device=encoder_x.device, dtype=cache[0].dtype)
        pre_t, new_cache = self.predictor.forward_step(pre_t.unsqueeze(-1), padding, cache)
        x = self.joint(encoder_x, pre_t)
        return x.log_softmax(dim=-1), new_cache

    @torch.no_grad()
    def prefix_beam_search_decode(self, encoder_outs, encoder_lens, ctc_probs, decoding_chunk_size: int = -1,
                                  beam_size: int = 5, num_decoding_left_chunks: int = -1,
                                  simulate_streaming: bool = False, ctc_weight: float = 0.3,
                                  transducer_weight: float = 0.7, cat_embs: Optional[torch.Tensor] = None,
                                  frame_body: Optional[str] = None):
        assert encoder_outs.shape[0] == encoder_lens.shape[0] == ctc_probs.shape[0]
        return self.prefix_beam_search_decode_batch(encoder_outs, encoder_lens, ctc_probs, decoding_chunk_size,
                                                    beam_size, num_decoding_left_chunks, simulate_streaming,
                                                    ctc_weight, transducer_weight, cat_embs, frame_body)

    @torch.no_grad()
    def prefix_beam_search_decode_batch(self, encoder_outs, encoder_lens, ctc_probs, decoding_chunk_size: int = -1,
                                        beam_size: int = 5, num_decoding_left_chunks: int = -1,
                                        simulate_streaming: bool = False, ctc_weight: float = 0.3,
                                        transducer_weight: float = 0.7, cat_embs: Optional[torch.Tensor] = None,
                                        frame_body: Optional[str] = None):
        """frame_body: None (this object's frame_body) or a value of FRAME_BODIES for this call."""
        device = encoder_outs.device
        B = encoder_outs.shape[0]
        if check_frame_body(self.frame_body if frame_body is None else frame_body) == "kernels":
            return self._decode_batch_kernels(encoder_outs, encoder_lens, ctc_probs, beam_size, ctc_weight, transducer_weight)
        if self.device_resident and encoder_outs.is_cuda and beam_size <= 16 and B > 0 and encoder_outs.shape[1] > 0:
            return self._decode_batch_resident(encoder_outs, encoder_lens, ctc_probs, beam_size, ctc_weight,
                                               transducer_weight)
        lens = [int(v) for v in encoder_lens.tolist()]
        max_len = max(lens) if lens else 0
        state = self.predictor.init_state(B, method="zero", device=device)
        state = [s.to(encoder_outs.dtype) for s in state]        # column b = utterance b's single start beam
        beams = [[Sequence([self.blank], 0.0, b)] for b in range(B)]

        for t in range(max_len):
            active = [i for i in range(B) if t < lens[i]]
            if not active:
                break
            live = [s for i in active for s in beams[i]]
            n = len(live)
            rows_t = torch.tensor([i for i in active for _ in beams[i]], device=device)
            cols_t = torch.tensor([s.cache for s in live], device=device)
            cache = [state[0].index_select(1, cols_t), state[1].index_select(1, cols_t)]
            cand_h, idx_h, state = self._host_frame(encoder_outs, ctc_probs, rows_t, t, live, cache, transducer_weight,
                                                    ctc_weight, beam_size)
            cur = 0
            for i in active:
                nb = len(beams[i])
                beams[i] = self._walk_row(beams[i], cand_h[cur:cur + nb], idx_h[cur:cur + nb], cur, n, beam_size)
                cur += nb

        return [_result([b.hyp[1:] for b in bs], [b.score for b in bs]) for bs in beams]

    def _host_frame(self, enc, ctc, rows_t, t: int, live: List[Sequence], cache, w_rnnt: float, w_ctc: float, beam_size: int):
        """Frame t of the host loops for the n live beams of the active rows: enc (B, T, D) and ctc (B, T, V), rows_t (n) each
        beam's utterance, cache its LSTM state ((layers, n, H) twice).  Returns the candidates' scores and tokens on the host,
        (n, beam_size) each, and next frame's state pool (layers, 2 n, H): old states (kept by blank extensions) then new
        states.  The rows are gathered here, each where it is used, so that the launches keep the order they always had."""
        device = enc.device
        enc_rows = enc[rows_t, t, :].unsqueeze(1)                                          # (n, 1, D)
        logp, new_cache = self.forward_decoder_one_step(enc_rows, torch.tensor([s.hyp[-1] for s in live], device=device), cache)
        logp = logp.squeeze(1).squeeze(1)                                                  # (n, V)
        logp = torch.log(torch.add(w_rnnt * torch.exp(logp), w_ctc * torch.exp(ctc[rows_t, t, :])))
        top_k_logp, top_k_index = logp.topk(beam_size)                                     # (n, beam)
        cand = torch.tensor([s.score for s in live], device=device).unsqueeze(1) + top_k_logp   # float32, as the reference
        packed = torch.cat([cand.float(), top_k_index.float()], dim=1).cpu()               # ONE device->host copy
        pool = [torch.cat([cache[0], new_cache[0]], dim=1), torch.cat([cache[1], new_cache[1]], dim=1)]
        return packed[:, :beam_size], packed[:, beam_size:].to(torch.int64), pool

    def _walk_row(self, beam: List[Sequence], cand_h: torch.Tensor, idx_h: torch.Tensor, cur: int, n: int,
                  beam_size: int) -> List[Sequence]:
        """One frame of one utterance on the host: the candidates (len(beam), beam_size) of its live beams, visited in
        descending order, equal hypotheses merged with log_add, stopped at beam_size distinct ones, sorted.  A survivor's
        cache is its column in [old states | new states] of this frame's n slots; the utterance's beams begin at `cur`."""
        flat = cand_h.reshape(-1)
        toks_flat = idx_h.reshape(-1).tolist()
        vals = flat.tolist()
        order = torch.argsort(flat, descending=True).tolist()                     # reference: :524
        beam_A: List[Sequence] = []
        seen = set()
        for k in order:
            b_idx, tok, score = k // beam_size, toks_flat[k], vals[k]
            base = beam[b_idx]
            new_hyp = list(base.hyp) if tok == self.blank else base.hyp + [tok]
            key = tuple(new_hyp)
            if key in seen:
                for ex in beam_A:
                    if ex.hyp == new_hyp:
                        ex.score = log_add([ex.score, score])
                        break
            else:
                seen.add(key)
                beam_A.append(Sequence(new_hyp, score, (cur + b_idx) if tok == self.blank else (n + cur + b_idx)))
                if len(beam_A) >= beam_size:
                    break
        beam_A.sort(key=lambda s: s.score, reverse=True)
        return beam_A[:beam_size]

    @torch.no_grad()
    def _decode_batch_resident(self, encoder_outs, encoder_lens, ctc_probs, beam_size: int, ctc_weight: float,
                               transducer_weight: float):
        """The same search with the beams on the device (pafc_rnnt_beam_*): B x beam fixed slots, predictor step,
        joint, fusion and top-k as batched ops over all slots, the candidate walk in a kernel, LSTM states re-indexed
        by the kernel's output -- no host synchronisation until the n-best lists are read back."""
        from ...hip_ops import RnntBeamState
        device = encoder_outs.device
        B, T, _ = encoder_outs.shape
        n = B * beam_size
        lens64 = encoder_lens.to(device=device, dtype=torch.int64).contiguous()
        st = RnntBeamState(B, T, beam_size, self.blank, device)
        state = self.predictor.init_state(n, method="zero", device=device)
        cache = [s.to(encoder_outs.dtype).contiguous() for s in state]        # static buffers, updated in place
        eng = _ResidentFrames(self, st, lambda tv, ti, t_dev: st.step(0, lens64, tv, ti, t_dev=t_dev), encoder_outs,
                              ctc_probs.contiguous(), cache, transducer_weight, ctc_weight, chain_select=True)
        done = 0
        if self.use_graph and T >= 8:
            # launch-bound loop (~25 small kernels per frame): the two warm-up frames are frames 0 and 1, the captured body
            # is replayed for the remaining ones.  MIOpen's RNN call is not capturable (it sizes its workspace inside the
            # call), so the LSTM runs through the framework's own cell.  After a refused capture the rest runs eagerly.
            with torch.backends.cudnn.flags(enabled=False):
                eng.capture()
                done = 2
                if eng.graph is not None:
                    eng.run(T - done)
                    done = T
        eng.run(T - done)
        return self._nbest(st, B, beam_size)

    @staticmethod
    def _nbest(st, B: int, beam_size: int) -> List[DecodeResult]:
        """The n-best lists of a finished device-resident search (hip_ops.RnntBeamState)."""
        toks, lens_n, scores = st.finish()
        lens_h, scores_h = lens_n.tolist(), scores.tolist()
        maxlen = max(1, int(lens_n.max()))
        toks_h = toks[:, :, :maxlen].tolist()
        used = [[k for k in range(beam_size) if lens_h[b][k] >= 0] for b in range(B)]
        return [_result([toks_h[b][k][:lens_h[b][k]] for k in used[b]], [scores_h[b][k] for k in used[b]]) for b in range(B)]

    @torch.no_grad()
    def _decode_batch_kernels(self, encoder_outs, encoder_lens, ctc_probs, beam_size: int, ctc_weight: float,
                              transducer_weight: float):
        """_decode_batch_resident with the frame as the library's own kernels (frame_body "kernels"): E = enc_ffn(encoder_outs)
        once through gemm_f32 / gemm_bf16, then per frame pafc_rnnt_beam_body (predictor step, joint, fusion with the CTC row
        read in place, top-k), the step kernel, pafc_rnnt_beam_select_state and the frame counter's increment -- captured
        once and replayed.  No framework op and no cudnn restriction in the loop; an unmet condition raises PafcError."""
        from ..._lib import PafcError
        from ...hip_ops import RnntBeamBody, RnntBeamState, rnnt_beam_body_unmet
        if not self.device_resident:
            raise PafcError("frame_body 'kernels': the kernels are the frame of the device-resident search (device_resident is False)")
        unmet = rnnt_beam_body_unmet(self.predictor, self.joint, encoder_outs, beam_size)
        if unmet is not None:
            raise PafcError(f"frame_body 'kernels': {unmet}")
        device = encoder_outs.device
        B, T, D = encoder_outs.shape
        if ctc_probs.device != device or ctc_probs.dim() != 3 or ctc_probs.shape[:2] != encoder_outs.shape[:2]:
            raise PafcError("frame_body 'kernels': ctc_probs must be (B, T, V) on the encoder output's GPU")
        body = RnntBeamBody(self.predictor, self.joint, B, beam_size)
        E = body.project(encoder_outs.detach().to(body.dtype).reshape(B * T, D).contiguous()).view(B, T, -1)
        if ctc_probs.dtype not in (torch.float32, torch.bfloat16):
            ctc_probs = ctc_probs.float()
        ctc_probs = ctc_probs.detach().contiguous()
        lens64 = encoder_lens.to(device=device, dtype=torch.int64).contiguous()
        st = RnntBeamState(B, T, beam_size, self.blank, device)
        eng = _ResidentFrames(self, st, lambda tv, ti, t_dev: st.step(0, lens64, tv, ti, t_dev=t_dev), E, ctc_probs,
                              list(body.zero_state()), transducer_weight, ctc_weight, body=body)
        done = 0
        if self.use_graph and T >= 8:
            eng.capture()                      # frames 0 and 1; after a refused capture the remainder runs eagerly
            done = 2
        eng.run(T - done)
        return self._nbest(st, B, beam_size)


class BeamStreamer:
    """CTC-fused RNN-T prefix beam search of `batch_size` streams fed chunk by chunk, the beams and the LSTM state of
    every stream carried from one feed to the next.  `model` holds predictor, joint and blank (a Transducer or a
    PrefixBeamSearch).  Over a stream, for any cut of its frames into chunks, the n-best token lists and float64 scores
    equal the offline search of the concatenated frames where both sides run the same arithmetic: host loop against
    prefix_beam_search_decode_batch's (both run _host_frame and _walk_row), device path against _decode_batch_resident's
    or _decode_batch_kernels' (both run _ResidentFrames on the same B x beam slots, and the candidate walk of
    csrc/rnnt_beam_frame.inc); only the step call, the frame clamp and where the state lives differ.

    feed(encoder_chunk (B, n <= max_frames, D), ctc_chunk (B, n, V) log-probs, nframes=None): row b consumes its first
    nframes[b] frames (default n; 0 = the row sits the chunk out, state unchanged).  Returns per row a partial
    DecodeResult: the 1-best and n-best if the stream ended here (None with partials=False).  `.committed` holds per row
    the tokens that can no longer change -- the common prefix of the row's live hypotheses; every later hypothesis is a
    live one or a live one plus a token -- and only grows.  reset(rows=None) restarts rows (all when None) from their
    next chunk on, LSTM state zeroed.  results(): per row the full DecodeResult.
    max_total_frames: the most frames a row may take between resets (the device path's trie pools are sized by it and are
    not compacted: reset a row at an endpoint).  A feed that would pass it leaves that row as it was, serves the other
    rows and raises PafcError naming the rows.

    Device path (GPU tensors, beam_size <= 16; hip_ops.RnntBeamStream, never a fallback): fixed (B, max_frames, D) and
    (B, max_frames, V) staging buffers; the frame body -- predictor step, joint, log-softmax, fusion, top-k, the step
    kernel, pafc_rnnt_beam_select_state -- reads the chunk frame its device counter names, always under
    cudnn.flags(enabled=False), and is captured once per streamer into a hipGraph (two eager warm-up frames on a side
    stream, with no row taking frames, so no state moves) and replayed once per chunk frame: max(nframes) times when the
    host knows the counts, else n times.  Only a REFUSED capture runs the body eagerly, with the same results.  Host reads per feed: one, the drain
    (none with partials=False); the chunk copies, the frame counts and the `from` offsets go to the device without a
    synchronising call (pass nframes as a device int64 tensor to keep them off the host altogether).
    frame_body "kernels" (default: the model's PrefixBeamSearch.frame_body, "framework"): the device path stages the chunk's
    E = enc_ffn rows (gemm_f32 / gemm_bf16 once per feed) instead of the raw encoder rows, and a frame is
    pafc_rnnt_beam_body, the step kernel, pafc_rnnt_beam_select_state and the frame counter's increment -- no framework op,
    no cudnn restriction; a condition the kernels do not meet (CPU tensors and beam_size > 16 included) raises PafcError.
    Host path (CPU tensors, or beam_size > 16): the loop of prefix_beam_search_decode_batch with the beams and each row's
    LSTM state carried between feeds; the active set of a frame is the rows with nframes[b] > j."""

    def __init__(self, model, batch_size: int, max_frames: int, beam_size: int = 10, ctc_weight: float = 0.3,
                 transducer_weight: float = 0.7, max_total_frames: int = 4096, use_graph: bool = True, partials: bool = True,
                 frame_body: Optional[str] = None):
        if batch_size < 1 or max_frames < 1 or max_total_frames < 1 or beam_size < 1:
            raise ValueError("BeamStreamer: batch_size, max_frames, max_total_frames and beam_size must be >= 1")
        self.bs = model if isinstance(model, PrefixBeamSearch) else PrefixBeamSearch(
            getattr(model, "encoder", None), model.predictor, model.joint, getattr(model, "ctc", None), model.blank)
        self.blank = self.bs.blank
        self.frame_body = check_frame_body(self.bs.frame_body if frame_body is None else frame_body)
        self.B, self.Tmax, self.beam, self.max_total = batch_size, max_frames, beam_size, max_total_frames
        self.ctc_weight, self.transducer_weight = ctc_weight, transducer_weight
        self.use_graph, self.want_partials = use_graph, partials
        self.committed: List[List[int]] = [[] for _ in range(batch_size)]
        self._device = None
        self._gpu = None                                   # hip_ops.RnntBeamStream, made by the first feed of GPU tensors
        self._eng: Optional[_ResidentFrames] = None        # its frames, over the staging buffers
        self._frames = [0] * batch_size                    # frames consumed per row, as far as the host knows
        self._maxlen = [0] * batch_size                    # the longest token list of a row's beam as of the last drain
        self._full = [False] * batch_size
        self._beams = [[Sequence([self.blank], 0.0, 0)] for _ in range(batch_size)]      # host path
        self._hstate: List[Optional[List[torch.Tensor]]] = [None] * batch_size           # host path: (layers, beams, H) per row
        self._last: Optional[List[DecodeResult]] = None

    @property
    def graphed(self) -> bool:
        """Whether the device path replays a captured graph."""
        return bool(self._eng is not None and self._eng.graph)

    def reset(self, rows=None):
        rows = list(range(self.B)) if rows is None else [int(b) for b in rows]
        for b in rows:
            self.committed[b] = []
            self._frames[b], self._maxlen[b], self._full[b] = 0, 0, False
            self._beams[b] = [Sequence([self.blank], 0.0, 0)]
            self._hstate[b] = None
        if self._gpu is not None:
            self._gpu.reset(None if len(rows) == self.B else rows)
            for s in self._cache:                          # the LSTM state of the rows' slots
                if len(rows) == self.B:
                    s.zero_()
                else:
                    s.view(s.shape[0], self.B, -1).index_fill_(1, torch.tensor(rows, device=s.device), 0)

    # ---- device path -------------------------------------------------------------------------------------------
    def _make_gpu(self, enc: torch.Tensor, ctc: torch.Tensor):
        from ...hip_ops import RnntBeamStream
        dev, B, beam = enc.device, self.B, self.beam
        self._gpu = st = RnntBeamStream(B, self.Tmax, beam, self.blank, dev, self.max_total)
        self._body = None
        if self.frame_body == "kernels":
            # the chunk's encoder rows are staged only to be projected: the body reads E = enc_ffn rows and the CTC rows in place
            from ...hip_ops import RnntBeamBody
            self._body = body = RnntBeamBody(self.bs.predictor, self.bs.joint, B, beam)
            self._cache = list(body.zero_state())
            self._x = torch.zeros(B * self.Tmax, enc.shape[2], dtype=body.dtype, device=dev)
            self._E = torch.zeros(B, self.Tmax, body.join_dim, dtype=body.dtype, device=dev)
            cdt = ctc.dtype if ctc.dtype in (torch.float32, torch.bfloat16) else torch.float32
        else:
            state = self.bs.predictor.init_state(B * beam, method="zero", device=dev)
            self._cache = [s.to(enc.dtype).contiguous() for s in state]      # static buffers, updated in place
            self._enc = torch.zeros(B, self.Tmax, enc.shape[2], dtype=enc.dtype, device=dev)
            cdt = ctc.dtype
        self._ctc = torch.zeros(B, self.Tmax, ctc.shape[2], dtype=cdt, device=dev)
        # chunk frame t_dev of the staging buffers: the frames of the offline decode, the step and the clamp apart
        self._eng = _ResidentFrames(self.bs, st, lambda tv, ti, j_dev: st.step(0, tv, ti, j_dev=j_dev),
                                    self._enc if self._body is None else self._E, self._ctc, self._cache,
                                    self.transducer_weight, self.ctc_weight, body=self._body)

    def _feed_gpu(self, enc, ctc, nf, n):
        st, eng = self._gpu, self._eng
        kernels = self._body is not None
        if n:
            if kernels:
                self._x.view(self.B, self.Tmax, -1)[:, :n].copy_(enc.detach())
                self._body.project(self._x, out=self._E.view(self.B * self.Tmax, -1))
            else:
                self._enc[:, :n].copy_(enc.detach())
            self._ctc[:, :n].copy_(ctc.detach())
        # framework body: MIOpen's RNN call is not capturable; the same cell eagerly.  The kernels need no such restriction.
        with contextlib.nullcontext() if kernels else torch.backends.cudnn.flags(enabled=False):
            if self.use_graph and eng.graph is False:
                st.feed(0)                                 # once per streamer, while no row takes frames: the warm-up moves no state
                eng.capture()
            st.feed(nf, n)
            eng.t_dev.zero_()
            eng.run(n if isinstance(nf, torch.Tensor) else max(nf))

    def _drain_gpu(self, ld: int) -> List[DecodeResult]:
        """One drain from the committed counts on; full token lists are the committed tokens + the returned tails."""
        d = self._gpu.drain([len(c) for c in self.committed], ld)
        out = []
        for b in range(self.B):
            live = range(d["count"][b])
            head = list(self.committed[b])
            nbest = [head + list(d["tokens"][b][k]) for k in live]
            nsc = [d["score"][b][k] for k in live]
            new = d["committed"][b] - len(head)
            if new > 0:
                self.committed[b] += d["tokens"][b][0][:new]
            self._maxlen[b] = max([d["len"][b][k] for k in live], default=0)
            if d["overflow"][b]:
                self._full[b] = True
            out.append(_result(nbest, nsc))
        self._overflow = d["overflow"]
        return out

    def _tail(self) -> int:
        return max(self._maxlen[b] - len(self.committed[b]) for b in range(self.B))

    # ---- host path ---------------------------------------------------------------------------------------------
    def _feed_host(self, enc, ctc, nf):
        bs, B, beam_size, device = self.bs, self.B, self.beam, enc.device
        beams = self._beams
        for b in range(B):
            if self._hstate[b] is None:
                self._hstate[b] = [s.to(enc.dtype) for s in bs.predictor.init_state(1, method="zero", device=device)]
        for t in range(max(nf) if nf else 0):
            active = [i for i in range(B) if t < nf[i]]
            if not active:
                break
            live = [s for i in active for s in beams[i]]
            n = len(live)
            rows_t = torch.tensor([i for i in active for _ in beams[i]], device=device)
            # the live beams' states, utterance by utterance: the columns prefix_beam_search_decode_batch selects
            cache = [torch.cat([self._hstate[i][k] for i in active], dim=1) for k in (0, 1)]
            cand_h, idx_h, pool = bs._host_frame(enc, ctc, rows_t, t, live, cache, self.transducer_weight, self.ctc_weight,
                                                 beam_size)
            cur = 0
            for i in active:
                nb = len(beams[i])
                beams[i] = bs._walk_row(beams[i], cand_h[cur:cur + nb], idx_h[cur:cur + nb], cur, n, beam_size)
                cols = torch.tensor([s.cache for s in beams[i]], device=device)
                self._hstate[i] = [pool[0].index_select(1, cols), pool[1].index_select(1, cols)]   # the row's own columns
                for k, s in enumerate(beams[i]):
                    s.cache = k
                cur += nb

    def _host_results(self) -> List[DecodeResult]:
        out = [_result([s.hyp[1:] for s in seqs], [s.score for s in seqs]) for seqs in self._beams]
        self.committed[:] = [list(r.tokens[:_common_prefix_len(r.nbest)]) for r in out]
        return out

    # ---- both --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def feed(self, encoder_chunk: torch.Tensor, ctc_chunk: torch.Tensor, nframes=None) -> Optional[List[DecodeResult]]:
        from ..._lib import PafcError
        B = self.B
        if encoder_chunk.dim() != 3 or encoder_chunk.shape[0] != B or encoder_chunk.shape[1] > self.Tmax:
            raise ValueError(f"BeamStreamer.feed: the encoder chunk must be ({B}, n <= {self.Tmax}, D)")
        if ctc_chunk.dim() != 3 or ctc_chunk.shape[:2] != encoder_chunk.shape[:2] or ctc_chunk.device != encoder_chunk.device:
            raise ValueError("BeamStreamer.feed: the CTC chunk must be (B, n, V) on the encoder chunk's device")
        n = encoder_chunk.shape[1]
        on_gpu = encoder_chunk.is_cuda and self.beam <= 16
        if self._device is None:
            if self.frame_body == "kernels":                  # never a fallback: CPU tensors and beam > 16 are named too
                from ...hip_ops import _shape_like, rnnt_beam_body_unmet
                like = _shape_like(B, self.Tmax, encoder_chunk.shape[2], encoder_chunk.device)
                unmet = rnnt_beam_body_unmet(self.bs.predictor, self.bs.joint, like, self.beam)
                if unmet is not None:
                    raise PafcError(f"BeamStreamer: frame_body 'kernels': {unmet}")
            self._device = encoder_chunk.device
            if on_gpu:
                self._make_gpu(encoder_chunk, ctc_chunk)
        elif encoder_chunk.device != self._device:
            raise ValueError(f"BeamStreamer.feed: the stream began on {self._device}, this chunk is on {encoder_chunk.device}")
        if self._gpu is not None and isinstance(nframes, torch.Tensor) and nframes.is_cuda:
            if nframes.shape != (B,):
                raise ValueError(f"BeamStreamer.feed: nframes must be ({B},)")
            nf, over = nframes, []                          # the counts stay on the device: the kernel's flags report overflow
        else:
            nf = [n] * B if nframes is None else [max(0, min(n, int(v))) for v in torch.as_tensor(nframes).tolist()]
            if len(nf) != B:
                raise ValueError(f"BeamStreamer.feed: nframes must be ({B},)")
            over = [b for b in range(B) if nf[b] > 0 and (self._full[b] or self._frames[b] + nf[b] > self.max_total)]
            for b in over:
                self._full[b] = True
        if self._gpu is not None:
            self._feed_gpu(encoder_chunk, ctc_chunk, nf, n)   # (a row in `over` is refused by the kernel itself)
        else:
            self._feed_host(encoder_chunk, ctc_chunk, [0 if b in over else v for b, v in enumerate(nf)])
        if isinstance(nf, list):
            for b in range(B):
                if b not in over:
                    self._frames[b] += nf[b]
        self._last = None
        out = None
        if self.want_partials:
            if self._gpu is not None:
                # a list grows by at most one token per frame: the tails fit in the longest tail so far + n
                out = self._last = self._drain_gpu(self._tail() + n)
                over = sorted(set(over) | {b for b in range(B) if self._overflow[b] and not isinstance(nf, list)})
            else:
                out = self._last = self._host_results()
        if over:
            raise PafcError(f"BeamStreamer.feed: rows {over} would pass max_total_frames = {self.max_total} and took no frames; "
                            "reset them (the other rows were served)")
        return out

    def partials(self) -> List[DecodeResult]:
        """Per row the result if the stream ended here (what the last feed returned, when it returned partials)."""
        if self._last is not None:
            return self._last
        return self.results()

    def results(self) -> List[DecodeResult]:
        if self._gpu is not None:
            # with partials switched off no drain has bounded the tails: a list holds at most one token per frame
            ld = self._tail() if self.want_partials else max(1, min(self.max_total, max(self._frames) or self.max_total))
            return self._drain_gpu(max(1, ld))
        return self._host_results()
