"""RNN-T greedy search (reference: wenet/transducer/search/greedy_search.py, `basic_greedy_search`, behind
`Transducer.greedy_search`, wenet/transducer/transducer.py:427-472, and the recognizers' `--modes rnnt_greedy_search`).

`basic_greedy_search` is the reference's function: one utterance, device-agnostic torch ops, a host read per decision.  It is
the path for CPU tensors and the comparison path on the GPU.  `batch_greedy_search` decodes a batch: GPU tensors go to the
lockstep kernels of csrc/rnnt_greedy.hip (hip_ops.rnnt_greedy_search) and raise PafcError naming the unmet condition instead of
falling back to framework ops; CPU tensors run `basic_greedy_search` per utterance.  `GreedyStreamer` decodes streams chunk
by chunk with the decoder state carried between chunks (the reference's "TODO(Mddct): make t in chunk for streamming",
greedy_search.py:49): hip_ops.RnntGreedyStream on the GPU, the reference's loop resumed per chunk on the CPU."""
from typing import List

import torch

from ...transformer.search import DecodeResult


def basic_greedy_search(model: torch.nn.Module, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor,
                        n_steps: int = 64) -> List[List[int]]:
    """greedy_search.py:6-60 for B = 1: per decision, a predictor step if the last decision was not blank, the joint on
    encoder frame t, argmax of log_softmax; a non-blank is emitted and commits the predictor state, a blank (or the n_steps-th
    symbol of a frame) moves to the next frame.  Returns [tokens]."""
    return [_greedy_one(model, encoder_out, encoder_out_lens, n_steps, False)[0]]


class _RowState:
    """The reference's loop variables for one stream (greedy_search.py:26-36), kept between calls of _greedy_resume."""

    def __init__(self, model, device):
        dt = model.predictor.embed.weight.dtype        # (the reference's padding and zero state are fp32: bf16 models)
        self.padding = torch.zeros(1, 1, dtype=dt).to(device)
        self.pred_input = torch.tensor([model.blank], device=device).reshape(1, 1)
        self.cache = [c.to(dt) for c in model.predictor.init_state(1, method="zero", device=device)]
        self.new_cache: List[torch.Tensor] = []
        self.pred_out = None
        self.prev_out_nblk = True
        self.k = 0                 # symbols emitted in the current frame (the reference's per_frame_noblk)
        self.base = 0              # absolute index of frame 0 of the next call's frames
        self.score = 0.0


def _greedy_resume(model, r: _RowState, encoder_out, T_b: int, n_steps: int, with_path: bool):
    """The reference's loop over frames [0, T_b) of encoder_out (1, T, D), resumed from r and left in r.  Returns the tokens
    and their absolute frames (r.base + t); with_path also adds log p of every decision (blanks included: what the kernels
    report) to r.score.  A call over all frames of an utterance is the reference's basic_greedy_search; calls over
    consecutive pieces of it make the same decisions, since each call ends at a frame boundary (k = 0)."""
    hyps, times = [], []
    t = 0
    while t < T_b:
        encoder_out_step = encoder_out[:, t:t + 1, :]
        if r.prev_out_nblk:
            step_outs = model.predictor.forward_step(r.pred_input, r.padding, r.cache)
            r.pred_out, r.new_cache = step_outs[0], step_outs[1]
        joint_out_step = model.joint(encoder_out_step, r.pred_out)
        joint_out_probs = joint_out_step.log_softmax(dim=-1)
        joint_out_max = joint_out_probs.argmax(dim=-1).squeeze()
        if with_path:
            r.score += joint_out_probs.reshape(-1)[joint_out_max].item()
        if joint_out_max != model.blank:
            hyps.append(joint_out_max.item())
            times.append(r.base + t)
            r.prev_out_nblk = True
            r.k = r.k + 1
            r.pred_input = joint_out_max.reshape(1, 1)
            r.cache = r.new_cache
        if joint_out_max == model.blank or r.k >= n_steps:
            if joint_out_max == model.blank:
                r.prev_out_nblk = False
            t = t + 1
            r.k = 0
    r.base += T_b
    return hyps, times


def _greedy_one(model, encoder_out, encoder_out_lens, n_steps: int, with_path: bool):
    """The reference's loop over one whole utterance: (tokens, frames, path score -- 0.0 without with_path)."""
    r = _RowState(model, encoder_out.device)
    hyps, times = _greedy_resume(model, r, encoder_out, int(encoder_out_lens), n_steps, with_path)
    return hyps, times, r.score


def batch_greedy_search(model: torch.nn.Module, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor,
                        n_steps: int = 64) -> List[DecodeResult]:
    """Greedy search of every utterance of (B, T, D) encoder_out: DecodeResult(tokens, score = path log-probability, times =
    frame index of each token).  GPU: the lockstep kernels.  CPU: the reference's loop per utterance."""
    if encoder_out.is_cuda:
        from ... import hip_ops
        from ..._lib import PafcError
        unmet = hip_ops.rnnt_greedy_unmet(model.predictor, model.joint, encoder_out, n_steps)
        if unmet is not None:
            raise PafcError(f"rnnt_greedy_search: {unmet}")
        toks, times, scores = hip_ops.rnnt_greedy_search(model.predictor, model.joint, encoder_out, encoder_out_lens,
                                                         model.blank, n_steps)
        return [DecodeResult(tokens=tk, score=sc, times=tm) for tk, tm, sc in zip(toks, times, scores)]
    results = []
    for b, T_b in enumerate(encoder_out_lens.tolist()):
        toks, times, score = _greedy_one(model, encoder_out[b:b + 1], T_b, n_steps, True)
        results.append(DecodeResult(tokens=toks, score=score, times=times))
    return results


class GreedyStreamer:
    """Greedy search of `batch_size` streams fed chunk by chunk, the decoder state carried between chunks.  Over a stream,
    the tokens, absolute frames and scores equal batch_greedy_search of the concatenated frames (on the GPU bit for bit given
    the same enc_ffn rows: DESIGN.md section 4).

    feed(encoder_chunk (B, n <= max_frames, D), nframes=None) decodes row b's first nframes[b] frames (default n; 0 = the row
    sits the chunk out) and returns the new tokens per row; their absolute frames are on `.last_frames`.  reset(rows) restarts
    rows (all when None) from their next chunk on.  results() is, per row, everything since its reset.  GPU tensors run on
    hip_ops.RnntGreedyStream (PafcError naming the unmet condition otherwise, never a fallback); CPU tensors run the
    reference's loop (_greedy_resume, the same function the offline CPU path calls once per utterance) chunk after chunk."""

    def __init__(self, model: torch.nn.Module, batch_size: int, max_frames: int, n_steps: int = 64):
        self.model, self.B, self.Tmax, self.n_steps = model, batch_size, max_frames, n_steps
        dev = model.joint.ffn_out.weight.device
        self.device = dev
        self._gpu = None
        if dev.type == "cuda":
            from ... import hip_ops
            self._gpu = hip_ops.RnntGreedyStream(model.predictor, model.joint, batch_size, max_frames, n_steps, model.blank)
        elif max_frames < 1:
            raise ValueError("GreedyStreamer: max_frames must be >= 1")
        self._hyps: List[List[int]] = [[] for _ in range(batch_size)]
        self._times: List[List[int]] = [[] for _ in range(batch_size)]
        self._rows: List[_RowState] = []
        self.last_frames: List[List[int]] = [[] for _ in range(batch_size)]
        self.reset()

    def reset(self, rows=None):
        rows = range(self.B) if rows is None else list(rows)
        for b in rows:
            self._hyps[b], self._times[b] = [], []
        if self._gpu is not None:
            self._gpu.reset(None if rows == range(self.B) else rows)
            return
        if not self._rows:
            self._rows = [_RowState(self.model, self.device) for _ in range(self.B)]
        for b in rows:
            self._rows[b] = _RowState(self.model, self.device)

    def feed(self, encoder_chunk: torch.Tensor, nframes=None) -> List[List[int]]:
        n = encoder_chunk.shape[1]
        if encoder_chunk.shape[0] != self.B or n > self.Tmax:
            raise ValueError(f"GreedyStreamer.feed: the chunk must be ({self.B}, n <= {self.Tmax}, D)")
        if self._gpu is not None:
            toks, frames = self._gpu.feed(encoder_chunk, nframes)
        else:
            nf = [n] * self.B if nframes is None else [max(0, min(n, int(v))) for v in torch.as_tensor(nframes).tolist()]
            toks, frames = [], []
            for b in range(self.B):
                tk, fr = _greedy_resume(self.model, self._rows[b], encoder_chunk[b:b + 1], nf[b], self.n_steps, True)
                toks.append(tk)
                frames.append(fr)
        for b in range(self.B):
            self._hyps[b] += toks[b]
            self._times[b] += frames[b]
        self.last_frames = frames
        return toks

    def results(self) -> List[DecodeResult]:
        scores = self._gpu.score if self._gpu is not None else [r.score for r in self._rows]
        return [DecodeResult(tokens=list(self._hyps[b]), score=scores[b], times=list(self._times[b])) for b in range(self.B)]
