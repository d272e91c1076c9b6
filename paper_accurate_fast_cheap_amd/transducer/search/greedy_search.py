"""RNN-T greedy search (reference: wenet/transducer/search/greedy_search.py, `basic_greedy_search`, behind
`Transducer.greedy_search`, wenet/transducer/transducer.py:427-472, and the recognizers' `--modes rnnt_greedy_search`).

`basic_greedy_search` is the reference's function: one utterance, device-agnostic torch ops, a host read per decision.  It is
the path for CPU tensors and the comparison path on the GPU.  `batch_greedy_search` decodes a batch: GPU tensors go to the
lockstep kernels of csrc/rnnt_greedy.hip (hip_ops.rnnt_greedy_search) and raise PafcError naming the unmet condition instead of
falling back to framework ops; CPU tensors run `basic_greedy_search` per utterance."""
from typing import List

import torch

from ...transformer.search import DecodeResult


def basic_greedy_search(model: torch.nn.Module, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor,
                        n_steps: int = 64) -> List[List[int]]:
    """greedy_search.py:6-60 for B = 1: per decision, a predictor step if the last decision was not blank, the joint on
    encoder frame t, argmax of log_softmax; a non-blank is emitted and commits the predictor state, a blank (or the n_steps-th
    symbol of a frame) moves to the next frame.  Returns [tokens]."""
    return [_greedy_one(model, encoder_out, encoder_out_lens, n_steps, False)[0]]


def _greedy_one(model, encoder_out, encoder_out_lens, n_steps: int, with_path: bool):
    """The reference's loop; with_path also records each token's frame and the path score (the sum of log p over every
    decision, blanks included: what the kernels report)."""
    dt = model.predictor.embed.weight.dtype            # (the reference's padding and zero state are fp32: bf16 models)
    padding = torch.zeros(1, 1, dtype=dt).to(encoder_out.device)
    pred_input_step = torch.tensor([model.blank], device=encoder_out.device).reshape(1, 1)
    cache = [c.to(dt) for c in model.predictor.init_state(1, method="zero", device=encoder_out.device)]
    new_cache: List[torch.Tensor] = []
    t = 0
    hyps, times, score = [], [], 0.0
    prev_out_nblk = True
    pred_out_step = None
    per_frame_max_noblk = n_steps
    per_frame_noblk = 0
    while t < encoder_out_lens:
        encoder_out_step = encoder_out[:, t:t + 1, :]
        if prev_out_nblk:
            step_outs = model.predictor.forward_step(pred_input_step, padding, cache)
            pred_out_step, new_cache = step_outs[0], step_outs[1]
        joint_out_step = model.joint(encoder_out_step, pred_out_step)
        joint_out_probs = joint_out_step.log_softmax(dim=-1)
        joint_out_max = joint_out_probs.argmax(dim=-1).squeeze()
        if with_path:
            score += joint_out_probs.reshape(-1)[joint_out_max].item()
        if joint_out_max != model.blank:
            hyps.append(joint_out_max.item())
            times.append(t)
            prev_out_nblk = True
            per_frame_noblk = per_frame_noblk + 1
            pred_input_step = joint_out_max.reshape(1, 1)
            cache = new_cache
        if joint_out_max == model.blank or per_frame_noblk >= per_frame_max_noblk:
            if joint_out_max == model.blank:
                prev_out_nblk = False
            t = t + 1
            per_frame_noblk = 0
    return hyps, times, score


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
