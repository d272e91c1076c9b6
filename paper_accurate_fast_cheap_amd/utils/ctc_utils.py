"""Time stamps from CTC alignments (reference: wenet/utils/ctc_utils.py: gen_ctc_peak_time, gen_timestamps_from_peak,
force_align).  force_align is the one-utterance front end of transformer.search.ctc_forced_align: the kernel for a GPU tensor,
the host recursion for a host tensor."""
from typing import List, Tuple

import torch


def gen_ctc_peak_time(hyp: List[int], blank_id: int = 0) -> List[int]:
    """The first frame of every run of a non-blank token in a frame-level alignment."""
    times = []
    prev = None
    for t, tok in enumerate(hyp):
        if tok != prev and tok != blank_id:
            times.append(t)
        prev = tok
    return times


def gen_timestamps_from_peak(peaks: List[int], max_duration: float, frame_rate: float = 0.04,
                             max_token_duration: float = 1.0) -> List[Tuple[float, float]]:
    """(start, end) seconds per token: a token reaches from the midpoint towards its left neighbour's peak to the midpoint
    towards its right neighbour's, at most max_token_duration / 2 either side of its own peak, inside [0, max_duration].
    The arithmetic is written in the reference's order, so the floats are the reference's."""
    half = max_token_duration / 2
    n = len(peaks)
    out = []
    for i, p in enumerate(peaks):
        start = max(0, p * frame_rate - half) if i == 0 else max((peaks[i - 1] + p) / 2 * frame_rate, p * frame_rate - half)
        end = (min(max_duration, p * frame_rate + half) if i == n - 1
               else min((p + peaks[i + 1]) / 2 * frame_rate, p * frame_rate + half))
        out.append((start, end))
    return out


def force_align(ctc_probs: torch.Tensor, y: torch.Tensor, blank_id=0) -> List[int]:
    """The token of every frame on the best CTC path of `y` through ctc_probs (T, V) log-probabilities.  Where the
    reference's path does not wrap from state 0 to the last state (its index -1, see DESIGN.md "CTC forced alignment"), this is
    the reference's list; where `y` cannot be aligned the list is empty."""
    from ..transformer.search import ctc_forced_align
    y = torch.as_tensor(y, dtype=torch.long, device=ctc_probs.device).reshape(1, -1)
    lens = torch.tensor([ctc_probs.shape[0]], device=ctc_probs.device)
    ylens = torch.tensor([y.shape[1]], device=ctc_probs.device)
    results, align = ctc_forced_align(ctc_probs.unsqueeze(0), lens, y, ylens, blank_id, return_alignment=True)
    return align[0].tolist() if results[0].ok else []
