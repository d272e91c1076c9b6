"""CTC greedy and prefix beam search (reference: wenet/transformer/search.py:106-248,
wenet/utils/ctc_utils.py:22-32, wenet/utils/common.py:355-363).  Token ids are the bit-exact parity bar."""
import math
from collections import defaultdict
from typing import List, Optional

import torch

from ..utils.mask import make_pad_mask


class DecodeResult:
    def __init__(self, tokens: List[int], score: float = 0.0, confidence: float = 0.0, tokens_confidence=None,
                 times=None, nbest: Optional[List[List[int]]] = None, nbest_scores: Optional[List[float]] = None,
                 nbest_times=None):
        self.tokens = tokens
        self.score = score
        self.confidence = confidence
        self.tokens_confidence = tokens_confidence
        self.times = times
        self.nbest = nbest
        self.nbest_scores = nbest_scores
        self.nbest_times = nbest_times


def log_add(args: List[float]) -> float:
    """Stable log-sum-exp over python floats (common.py:355-363)."""
    if all(a == -float("inf") for a in args):
        return -float("inf")
    a_max = max(args)
    return a_max + math.log(sum(math.exp(a - a_max) for a in args))


def remove_duplicates_and_blank(hyp: List[int], blank_id: int = 0) -> List[int]:
    new_hyp: List[int] = []
    cur = 0
    while cur < len(hyp):
        if hyp[cur] != blank_id:
            new_hyp.append(hyp[cur])
        prev = cur
        while cur < len(hyp) and hyp[cur] == hyp[prev]:
            cur += 1
    return new_hyp


def ctc_greedy_search(ctc_probs: torch.Tensor, ctc_lens: torch.Tensor, blank_id: int = 0, defer: bool = False):
    """search.py:106-121.  On the GPU the argmax, the padding rule and the collapse run in two kernels
    (``pafc_ctc_greedy``) and only the collapsed ids come back -- two small copies for the whole batch instead of a
    (B, T) copy and a Python loop per frame.  Host tensors take the reference's own steps below.
    defer (GPU only): return a zero-argument function that fetches the List[DecodeResult] -- the device work is queued
    now, the host waits for it only when the function is called, so several batches can be in flight."""
    if ctc_probs.is_cuda:
        from ..hip_ops import ctc_greedy
        tokens, ntok = ctc_greedy(ctc_probs.contiguous(), ctc_lens.to(ctc_probs.device), blank_id)
        if defer:       # nothing here may wait for the device (a boolean-mask gather would): whole rows come back later
            def fetch() -> List[DecodeResult]:
                rows, counts = tokens.tolist(), ntok.tolist()
                return [DecodeResult(r[:n]) for r, n in zip(rows, counts)]
            return fetch
        keep = torch.arange(tokens.shape[1], device=tokens.device)[None, :] < ntok[:, None]
        flat = tokens[keep].tolist()          # all utterances back to back
        counts = ntok.tolist()
        out, pos = [], 0
        for n in counts:
            out.append(DecodeResult(flat[pos:pos + n]))
            pos += n
        return out
    batch_size, maxlen = ctc_probs.shape[:2]
    topk_index = ctc_probs.argmax(dim=2)  # == topk(1): ties resolve to the lowest index in both
    mask = make_pad_mask(ctc_lens, maxlen)
    topk_index = topk_index.masked_fill(mask, blank_id)
    hyps = topk_index.tolist()  # ONE device->host copy, then the reference's collapse per utterance
    return [DecodeResult(remove_duplicates_and_blank(h, blank_id)) for h in hyps]


class _PrefixScore:
    """Score of one prefix in one frame (search.py:59-103): blank-ending / non-blank-ending log-probabilities, the
    viterbi scores and frame lists of both endings, the probability of the current token in this frame, and the context
    graph state with its accumulated bonus."""
    __slots__ = ("s", "ns", "v_s", "v_ns", "cur_token_prob", "times_s", "times_ns", "context_state", "context_score",
                 "has_context")

    def __init__(self, s: float = -float("inf"), ns: float = -float("inf"), v_s: float = -float("inf"),
                 v_ns: float = -float("inf"), context_state=None, context_score: float = 0.0):
        self.s = s
        self.ns = ns
        self.v_s = v_s
        self.v_ns = v_ns
        self.cur_token_prob = -float("inf")
        self.times_s: List[int] = []
        self.times_ns: List[int] = []
        self.context_state = context_state
        self.context_score = context_score
        self.has_context = False

    def score(self) -> float:
        return log_add([self.s, self.ns])

    def viterbi_score(self) -> float:
        return self.v_s if self.v_s > self.v_ns else self.v_ns

    def times(self) -> List[int]:
        return self.times_s if self.v_s > self.v_ns else self.times_ns

    def total_score(self) -> float:
        return self.score() + self.context_score

    def copy_context(self, other: "_PrefixScore"):
        self.context_score = other.context_score
        self.context_state = other.context_state

    def update_context(self, graph, other: "_PrefixScore", token: int):
        self.copy_context(other)
        score, state = graph.forward_one_step(other.context_state, token)
        self.context_score += score
        self.context_state = state


def ctc_prefix_beam_search(ctc_probs: torch.Tensor, ctc_lens: torch.Tensor, beam_size: int, context_graph=None,
                           blank_id: int = 0) -> List[DecodeResult]:
    """search.py:124-248.  The per-frame top-`beam` tokens of the WHOLE batch are taken in one device op and
    copied to the host once (the reference calls .item() per candidate); the prefix bookkeeping then follows the
    reference's loop order exactly, because that order decides ties in its stable sort and the viterbi frame lists.
    context_graph (utils.context_graph.ContextGraph, or None): hotword biasing -- the second prune ranks on
    score + context bonus, and at the end each survivor's bonus is replaced by its finalize() value.  Every result
    carries the frame of each token of its viterbi path (times / nbest_times)."""
    B = ctc_probs.shape[0]
    k = min(beam_size, ctc_probs.shape[-1])
    top_p, top_i = ctc_probs.float().topk(k, dim=-1)          # (B, T, k)
    if ctc_probs.is_cuda and beam_size <= 16:
        # GPU-resident: one wave per utterance walks the frames (pafc_ctc_prefix_beam_search_ex); only the n-best lists
        # and their frames come back.  Same candidates, merges, tie order and context steps as the loop below; float64
        # scores from the device's exp / log agree with the host's to a few ulps.
        from ..hip_ops import ctc_prefix_beam
        tables = None if context_graph is None else context_graph.device_tables(ctc_probs.device)
        toks, lens_n, scores, times = ctc_prefix_beam(top_p.contiguous(), top_i.contiguous(),
                                                      ctc_lens.to(ctc_probs.device), beam_size, blank_id,
                                                      graph_tables=tables, want_times=True)
        lens_h, scores_h = lens_n.tolist(), scores.tolist()
        maxlen = max(1, int(lens_n.max()))
        toks_h = toks[:, :, :maxlen].tolist()
        ntim = (times >= 0).sum(-1)                           # a frame list ends at its first -1
        times_h = times[:, :, :max(1, int(ntim.max()))].tolist()
        ntim_h = ntim.tolist()
        results = []
        for b in range(B):
            live = [n for n in range(beam_size) if lens_h[b][n] >= 0]
            nbest = [tuple(toks_h[b][n][:lens_h[b][n]]) for n in live]
            nsc = [scores_h[b][n] for n in live]
            ntimes = [times_h[b][n][:ntim_h[b][n]] for n in live]
            results.append(DecodeResult(tokens=nbest[0], score=nsc[0], times=ntimes[0], nbest=nbest, nbest_scores=nsc,
                                        nbest_times=ntimes))
        return results
    top_p, top_i, lens = top_p.cpu().tolist(), top_i.cpu().tolist(), [int(v) for v in ctc_lens.tolist()]
    graph = context_graph
    results = []
    for b in range(B):
        cur = [(tuple(), _PrefixScore(s=0.0, ns=-float("inf"), v_s=0.0, v_ns=0.0,
                                      context_state=None if graph is None else graph.root, context_score=0.0))]
        for t in range(lens[b]):
            nxt = defaultdict(_PrefixScore)
            for prob, u in zip(top_p[b][t], top_i[b][t]):
                for prefix, ps in cur:
                    last = prefix[-1] if len(prefix) > 0 else None
                    if u == blank_id:
                        n = nxt[prefix]
                        n.s = log_add([n.s, ps.score() + prob])
                        n.v_s = ps.viterbi_score() + prob
                        n.times_s = ps.times().copy()
                        if graph is not None and not n.has_context:
                            n.copy_context(ps)
                            n.has_context = True
                    elif u == last:
                        n1 = nxt[prefix]                       # *uu -> *u
                        n1.ns = log_add([n1.ns, ps.ns + prob])
                        # the reference assigns a misspelt attribute here (search.py:186), so v_ns stays as it is
                        if n1.v_ns < ps.v_ns + prob and n1.cur_token_prob < prob:
                            n1.cur_token_prob = prob
                            n1.times_ns = ps.times_ns.copy()
                            n1.times_ns[-1] = t
                        if graph is not None and not n1.has_context:
                            n1.copy_context(ps)
                            n1.has_context = True
                        n2 = nxt[prefix + (u,)]                # *u-u -> *uu
                        n2.ns = log_add([n2.ns, ps.s + prob])
                        if n2.v_ns < ps.v_s + prob:
                            n2.v_ns = ps.v_s + prob
                            n2.cur_token_prob = prob
                            n2.times_ns = ps.times_s.copy()
                            n2.times_ns.append(t)
                        if graph is not None and not n2.has_context:
                            n2.update_context(graph, ps, u)
                            n2.has_context = True
                    else:
                        n = nxt[prefix + (u,)]
                        n.ns = log_add([n.ns, ps.score() + prob])
                        if n.v_ns < ps.viterbi_score() + prob:
                            n.v_ns = ps.viterbi_score() + prob
                            n.cur_token_prob = prob
                            n.times_ns = ps.times().copy()
                            n.times_ns.append(t)
                        if graph is not None and not n.has_context:
                            n.update_context(graph, ps, u)
                            n.has_context = True
            cur = sorted(nxt.items(), key=lambda x: x[1].total_score(), reverse=True)[:beam_size]
        if graph is not None:            # back off partial matches; the order is NOT revisited (search.py:224-231)
            for _, ps in cur:
                ps.context_score, ps.context_state = graph.finalize(ps.context_state)
        nbest = [tuple(y[0]) for y in cur]
        nbest_scores = [y[1].total_score() for y in cur]
        nbest_times = [y[1].times() for y in cur]
        results.append(DecodeResult(tokens=nbest[0], score=nbest_scores[0], times=nbest_times[0], nbest=nbest,
                                    nbest_scores=nbest_scores, nbest_times=nbest_times))
    return results
