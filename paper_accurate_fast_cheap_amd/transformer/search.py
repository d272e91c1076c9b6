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
                 nbest_times=None, end_times=None, tokens_info=None, ok: bool = True,
                 nbest_td_scores: Optional[List[float]] = None, nbest_attn_scores: Optional[List[float]] = None,
                 stats: Optional[dict] = None, trace: Optional[dict] = None):
        self.tokens = tokens
        self.score = score
        self.confidence = confidence
        self.tokens_confidence = tokens_confidence
        self.times = times
        self.nbest = nbest
        self.nbest_scores = nbest_scores
        self.nbest_times = nbest_times
        self.end_times = end_times          # forced alignment: the last frame of every token (times: the first)
        self.tokens_info = tokens_info      # forced alignment: (start, end) seconds per token
        self.ok = ok                        # forced alignment: False when the labels cannot be aligned to the frames
        self.nbest_td_scores = nbest_td_scores    # transducer rescoring: log p(y | x) of every entry of nbest, in its order
        self.nbest_attn_scores = nbest_attn_scores    # attention rescoring: the attention decoder's score of every entry of nbest
        self.stats = stats                  # attention beam search, kernels backend: steps, host reads, launches per step
        self.trace = trace                  # attention beam search with return_trace: parent / token / score per step and slot


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


class _BeamRow:
    """The host loop's variables for one stream, kept between calls of _prefix_beam_resume: the current beam (prefix,
    score) best first, and the number of frames consumed."""
    __slots__ = ("cur", "base")

    def __init__(self, graph):
        self.cur = [(tuple(), _PrefixScore(s=0.0, ns=-float("inf"), v_s=0.0, v_ns=0.0,
                                           context_state=None if graph is None else graph.root, context_score=0.0))]
        self.base = 0


def _prefix_beam_resume(r: _BeamRow, top_p, top_i, nframes: int, beam_size: int, graph, blank_id: int):
    """The reference's loop (search.py:150-222) over frames [0, nframes) of one utterance's top-k lists, resumed from r and left
    in r; the frame lists record r.base + j.  One call over all frames is the offline search; calls over consecutive
    pieces do the same arithmetic in the same order, since nothing but the beam lives from one frame to the next."""
    cur = r.cur
    for j in range(nframes):
        t = r.base + j
        nxt = defaultdict(_PrefixScore)
        for prob, u in zip(top_p[j], top_i[j]):
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
    r.cur = cur
    r.base += nframes


def _prefix_beam_result(r: _BeamRow, graph) -> DecodeResult:
    """The n-best of a stream that ends here.  With a graph each survivor's bonus is replaced by its finalize() value
    (partial matches are backed off; the order is NOT revisited, search.py:224-231) -- on a copy, r goes on unchanged."""
    cur = r.cur
    nbest = [tuple(y[0]) for y in cur]
    if graph is not None:
        nbest_scores = [y[1].score() + graph.finalize(y[1].context_state)[0] for y in cur]
    else:
        nbest_scores = [y[1].total_score() for y in cur]
    nbest_times = [list(y[1].times()) for y in cur]
    return DecodeResult(tokens=nbest[0], score=nbest_scores[0], times=nbest_times[0], nbest=nbest,
                        nbest_scores=nbest_scores, nbest_times=nbest_times)


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
    results = []
    for b in range(B):
        r = _BeamRow(context_graph)
        _prefix_beam_resume(r, top_p[b], top_i[b], lens[b], beam_size, context_graph, blank_id)
        results.append(_prefix_beam_result(r, context_graph))
    return results


def _forced_align_host(lp: torch.Tensor, y: List[int], blank_id: int):
    """One utterance of ctc_forced_align on the host: lp (T, V) float32, the frames and labels without padding ->
    (align, first, last, score, ok).  The recursion of include/pafc_search.h (pafc_ctc_align), a frame at a time over all
    states at once: the same fp32 adds, candidates in the same order, a later one only when strictly greater."""
    T, V = lp.shape
    L = len(y)
    bad = (-1.0 * float("inf"), False)
    if T <= 0 or any(c == blank_id or c < 0 or c >= V for c in y):
        return [-1] * T, [-1] * L, [-1] * L, *bad
    if L + sum(1 for i in range(1, L) if y[i] == y[i - 1]) > T:
        return [-1] * T, [-1] * L, [-1] * L, *bad
    S = 2 * L + 1
    ext = torch.full((S,), blank_id, dtype=torch.long)
    ext[1::2] = torch.tensor(y, dtype=torch.long)
    skip = torch.zeros(S, dtype=torch.bool)
    skip[2:] = (ext[2:] != blank_id) & (ext[2:] != ext[:-2])
    ninf = torch.full((2,), -float("inf"), dtype=torch.float32)
    alpha = torch.full((S,), -float("inf"), dtype=torch.float32)
    alpha[:2] = lp[0, ext[:2]]
    back = torch.zeros(T, S, dtype=torch.int8)
    for t in range(1, T):
        padded = torch.cat([ninf, alpha])                       # two guard entries in front, as the kernel keeps them
        a1 = padded[1:S + 1]
        a2 = torch.where(skip, padded[:S], ninf[0])
        m1 = a1 > alpha
        best = torch.where(m1, a1, alpha)
        m2 = a2 > best
        best = torch.where(m2, a2, best)
        back[t] = torch.where(m2, 2, m1.to(torch.int8))
        alpha = best + lp[t, ext]
    s = S - 1
    if S >= 2 and bool(alpha[S - 2] > alpha[S - 1]):
        s = S - 2
    score = float(alpha[s])
    if score == -float("inf"):
        return [-1] * T, [-1] * L, [-1] * L, *bad
    back = back.numpy()
    ext_l = ext.tolist()
    align, first, last = [0] * T, [-1] * L, [-1] * L
    for t in range(T - 1, -1, -1):
        align[t] = ext_l[s]
        if s & 1:
            first[s >> 1] = t
            if last[s >> 1] < 0:
                last[s >> 1] = t
        s -= int(back[t, s])
    return align, first, last, score, True


def ctc_forced_align(ctc_probs: torch.Tensor, ctc_lens: torch.Tensor, ys: torch.Tensor, ys_lens: torch.Tensor, blank_id: int = 0,
                     return_alignment: bool = False, defer: bool = False):
    """CTC forced alignment of a batch (the reference aligns one utterance at a time on the host: force_align,
    wenet/utils/ctc_utils.py:105-161, and builds this result in wenet/cli/model.py:92-104): the best path of the labels
    ys[b, :ys_lens[b]] through ctc_probs[b, :ctc_lens[b]] (log-probabilities, float32 or bfloat16).  Each DecodeResult carries
    tokens = the labels, score = the path's log-probability, times = the first frame of every token (gen_ctc_peak_time of the
    alignment), end_times = the last, and nbest / nbest_scores / nbest_times holding that one entry.  Labels that cannot be
    aligned (more labels plus adjacent repeats than frames, a blank or out-of-vocabulary label, no path of finite score,
    ctc_lens[b] outside [1, T] or ys_lens[b] outside [0, Lmax]) give ok = False, score = -inf and times = []; tokens then holds
    the labels with ys_lens[b] clamped to [0, Lmax].  Host and GPU paths follow the same rule.  State 0 of the lattice has itself as its only predecessor, which the reference
    gets wrong (DESIGN.md "CTC forced alignment"); wherever the reference's path collapses to the labels this is its path.
    return_alignment: -> (results, (B, T) int32 token of every frame, -1 beyond an utterance and in rows that are not ok).
    GPU tensors run pafc_ctc_align (one launch; PafcError if it cannot, never a fallback); host tensors the recursion above.
    defer (GPU only): return a zero-argument function that fetches the result; nothing waits for the device before it is called."""
    B, T = ctc_probs.shape[:2]

    def pack(ys_h, first_h, last_h, score_h, ok_h):
        out = []
        for b in range(B):
            y = list(ys_h[b])
            if ok_h[b]:
                out.append(DecodeResult(tokens=y, score=score_h[b], times=first_h[b][:len(y)], nbest=[y], nbest_scores=[score_h[b]],
                                        nbest_times=[first_h[b][:len(y)]], end_times=last_h[b][:len(y)]))
            else:
                out.append(DecodeResult(tokens=y, score=-float("inf"), times=[], nbest=[y], nbest_scores=[-float("inf")],
                                        nbest_times=[[]], end_times=[], ok=False))
        return out

    if ctc_probs.is_cuda:
        from ..hip_ops import ctc_align
        dev = ctc_probs.device
        ys_d, yl_d = ys.to(dev), ys_lens.to(dev)
        align, first, last, score, ok = ctc_align(ctc_probs, ctc_lens.to(dev), ys_d, yl_d, blank_id)

        def fetch():
            yl = [max(0, min(int(n), ys_d.shape[1])) for n in yl_d.tolist()]
            ys_h = [row[:n] for row, n in zip(ys_d.tolist(), yl)]
            res = pack(ys_h, first.tolist(), last.tolist(), score.tolist(), ok.tolist())
            return (res, align) if return_alignment else res
        return fetch if defer else fetch()
    lp = ctc_probs.float()
    lens = [int(v) for v in ctc_lens.tolist()]
    yl_raw = [int(n) for n in ys_lens.tolist()]
    yl = [max(0, min(n, ys.shape[1])) for n in yl_raw]
    ys_h = [row[:n] for row, n in zip(ys.tolist(), yl)]
    align = torch.full((B, T), -1, dtype=torch.int32)
    firsts, lasts, scores, oks = [], [], [], []
    for b in range(B):
        n = lens[b] if 0 <= lens[b] <= T and yl_raw[b] == yl[b] else 0       # a length outside its tensor: no frames, not ok
        a, f, l, sc, ok = _forced_align_host(lp[b, :n], ys_h[b], blank_id)
        if ok:
            align[b, :n] = torch.tensor(a, dtype=torch.int32)
        firsts.append(f); lasts.append(l); scores.append(sc); oks.append(ok)
    res = pack(ys_h, firsts, lasts, scores, oks)
    return (res, align) if return_alignment else res


def _common_prefix_len(lists) -> int:
    n = min(len(x) for x in lists)
    for i in range(n):
        if any(x[i] != lists[0][i] for x in lists[1:]):
            return i
    return n


STREAM_MODES = ("ctc_prefix_beam_search", "ctc_greedy_search")


class CtcStreamer:
    """CTC greedy or prefix beam search of `batch_size` streams fed chunk by chunk.  Over a stream, for any cut of its
    frames into chunks, the result equals the offline function on the concatenated frames: tokens and times exactly, and
    scores bit for bit where both sides run the same arithmetic (host loop against host loop, kernel against kernel).

    feed(ctc_logp_chunk (B, n <= max_frames, V), nframes=None): row b consumes its first nframes[b] frames (default n;
    0 = the row sits the chunk out).  The chunk's top-k is taken exactly as the offline function takes it.  Returns per row
    a partial DecodeResult -- the 1-best and n-best tokens and scores if the stream ended here (with a context graph the
    finalize value is applied to a copy; greedy: the tokens and frames so far) -- without times.  `.committed` holds per
    row the tokens that can no longer change: the common prefix of the row's n-best.  Every later hypothesis extends a
    member of the beam, so a committed token is final; the list only grows.
    reset(rows=None) restarts rows (all when None) from their next chunk on.
    results(): per row the full DecodeResult, times / nbest_times included.
    max_total_frames: the most frames a row may take between resets (the beam search's node pools are sized by it and are
    not compacted: reset a row at an endpoint).  A feed that would pass it leaves that row as it was -- the row takes no
    more frames until its reset --, serves the other rows, and raises PafcError naming the rows.
    GPU tensors run on hip_ops.CtcBeamStream / CtcGreedyStream (PafcError otherwise, never a fallback); CPU tensors, and
    beam_size > 16 as in the offline function, run the host loop (_prefix_beam_resume, the function the offline host
    path calls once per utterance)."""

    def __init__(self, batch_size: int, max_frames: int, mode: str = "ctc_prefix_beam_search", beam_size: int = 10,
                 context_graph=None, blank_id: int = 0, max_total_frames: int = 4096):
        if mode not in STREAM_MODES:
            raise ValueError(f"CtcStreamer: mode must be one of {STREAM_MODES}, got {mode!r}")
        if batch_size < 1 or max_frames < 1 or max_total_frames < 1 or beam_size < 1:
            raise ValueError("CtcStreamer: batch_size, max_frames, max_total_frames and beam_size must be >= 1")
        self.B, self.Tmax, self.mode, self.beam, self.graph = batch_size, max_frames, mode, beam_size, context_graph
        self.blank, self.max_total = blank_id, max_total_frames
        self.greedy = mode == "ctc_greedy_search"
        self._gpu = None                                   # made by the first feed of a GPU tensor
        self._device = None
        self.committed: List[List[int]] = [[] for _ in range(batch_size)]
        self._rows: List[Optional[_BeamRow]] = [None] * batch_size
        self._frames = [0] * batch_size                    # frames consumed per row
        self._maxlen = [0] * batch_size                    # the longest token list of a row's beam
        self._times: List[List[int]] = [[] for _ in range(batch_size)]      # greedy: frames of the committed tokens
        self._prev = [-1] * batch_size                     # greedy on the host: the previous frame's argmax
        self._full = [False] * batch_size                  # the row was refused frames: it takes no more until its reset
        self.last_read_bytes = 0
        self.reset()

    def reset(self, rows=None):
        rows = list(range(self.B)) if rows is None else [int(b) for b in rows]
        for b in rows:
            self.committed[b], self._times[b] = [], []
            self._frames[b], self._maxlen[b], self._prev[b], self._full[b] = 0, 0, -1, False
            self._rows[b] = None if self.greedy else _BeamRow(self.graph)
        if self._gpu is not None:
            self._gpu.reset(None if len(rows) == self.B else rows)

    def _make_gpu(self, chunk: torch.Tensor):
        from .. import hip_ops
        if self.greedy:
            return hip_ops.CtcGreedyStream(self.B, self.Tmax, chunk.device, self.blank)
        tables = None if self.graph is None else self.graph.device_tables(chunk.device)
        return hip_ops.CtcBeamStream(self.B, self.Tmax, min(self.beam, chunk.shape[-1]), self.beam, chunk.device, self.blank,
                                     tables, self.max_total)

    def feed(self, ctc_logp_chunk: torch.Tensor, nframes=None) -> List[DecodeResult]:
        B = self.B
        if ctc_logp_chunk.dim() != 3 or ctc_logp_chunk.shape[0] != B or ctc_logp_chunk.shape[1] > self.Tmax:
            raise ValueError(f"CtcStreamer.feed: the chunk must be ({B}, n <= {self.Tmax}, V)")
        n = ctc_logp_chunk.shape[1]
        nf = [n] * B if nframes is None else [max(0, min(n, int(v))) for v in torch.as_tensor(nframes).tolist()]
        if len(nf) != B:
            raise ValueError(f"CtcStreamer.feed: nframes must be ({B},)")
        on_gpu = ctc_logp_chunk.is_cuda and (self.greedy or self.beam <= 16)
        if self._device is None:
            self._device = ctc_logp_chunk.device
            if on_gpu:
                self._gpu = self._make_gpu(ctc_logp_chunk)
        elif ctc_logp_chunk.device != self._device:
            raise ValueError(f"CtcStreamer.feed: the stream began on {self._device}, this chunk is on {ctc_logp_chunk.device}")
        over = [] if self.greedy else [b for b in range(B)      # (the greedy search keeps no pool)
                                      if nf[b] > 0 and (self._full[b] or self._frames[b] + nf[b] > self.max_total)]
        for b in over:
            self._full[b] = True
        if self.greedy:
            out = self._feed_greedy(ctc_logp_chunk, nf, over)
        elif self._gpu is not None:
            out = self._feed_beam_gpu(ctc_logp_chunk, nf, over)
        else:
            out = self._feed_beam_host(ctc_logp_chunk, nf, over)
        if over:
            from .._lib import PafcError
            raise PafcError(f"CtcStreamer.feed: rows {over} would pass max_total_frames = {self.max_total} and took no frames; "
                            "reset them (the other rows were served)")
        return out

    # ---- greedy ------------------------------------------------------------------------------------------------
    def _feed_greedy(self, chunk, nf, over):
        nf = [0 if b in over else v for b, v in enumerate(nf)]
        if self._gpu is not None:
            toks, frames = self._gpu.feed(chunk, nf)
        else:
            best = chunk.argmax(dim=2).tolist()            # == topk(1), as in ctc_greedy_search
            toks, frames = [], []
            for b in range(self.B):
                tk, fr, prev = [], [], self._prev[b]
                for t in range(nf[b]):
                    u = best[b][t]
                    if u != self.blank and u != prev:
                        tk.append(u)
                        fr.append(self._frames[b] + t)
                    prev = u
                self._prev[b] = prev
                toks.append(tk)
                frames.append(fr)
        for b in range(self.B):
            self.committed[b] += toks[b]
            self._times[b] += frames[b]
            self._frames[b] += nf[b]
        return self.partials()

    # ---- prefix beam search ------------------------------------------------------------------------------------
    def _feed_beam_host(self, chunk, nf, over):
        k = min(self.beam, chunk.shape[-1])
        top_p, top_i = chunk.float().topk(k, dim=-1)
        top_p, top_i = top_p.cpu().tolist(), top_i.cpu().tolist()
        for b in range(self.B):
            if nf[b] and b not in over:
                _prefix_beam_resume(self._rows[b], top_p[b], top_i[b], nf[b], self.beam, self.graph, self.blank)
                self._frames[b] += nf[b]
        return self.partials()

    def _drain_gpu(self, ld: int, want_times: bool):
        """One drain from the committed counts on; full token lists are the committed tokens + the returned tails."""
        B = self.B
        d = self._gpu.drain([len(c) for c in self.committed], ld, want_times)
        self.last_read_bytes = self._gpu.last_read_bytes
        out = []
        for b in range(B):
            live = range(d["count"][b])
            head = tuple(self.committed[b])
            nbest = [head + tuple(d["tokens"][b][n]) for n in live]
            nsc = [d["score"][b][n] for n in live]
            new = d["committed"][b] - len(head)
            if new > 0:
                self.committed[b] += d["tokens"][b][0][:new]
            self._maxlen[b] = max(d["len"][b][n] for n in live)
            ntimes = [d["times"][b][n] for n in live] if want_times else None
            out.append(DecodeResult(tokens=nbest[0], score=nsc[0], times=ntimes[0] if want_times else None, nbest=nbest,
                                    nbest_scores=nsc, nbest_times=ntimes))
        return out, d["overflow"]

    def _feed_beam_gpu(self, chunk, nf, over):
        k = min(self.beam, chunk.shape[-1])
        top_p, top_i = chunk.float().topk(k, dim=-1)
        self._gpu.feed(top_p, top_i, nf)                    # (a row in `over` is refused by the kernel itself)
        for b in range(self.B):
            if b not in over:
                self._frames[b] += nf[b]
        # a list grows by at most one token per frame: the tails fit in the longest tail so far + n
        out, flags = self._drain_gpu(self._tail() + chunk.shape[1], False)
        for b in range(self.B):                             # the kernel's own flags say the same
            if flags[b] and nf[b] > 0 and b not in over:
                over.append(b)
        return out

    def _tail(self) -> int:
        """The longest uncommitted tail of any row's token lists as of the last drain."""
        return max(self._maxlen[b] - len(self.committed[b]) for b in range(self.B))

    def partials(self) -> List[DecodeResult]:
        """What the last feed returned: per row the result if the stream ended here, without times."""
        if self.greedy:
            return [DecodeResult(list(self.committed[b])) for b in range(self.B)]
        if self._gpu is not None:
            return self._drain_gpu(self._tail(), False)[0]
        out = []
        for b in range(self.B):
            r = _prefix_beam_result(self._rows[b], self.graph)
            self.committed[b] = list(r.nbest[0][:_common_prefix_len(r.nbest)])
            r.times = r.nbest_times = None
            out.append(r)
        return out

    def results(self) -> List[DecodeResult]:
        if self.greedy:
            return [DecodeResult(list(self.committed[b]), times=list(self._times[b])) for b in range(self.B)]
        if self._gpu is not None:
            return self._drain_gpu(self._tail(), True)[0]
        return [_prefix_beam_result(r, self.graph) for r in self._rows]
