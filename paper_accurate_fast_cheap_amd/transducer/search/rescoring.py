"""Second pass over n-best lists with the transducer's full-sum score log p(y | x) (reference:
`Transducer._cal_transducer_score` / `transducer_attention_rescoring`, wenet/transducer/transducer.py:185-210, :288-425,
without the attention term: its decoder was not released).

The reference repeats the encoder output once per hypothesis and pushes every (hypothesis, t, u) row through the joint.  The
hypotheses of one n-best list share almost all their prefixes, and the joint row of (t, prefix) is the same for every
hypothesis that runs through that prefix, so the kernels backend (hip_ops.rnnt_score_hypotheses, csrc/rnnt_loss.hip) scores
the prefix TRIE: this module builds its table on the host.

A lattice column ("arc") of utterance b is (node, label) for every child edge of a trie node, or (node, none) for every node
without children: K_b = edges + leaves, and one hypothesis alone gives U + 1 arcs.  Position u of hypothesis n (0 <= u <= U_n)
maps to the column col[n][u]: for u < U_n the arc (h[:u], h[u]); for u = U_n any arc of node h[:U_n] (there only lse and
z[blank] are read, which depend on the node alone).  Each arc records the predictor row of its node as (n', u) of the first
hypothesis that passes through it, and its label (or -1)."""
from typing import List, Optional, Sequence

import numpy as np
import torch

from ...transformer.search import DecodeResult

MAX_HYP_TOKENS = 2558                      # U + 1 <= 2559: the lattice kernel's LDS (pafc_rnnt_score)
SCORE_BACKENDS = ("framework", "kernels")
RESCORING_MODES = ("ctc_beam_td_rescoring", "rnnt_beam_td_rescoring")


def check_score_backend(value: Optional[str], on_gpu: bool) -> str:
    """The backend of Transducer.score_hypotheses: "framework" (the reference's recipe as framework ops, CPU and GPU) or
    "kernels" (the prefix-trie scorer of the library, GPU only, never a fallback); None: kernels on the GPU, framework on
    the CPU."""
    if value is None:
        return "kernels" if on_gpu else "framework"
    if value not in SCORE_BACKENDS:
        raise ValueError(f"backend must be one of {SCORE_BACKENDS} or None, got {value!r}")
    return value


def check_hypotheses(hyps: Sequence[Sequence[Sequence[int]]], vocab_size: int, blank: int) -> None:
    for b, nbest in enumerate(hyps):
        for i, h in enumerate(nbest):
            if len(h) > MAX_HYP_TOKENS:
                raise ValueError(f"utterance {b}, hypothesis {i}: {len(h)} tokens, more than {MAX_HYP_TOKENS}")
            if not len(h):
                continue
            toks = np.asarray(h, dtype=np.int64)
            if (toks == blank).any():
                raise ValueError(f"utterance {b}, hypothesis {i}: the blank ({blank}) inside a hypothesis")
            bad = toks[(toks < 0) | (toks >= vocab_size)]
            if bad.size:
                raise ValueError(f"utterance {b}, hypothesis {i}: token {int(bad[0])} outside the vocabulary [0, {vocab_size})")


def _common_prefix(a: Sequence[int], b: Sequence[int]) -> int:
    """Length of the longest common prefix of two token lists, by bisection on slice comparisons."""
    hi = min(len(a), len(b))
    if a[:hi] == b[:hi]:
        return hi
    lo = 0                                  # a[:lo] == b[:lo] and a[:hi] != b[:hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[lo:mid] == b[lo:mid]:
            lo = mid
        else:
            hi = mid
    return lo


class ArcTables:
    """The arc tables of a batch of n-best lists as flat int32 arrays (views of `packed`, the one array that is uploaded, in
    the layout include/pafc_search.h documents for pafc_rnnt_score):
      utt_enc (nutt) the encoder row of utterance b, utt_T (nutt) its frames, arc_off / hyp_off (nutt + 1) its first arc /
      hypothesis; arc_prow / arc_label (narc) per arc the predictor row n' * pred_stride + u of its node and its label or -1;
      hyp_utt / hyp_len (nhyp); col_off (nhyp + 1) and col (ncol): col[col_off[n] + u] is the column, in [0, K_b), of position u.
    Hypotheses are numbered utterance by utterance in the order given (n = hyp_off[b] + i).  rows = sum_b T_b K_b is what the
    scorer computes, rows_repeated = sum_n T_b (U_n + 1) what one lattice per hypothesis would."""

    FIELDS = ("utt_enc", "utt_T", "arc_off", "hyp_off", "arc_prow", "arc_label", "hyp_utt", "hyp_len", "col_off", "col")

    def __init__(self, fields: dict, pred_stride: int):
        self.nutt, self.nhyp = len(fields["utt_enc"]), len(fields["hyp_utt"])
        self.narc, self.ncol = len(fields["arc_prow"]), len(fields["col"])
        self.pred_stride = pred_stride
        total = sum(len(fields[f]) for f in self.FIELDS)
        try:
            self.packed = torch.empty(total, dtype=torch.int32, pin_memory=torch.cuda.is_available())
        except RuntimeError:                           # (no pinned memory on this host: a pageable upload is still one upload)
            self.packed = torch.empty(total, dtype=torch.int32)
        at = 0
        for f in self.FIELDS:
            n = len(fields[f])
            view = self.packed[at:at + n]
            if n:
                view.copy_(torch.from_numpy(np.asarray(fields[f], dtype=np.int32)))
            setattr(self, f, view)
            at += n
        T, ao = fields["utt_T"], fields["arc_off"]
        self.utt_rows = [T[b] * (ao[b + 1] - ao[b]) for b in range(self.nutt)]
        self.rows = sum(self.utt_rows)
        self.rows_repeated = sum(T[b] * (u + 1) for b, u in zip(fields["hyp_utt"], fields["hyp_len"]))

    def arcs(self, b: int) -> int:
        return int(self.arc_off[b + 1] - self.arc_off[b])


def build_arc_tables(hyps: Sequence[Sequence[Sequence[int]]], lens: Sequence[int], vocab_size: int, blank: int,
                     pred_stride: Optional[int] = None, share: bool = True) -> ArcTables:
    """hyps[b]: the token lists of utterance b; lens[b]: its encoder frames T_b.  pred_stride: the row pitch of the predictor
    output the arcs index (row n * pred_stride + u holds the predictor after the first u tokens of hypothesis n); default
    max U + 1.  share=False makes every hypothesis an utterance of its own (utt_enc names its encoder row): the same rows the
    reference's repeat computes.  ValueError (naming utterance and hypothesis) for a blank inside a hypothesis, a token outside
    [0, vocab_size) or more than 2558 tokens."""
    check_hypotheses(hyps, vocab_size, blank)
    if len(lens) != len(hyps):
        raise ValueError(f"{len(hyps)} n-best lists but {len(lens)} lengths")
    umax = max((len(h) for nbest in hyps for h in nbest), default=0)
    if pred_stride is None:
        pred_stride = umax + 1
    if pred_stride < umax + 1:
        raise ValueError(f"pred_stride {pred_stride} is below the longest hypothesis + 1 ({umax + 1})")
    for b, nbest in enumerate(hyps):
        if len(nbest) and int(lens[b]) < 1:
            raise ValueError(f"utterance {b}: {int(lens[b])} frames")
    if share:
        units = [(b, int(lens[b]), [list(h) for h in nbest]) for b, nbest in enumerate(hyps)]
    else:
        units = [(b, int(lens[b]), [list(h)]) for b, nbest in enumerate(hyps) for h in nbest]
    # Per utterance the trie is built without a Python step per token: hypothesis i shares its first L_i + 1 nodes with the
    # earlier hypothesis of the longest common prefix (found by bisection on slice comparisons) and creates one node per
    # remaining token.  Node c >= 1 is created by exactly one edge, so the edges are the arcs 0 .. nodes - 2 (arc c - 1 enters
    # node c: its label, and the predictor row of c's PARENT), followed by one label-less arc per node without children.
    utt_enc, utt_T, arc_off, hyp_off, hyp_utt, hyp_len, col_off = [], [], [0], [0], [], [], [0]
    prow_parts, label_parts, col_parts = [], [], []
    n0 = 0
    for ui, (b, T, nbest) in enumerate(units):
        utt_enc.append(b)
        utt_T.append(T)
        K = 0
        if nbest:
            paths, nodes = [], 1
            parent, label, first_n, first_u = [np.array([-1])], [np.array([-1])], [np.array([n0])], [np.array([0])]
            for i, h in enumerate(nbest):
                L, src = 0, -1
                for j in range(i):
                    lcp = _common_prefix(h, nbest[j])
                    if lcp > L:
                        L, src = lcp, j
                new = len(h) - L
                ids = np.arange(nodes, nodes + new, dtype=np.int64)
                path = np.concatenate([paths[src][:L + 1] if src >= 0 else np.zeros(1, dtype=np.int64), ids])
                if new:
                    parent.append(path[L:-1])
                    label.append(np.asarray(h[L:], dtype=np.int64))
                    first_n.append(np.full(new, n0 + i, dtype=np.int64))
                    first_u.append(np.arange(L + 1, len(h) + 1, dtype=np.int64))
                nodes += new
                paths.append(path)
            parent, label = np.concatenate(parent), np.concatenate(label)
            row = np.concatenate(first_n) * pred_stride + np.concatenate(first_u)        # predictor row of every node
            edges = nodes - 1
            has_child = np.zeros(nodes, dtype=bool)
            has_child[parent[1:]] = True
            leaves = np.flatnonzero(~has_child)
            end_arc = np.full(nodes, nodes, dtype=np.int64)                              # an arc of the node, for u = U_n:
            np.minimum.at(end_arc, parent[1:], np.arange(edges, dtype=np.int64))         # its first edge, or
            end_arc[leaves] = edges + np.arange(len(leaves))                             # its label-less arc
            K = edges + len(leaves)
            prow_parts += [row[parent[1:]], row[leaves]]
            label_parts += [label[1:], np.full(len(leaves), -1, dtype=np.int64)]
            for i, h in enumerate(nbest):
                hyp_utt.append(ui)
                hyp_len.append(len(h))
                col_parts += [paths[i][1:] - 1, end_arc[paths[i][-1:]]]
                col_off.append(col_off[-1] + len(h) + 1)
        arc_off.append(arc_off[-1] + K)
        n0 += len(nbest)
        hyp_off.append(n0)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)      # noqa: E731
    f = {"utt_enc": utt_enc, "utt_T": utt_T, "arc_off": arc_off, "hyp_off": hyp_off, "arc_prow": cat(prow_parts),
         "arc_label": cat(label_parts), "hyp_utt": hyp_utt, "hyp_len": hyp_len, "col_off": col_off, "col": cat(col_parts)}
    return ArcTables(f, pred_stride)


def rescore(first_pass: List[DecodeResult], td_scores: List[List[float]], ctc_weight: float, transducer_weight: float
            ) -> List[DecodeResult]:
    """final_i = ctc_weight * first_pass_score_i + transducer_weight * td_i (transducer.py:418-420 without the attention term);
    the n-best list re-ordered by final, descending and stable, so on ties the earlier first-pass rank wins (the reference's
    strict `>`).  times / nbest_times follow their hypotheses when the first pass reports them; nbest_td_scores holds the raw
    td_i in the new order."""
    out = []
    for r, td in zip(first_pass, td_scores):
        nbest = r.nbest if r.nbest is not None else [r.tokens]
        scores = r.nbest_scores if r.nbest_scores is not None else [r.score]
        assert len(td) == len(nbest) == len(scores)
        if not nbest:
            out.append(DecodeResult(tokens=[], score=r.score, nbest=[], nbest_scores=[], nbest_td_scores=[]))
            continue
        # (a zero weight drops its term: 0 * -inf of an unreachable first-pass entry must not turn the sum into NaN)
        final = [(ctc_weight * s if ctc_weight != 0 else 0.0) + (transducer_weight * t if transducer_weight != 0 else 0.0)
                 for s, t in zip(scores, td)]
        order = sorted(range(len(nbest)), key=lambda i: -final[i])          # (sorted is stable)
        ntimes = None if r.nbest_times is None else [r.nbest_times[i] for i in order]
        out.append(DecodeResult(tokens=nbest[order[0]], score=final[order[0]], times=None if ntimes is None else ntimes[0],
                                nbest=[nbest[i] for i in order], nbest_scores=[final[i] for i in order], nbest_times=ntimes,
                                nbest_td_scores=[td[i] for i in order]))
    return out
