"""Float64 restatement of joint CTC/attention decoding, the time-synchronous beam search (wenet/espnet/beam_search_timesync.py:
BeamSearchTimeSync; joint_decoding, wenet/transformer/search.py:450-496).  It imports nothing of the product and keeps no decoder
state: the decoder is a callable logp(prefix) -> (V,) log-probabilities of the next token, which decoder_logp() below builds
on tests/attn_decoder_ref.decoder_forward (a full forward of the prefix per evaluation) and which a test may replace with a
stand-in.  Everything is keyed by the prefix (a tuple that starts with sos) for the whole utterance, as the reference's four
dictionaries are; all sums are Python floats over float(p_ctc[c]) and float(logp[c]).

The quirks are the reference's and are kept on purpose: a beam prefix enters the frame's candidate list only through the blank
branch; a child that is not on the beam but stands in the previous frame's table takes that entry's mass as well; a prefix's
start frames are fixed at its first sighting while its last end frame follows every later sighting; a child copies its parent's
end frames and confidences when it is created and never looks at the parent again; bit-equal joint scores collapse into one
candidate (the later one), and every token tied at the pre-beam threshold is a candidate.

Per executed frame the search records what the tests need: the candidate tokens, every scored prefix with its joint score,
the margin (the smallest gap between adjacent joint scores among the best beam + 1), the beam, and which of the quirks the frame
showed."""
import math

import torch

from tests import attn_decoder_ref as REF

NEG = -math.inf


def log_add(a: float, b: float) -> float:
    if a == NEG and b == NEG:
        return NEG
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def decoder_logp(state_dict, conf, memory, dtype=torch.float64):
    """logp(prefix) of the left decoder of state_dict over one utterance's memory (T', d): the log-softmax of the last row of a
    full forward, as Python floats' source (a (V,) tensor of `dtype`).  Counts its evaluations in .calls (a list of prefixes)."""
    sd = {k: v.detach().to(dtype) for k, v in state_dict.items()}
    prefix_key = "left_decoder." if conf["bidirectional"] else ""
    mem = memory.to(dtype).unsqueeze(0)
    mask = torch.ones(1, 1, mem.size(1), dtype=torch.bool)

    def logp(prefix):
        logp.calls.append(tuple(prefix))
        ys = torch.tensor([list(prefix)], dtype=torch.int64)
        logits = REF.decoder_forward(sd, prefix_key, conf, mem, mask, ys, torch.tensor([len(prefix)]))
        return torch.log_softmax(logits[0, -1], dim=-1)

    logp.calls = []
    return logp


class Search:
    """One utterance.  lpz: (T', V) float32 CTC log-probabilities; logp: the decoder callable (never called with dec_w == 0)."""

    def __init__(self, lpz, logp, sos, beam, ctc_weight=0.5, length_bonus=0.5, pre_beam_ratio=1.5, blank=0,
                 blank_threshold=1.0):
        self.lpz, self.logp, self.sos, self.beam, self.blank = lpz, logp, sos, beam, blank
        self.pre_beam = int(pre_beam_ratio * beam)
        self.ctc_w, self.dec_w, self.bonus = ctc_weight, 1.0 - ctc_weight, length_bonus
        self.log_threshold = math.log(blank_threshold)
        root = (sos,)
        self.hyps = [root]
        self.scores = {}
        self.table = {root: (NEG, 0.0)}                    # the previous executed frame's (p_nb, p_b)
        self.starts = {root: [0]}
        self.ends = {root: [0]}
        self.confs = {root: [(NEG, NEG)]}
        self.rows = {}                                     # prefix -> its decoder row (V floats), made at most once
        self.att = {root: 0.0}                             # prefix -> sum of its tokens' decoder log-probabilities
        self.frames = []                                   # one record per frame
        self.ever_on_beam = {root}

    def _row(self, prefix):
        if prefix not in self.rows:
            self.rows[prefix] = [float(x) for x in self.logp(prefix)]
        return self.rows[prefix]

    def _joint(self, h, table):
        score = self.ctc_w * log_add(*table[h])
        if len(h) > 1 and self.dec_w > 0:
            parent = h[:-1]
            step = self._row(parent)[h[-1]]
            self.att[h] = self.att[parent] + step
            score += self.att[h] * self.dec_w
            self.confs[h][-1] = (self.confs[h][-1][0], step)
        return score + self.bonus * (len(h) - 1)

    def time_step(self, t, forced=None):
        p = self.lpz[t]
        rec = dict(t=t, skipped=False, cands=None, scored=None, margin=None, beam=None, repeated=0, dropped=0, reentry=0,
                   back_on_beam=0, pre_beam_tie=False, score_tie=False)
        self.frames.append(rec)
        top = int(torch.argmax(p))
        if top == self.blank and float(p[top]) >= self.log_threshold:
            rec.update(skipped=True, beam=list(self.hyps))
            return
        threshold = torch.sort(p)[0][-self.pre_beam]
        cands = [int(i) for i in (p >= threshold).nonzero().reshape(-1)]
        rec["cands"] = cands
        rec["pre_beam_tie"] = len(cands) != self.pre_beam
        prev, nxt, order = self.table, {}, []
        p_blank = float(p[self.blank])
        for hyp in self.hyps:
            total = log_add(*prev[hyp])
            for c in cands:
                pc = float(p[c])
                if c == self.blank:
                    nb, b = nxt.get(hyp, (NEG, NEG))
                    nxt[hyp] = (nb, log_add(b, pc + total))
                    if hyp not in order:
                        order.append(hyp)
                    continue
                child = hyp + (c,)
                nb, b = nxt.get(child, (NEG, NEG))
                if child not in self.starts:
                    self.starts[child] = self.starts[hyp] + [t]
                    self.ends[child] = self.ends[hyp] + [t + 1]
                    self.confs[child] = self.confs[hyp] + [(NEG, NEG)]
                else:
                    self.ends[child][-1] = t + 1
                self.confs[child][-1] = (max(self.confs[child][-1][0], pc), self.confs[child][-1][1])
                if c == hyp[-1]:
                    rec["repeated"] += 1
                    nb_prev, b_prev = prev[hyp]
                    nb = log_add(nb, pc + b_prev)
                    own_nb, own_b = nxt.get(hyp, (NEG, NEG))
                    nxt[hyp] = (log_add(own_nb, pc + nb_prev), own_b)
                    self.ends[hyp][-1] = t + 1
                    self.confs[hyp][-1] = (max(self.confs[hyp][-1][0], pc), self.confs[hyp][-1][1])
                else:
                    nb = log_add(nb, pc + total)
                if child not in self.hyps and child in prev:
                    rec["reentry"] += 1
                    b = log_add(b, p_blank + log_add(*prev[child]))
                    nb = log_add(nb, pc + prev[child][0])
                nxt[child] = (nb, b)
                if child not in order:
                    order.append(child)
        rec["dropped"] = sum(h not in order for h in self.hyps)
        scores = {h: self._joint(h, nxt) for h in order}
        by_score = {}
        for h in order:                                    # bit-equal scores collapse, the later prefix staying
            by_score[scores[h]] = h
        ranked = sorted(by_score, reverse=True)
        flat = sorted(scores.values(), reverse=True)[:self.beam + 1]
        rec["score_tie"] = any(a == b for a, b in zip(flat, flat[1:]))      # a tie that reaches the beam or its edge
        best = ranked[:self.beam + 1]
        gaps = [a - b for a, b in zip(best, best[1:])]
        rec["margin"] = min(gaps) if gaps else math.inf
        rec["scored"] = dict(scores)
        rec["table"] = dict(nxt)
        before = self.hyps
        if forced is None:
            self.hyps = [by_score[s] for s in ranked[:self.beam]]
        else:
            self.hyps = [tuple(h) for h in forced]
        rec["back_on_beam"] = sum(h in self.ever_on_beam and h not in before for h in self.hyps)
        self.ever_on_beam.update(self.hyps)
        self.scores, self.table = scores, nxt
        rec["beam"] = list(self.hyps)
        rec["live"] = {h: (self.ends[h][-1], self.confs[h][-1]) for h in self.hyps}      # as they stand after this frame

    def run(self, forced=None):
        """forced: per frame the beam to continue from (None for a frame to prune by itself), or None."""
        for t in range(self.lpz.shape[0]):
            self.time_step(t, None if forced is None else forced[t])
        return self.result()

    def result(self):
        """The beam in order: tokens (without sos), scores, start and end frames, confidences exp(max(ctc, att)) per token, and
        the per-token live values next to the reported ones (they differ where a snapshot was taken before a later update)."""
        out = dict(nbest=[], nbest_scores=[], nbest_times=[], nbest_end_times=[], nbest_confidence=[], stale=0)
        if not self.scores:                                # every frame skipped: the empty hypothesis at 0.0
            return dict(nbest=[[]], nbest_scores=[0.0], nbest_times=[[]], nbest_end_times=[[]], nbest_confidence=[[]], stale=0)
        for h in self.hyps:
            out["nbest"].append(list(h[1:]))
            out["nbest_scores"].append(self.scores[h])
            out["nbest_times"].append(self.starts[h][1:])
            out["nbest_end_times"].append(self.ends[h][1:])
            out["nbest_confidence"].append([math.exp(max(c)) for c in self.confs[h][1:]])
            for j in range(1, len(h) - 1):
                anc = h[:j + 1]
                if self.ends[anc][-1] != self.ends[h][j] or self.confs[anc][-1] != self.confs[h][j]:
                    out["stale"] += 1
        return out

    def min_margin(self):
        return min((f["margin"] for f in self.frames if not f["skipped"]), default=math.inf)

