"""The formulation of pafc_joint_frame (csrc/joint_search.hip) as a plain Python model, against the float64 restatement
(tests/joint_search_ref.py), without a GPU.

The reference loops over (beam prefix, candidate) and accumulates into dictionaries.  The kernel instead makes every scored
prefix of a frame one item that one lane owns and GATHERS its table entry: p_nb from the expansion of its one parent plus
either its own repeat (it is on the beam) or the "considered before" term (it is not); p_b from its own blank branch or the
"considered before" term.  At most two terms meet in one log-add, so no result depends on the order in which items are
processed; the only order that matters, the reference's loop order for the snapshot a new node takes of its parent's live (end
frame, ctc confidence), is decided per item from its place in the loop (`sees`).  Model.frame below is that formulation line
for line (phases A to D of frame_kernel, the same names), with lists for the node pool and a dict for the hash; the tests hold
it to the restatement -- beams of every frame, n-best lists, start and end frames exactly, scores and confidences to 1e-10 --
and run it with the items of phase C in reversed and in shuffled order, which must change nothing."""
import math
import random

import pytest

from tests import attn_rescore_cases as C
from tests import joint_search_ref as JR
from tests.test_joint_search import SETTINGS, ctc_case, joint_model, shared_logp

NEG = -math.inf


def logadd(a, b):
    if a == NEG and b == NEG:
        return NEG
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


class Node:
    """A trie node as pafc_joint_state holds it; tab: executed frame -> (p_nb, p_b) (the kernel keeps the last two)."""

    def __init__(self, parent, token, length):
        self.parent, self.token, self.length = parent, token, length
        self.start = self.end = self.snap_end = 0
        self.ctc = self.snap_ctc = self.att_conf = NEG
        self.att_sum = 0.0
        self.tab = {}


class Model:
    """One utterance.  order: a function that permutes the list of a frame's items in place (the lanes' order of arrival)."""

    def __init__(self, lpz, logp, sos, N, C, ctc_w, bonus, blank=0, thr=1.0, order=None):
        self.lpz, self.logp, self.N, self.C, self.blank, self.order = lpz, logp, N, C, blank, order
        self.ctc_w, self.dec_w, self.bonus = ctc_w, 1.0 - ctc_w, bonus
        self.log_threshold = math.log(thr)
        root = Node(-1, sos, 1)
        root.tab[0] = (NEG, 0.0)
        self.nodes, self.hash = [root], {}
        self.beam, self.score = [0], [0.0]
        self.e = 0                                         # executed frames so far
        self.trace = []

    def prefix(self, n):
        toks = []
        while n >= 0:
            toks.append(self.nodes[n].token)
            n = self.nodes[n].parent
        return tuple(toks[::-1])

    def frame(self, t):
        nodes, C, blank = self.nodes, self.C, self.blank
        vals = [float(x) for x in self.lpz[t]]
        ranked = sorted(range(len(vals)), key=lambda i: (-vals[i], i))
        if ranked[0] == blank and vals[ranked[0]] >= self.log_threshold:
            self.trace.append(None)
            return
        # the candidates (pafc_joint_candidates) and the beam's values as the kernel's phase 0 loads them
        ctok = sorted(ranked[:C])
        cp = [vals[c] for c in ctok]
        e, nl = self.e + 1, len(self.beam)
        hn = list(self.beam)
        hlast, hlen, hpar = ([getattr(nodes[n], k) for n in hn] for k in ("token", "length", "parent"))
        hnb = [nodes[n].tab.get(e - 1, (NEG, NEG))[0] for n in hn]
        hb = [nodes[n].tab.get(e - 1, (NEG, NEG))[1] for n in hn]
        htot = [logadd(a, b) for a, b in zip(hnb, hb)]
        hatt = [nodes[n].att_sum for n in hn]
        old_end, old_ctc = [nodes[n].end for n in hn], [nodes[n].ctc for n in hn]
        bci = ctok.index(blank) if blank in ctok else -1
        has_blank, pblank = bci >= 0, vals[blank]
        pj, lc = [-1] * nl, [-1] * nl                      # the parent's slot on the beam; the last token's candidate index
        for i in range(nl):
            for j in range(nl):
                if j != i and hn[j] == hpar[i]:
                    pj[i] = j
            for c in range(C):
                if ctok[c] == hlast[i] and ctok[c] != blank:
                    lc[i] = c
        rows = [None] * nl                                 # the beam's decoder rows, taken when first needed
        # A: look every child up; B: number the new nodes in the loop's order
        nit = nl * C
        cid, isnew = [-1] * nit, [False] * nit
        for k in range(nit):
            i, ci = divmod(k, C)
            cid[k] = hn[i] if ci == bci else self.hash.get((hn[i], ctok[ci]), -1)
        for k in range(nit):
            if cid[k] == -1:
                cid[k], isnew[k] = len(nodes), True
                nodes.append(None)
        # C: one lane per item, in any order
        isc, ikey = [math.nan] * nit, list(range(nit))
        items = list(range(nit))
        if self.order is not None:
            self.order(items)
        for k in items:
            i, ci = divmod(k, C)
            c, child = ctok[ci], cid[k]
            if ci == bci:
                # the prefix itself, through the blank branch -- unless another beam prefix's pair owns it this frame
                if pj[i] >= 0 and lc[i] >= 0:
                    continue
                nb = cp[lc[i]] + hnb[i] if lc[i] >= 0 else NEG
                bb = pblank + htot[i]
                nodes[child].tab[e] = (nb, bb)
                if lc[i] >= 0:
                    nodes[child].end, nodes[child].ctc = t + 1, max(old_ctc[i], cp[lc[i]])
                sc = self.ctc_w * logadd(nb, bb)
                if hlen[i] > 1 and self.dec_w > 0:
                    sc += hatt[i] * self.dec_w
                isc[k] = sc + self.bonus * (hlen[i] - 1)
                continue
            pc, fresh = cp[ci], isnew[k]
            j = -1 if fresh else next((q for q in range(nl) if hn[q] == child), -1)      # the child's slot, if on the beam
            if fresh:
                self.hash[(hn[i], c)] = child
                nd = nodes[child] = Node(hn[i], c, hlen[i] + 1)
                nd.start, nd.end, nd.ctc = t, t + 1, cp[ci]
                # has the parent's live (end, ctc_conf) changed by the time the loop forms this child?
                sees = lc[i] >= 0 and ((pj[i] >= 0 and pj[i] < i) or c > hlast[i])
                nd.snap_end = t + 1 if sees else old_end[i]
                nd.snap_ctc = max(old_ctc[i], cp[lc[i]]) if sees else old_ctc[i]
            else:
                nd = nodes[child]
                nd.end, nd.ctc = t + 1, max(old_ctc[j] if j >= 0 else nd.ctc, cp[ci])
            nb, bb = pc + (hb[i] if c == hlast[i] else htot[i]), NEG
            if j >= 0:
                nb = logadd(nb, pc + hnb[j])
                if has_blank:
                    bb = pblank + htot[j]
                    ikey[k] = min(k, j * C + bci)
            elif not fresh and (e - 1) in nd.tab:          # considered before
                pnb, pb = nd.tab[e - 1]
                bb = pblank + logadd(pnb, pb)
                nb = logadd(nb, pc + pnb)
            nd.tab[e] = (nb, bb)
            sc = self.ctc_w * logadd(nb, bb)
            if self.dec_w > 0:
                if fresh:
                    if rows[i] is None:
                        rows[i] = [float(x) for x in self.logp(self.prefix(hn[i]))]
                    nd.att_conf = rows[i][c]
                    nd.att_sum = hatt[i] + nd.att_conf
                sc += nd.att_sum * self.dec_w
            isc[k] = sc + self.bonus * hlen[i]
        # beam prefixes that no item covers still enter the table through their own repeat
        for i in range(nl):
            if not has_blank and lc[i] >= 0 and pj[i] < 0:
                n = nodes[hn[i]]
                n.tab[e] = (cp[lc[i]] + hnb[i], NEG)
                n.end, n.ctc = t + 1, max(old_ctc[i], cp[lc[i]])
        # D: the N best items, score descending, the reference's listing order ascending
        best = sorted((k for k in range(nit) if isc[k] == isc[k]), key=lambda k: (-isc[k], ikey[k]))[:self.N]
        self.beam, self.score, self.e = [cid[k] for k in best], [isc[k] for k in best], e
        self.trace.append([self.prefix(n) for n in self.beam])

    def result(self):
        """pafc_joint_collect: per beam (tokens, score, start frames, end frames, confidences); a token reports its node's live
        values if it is the last, else the snapshot held by the next node on the path."""
        out = []
        for n, sc in zip(self.beam, self.score):
            toks, starts, ends, confs = [], [], [], []
            first, snap_end, snap_ctc = True, None, None
            while n > 0:
                nd = self.nodes[n]
                toks.append(nd.token)
                starts.append(nd.start)
                ends.append(nd.end if first else snap_end)
                confs.append(math.exp(max(nd.ctc if first else snap_ctc, nd.att_conf)))
                first, snap_end, snap_ctc, n = False, nd.snap_end, nd.snap_ctc, nd.parent
            out.append((toks[::-1], sc, starts[::-1], ends[::-1], confs[::-1]))
        return out


ORDERS = {"loop": None, "reversed": lambda items: items.reverse(), "shuffled": random.Random(5).shuffle}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("beam", [1, 4, 10])
def test_item_formulation_equals_the_restatement(beam, order):
    for pre in (True, False):
        m, ctc = joint_model(pre), ctc_case(pre)
        for b, n in enumerate(C.LENS):
            for cw, bo, th in (SETTINGS[0], SETTINGS[4], SETTINGS[5]):
                ref = JR.Search(ctc[b, :n], shared_logp(pre, b), m.sos, beam, cw, bo, blank_threshold=th)
                want = ref.run()
                km = Model(ctc[b, :n], shared_logp(pre, b), m.sos, beam, int(1.5 * beam), cw, bo, thr=th, order=ORDERS[order])
                for t in range(n):
                    km.frame(t)
                got = km.result()
                case = (pre, beam, n, cw, bo, th)
                assert [x for x in km.trace if x is not None] == [f["beam"] for f in ref.frames if not f["skipped"]], case
                assert [g[0] for g in got] == want["nbest"] and [g[2] for g in got] == want["nbest_times"], case
                assert [g[3] for g in got] == want["nbest_end_times"], case                      # snapshots included
                for g, sc, cf in zip(got, want["nbest_scores"], want["nbest_confidence"]):
                    assert g[1] == sc or abs(g[1] - sc) <= 1e-10, case
                    assert all(abs(x - y) <= 1e-10 for x, y in zip(g[4], cf)), case
