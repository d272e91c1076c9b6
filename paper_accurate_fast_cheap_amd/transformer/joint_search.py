"""Joint CTC/attention decoding: the time-synchronous one-pass beam search (reference: joint_decoding,
wenet/transformer/search.py:450-496, on BeamSearchTimeSync, wenet/espnet/beam_search_timesync.py; the decode mode
"joint_decoding").

A CTC prefix beam search over the frames in which every candidate prefix h is scored jointly,
    joint(h) = ctc_w * logadd(p_nb(h), p_b(h)) + dec_w * att(h) + length_bonus * (len(h) - 1),
    att(h) = att(h[:-1]) + log p_dec(h[-1] | h[:-1]), att([sos]) = 0, dec_w = 1 - ctc_w,
and the beam is pruned on that score.  Per frame: the frame is skipped when blank is its arg-max at p >= log(blank_threshold);
the candidates are the tokens at or above the pre_beam_size-th largest CTC log-probability (pre_beam_size = int(pre_beam_ratio *
beam_size)); every beam prefix is expanded by every candidate; the beam_size best stay.  Every prefix carries the start and end
frame and the confidence exp(max(ctc_conf, att_conf)) of each of its tokens.

The reference's behaviour is kept where it surprises:
  * a repeated token c == h[-1] gives h + [c] the mass p_ctc[c] + p_b(h) and h itself p_ctc[c] + p_nb(h), but h enters the
    frame's candidate list through the blank branch only: a beam prefix whose frame has no blank candidate is not scored and
    leaves the beam, although it stays in the frame's table;
  * a child that is not on the beam but stands in the previous executed frame's table ("considered before") also takes
    p_ctc[blank] + logadd(previous) into p_b and p_ctc[c] + previous p_nb into p_nb -- p_ctc[blank] counts here even when blank is
    no candidate;
  * a prefix's start frames are fixed at its first sighting in the utterance and survive its leaving the beam; its last end
    frame is set to t + 1 at every later sighting; ctc_conf is the maximum of p_ctc[c] over those sightings;
  * a child copies its parent's end frames and confidences when it is first formed: what the parent's last entry becomes later
    reaches the children formed later, not the ones formed before;
  * the sums are float64 over float32 CTC log-probabilities and the decoder's log-probabilities in its dtype; -inf is data (a beam
    of 1 can end at a score of -inf).

Differences from the reference, all deliberate:
  * sos is model.sos (the reference's wrapper hard-codes 10000);
  * a result carries all beam_size hypotheses (nbest / nbest_scores / nbest_times), the reference's single best first;
  * cat_embs (language-specific decoders), the lexicon constraint (words / word_prefixes) and the LM hooks are left out;
  * an utterance whose every frame is skipped gives the empty hypothesis at score 0.0 (the reference raises KeyError);
  * ties: backend "framework" does what the reference does -- every token tied at the pre-beam threshold is a candidate, and
    hypotheses with bit-equal joint scores collapse into one (the later).  Backend "kernels" takes exactly pre_beam_size
    candidates, the lowest index winning a tie, and keeps tied hypotheses, the earlier candidate first.

backend "framework" is the reference's loop restated on decoder.forward_one_step with its per-prefix cache, one utterance after
the other, on the CPU or the GPU.  The CTC frames and each decoded row are brought to the host once (the reference reads the
device once per candidate).

backend "kernels" (GPU only, never a fallback) runs the whole batch in lockstep with every piece of state on the device
(include/pafc_joint_search.h): per utterance a trie of every prefix ever formed with an open-addressing hash (parent, token) ->
node, the float64 CTC table stamped with the executed frame that wrote it, per layer a key/value cache and a pool of decoded
hidden rows whose rows are written once and never moved (a prefix is decoded at most once per utterance and keeps its row when
it leaves the beam), and per beam slot the table of its ancestors' cache rows.  Before the loop one launch takes the
candidates of all frames; a frame is then: gather the beam's hidden rows, output_layer on the library's GEMM, pafc_joint_frame
(one block per utterance: expansion, recursion, times, confidences, joint scores, the new beam), and the decoder step of the
R = B * N rows at their different positions (decoder_rows.decoder_layers on the set-up of decoder_rows.SearchEngine, with
pafc_mha_step_paths as its self-attention; rows that enter the beam decoded ride along and write nothing).  Nothing in the loop
reads the device; one read after the last frame brings the beams' hypotheses in compact form (pafc_joint_collect), the scores
and the counters."""
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .attn_search import CACHE_CAP_BYTES, MAX_BEAM
from .decoder import subsequent_mask
from .decoder_rows import SearchEngine, kernels_unmet, left_right, pass_launches
from .search import DecodeResult

MAX_PRE_BEAM = 24                  # candidates per frame the kernels backend is laid out for (beam 16 at pre_beam_ratio 1.5)
NEG = -math.inf


def _log_add(a: float, b: float) -> float:
    if a == NEG and b == NEG:
        return NEG
    m = a if a > b else b
    return m + math.log(math.exp(a - m) + math.exp(b - m))


@torch.no_grad()
def joint_decoding(model, encoder_out: torch.Tensor, encoder_lens: torch.Tensor, ctc_probs: torch.Tensor,
                   ctc_weight: float = 0.5, beam_size: int = 4, pre_beam_ratio: float = 1.5, length_bonus: float = 0.5,
                   blank_id: int = 0, blank_threshold: float = 1.0, backend: Optional[str] = None, return_trace: bool = False,
                   cat_embs=None) -> List[DecodeResult]:
    """encoder_out (B, T', d), encoder_lens (B) (tensor or list), ctc_probs (B, T', V) CTC log-probabilities -> one DecodeResult
    per utterance: tokens / score of the best hypothesis, times and end_times its tokens' start and end frames,
    tokens_confidence exp(max(ctc_conf, att_conf)) per token, nbest / nbest_scores / nbest_times (start frames) all beam
    hypotheses in the search's order, stats (decoder_evaluations, frames, frames_skipped, host_reads, and nbest_end_times /
    nbest_tokens_confidence for the hypotheses behind the first), and with return_trace a trace:
    dict(beam, score): per frame the beam's token lists (without sos) and joint scores after that frame.
    backend: "framework" | "kernels" | None (kernels on the GPU, framework on the CPU); see the module's text.
    With ctc_weight == 1 the decoder is never run.
    ValueError: cat_embs, ctc_weight outside [0, 1], pre_beam_size < 1 or above V, a blank_threshold outside (0, 1], shapes."""
    from ..transducer.search.rescoring import check_score_backend
    decoder = getattr(model, "decoder", None)
    if decoder is None:
        raise NotImplementedError("joint_decoding needs an attention decoder (init_model builds one with "
                                  "args.attention_decoder)")
    if cat_embs is not None:
        raise ValueError("joint_decoding: cat_embs must be None (language-specific decoders are outside this search)")
    if not 0.0 <= ctc_weight <= 1.0:
        raise ValueError(f"joint_decoding: ctc_weight = {ctc_weight} is outside [0, 1]")
    if not 0.0 < blank_threshold <= 1.0:
        raise ValueError(f"joint_decoding: blank_threshold = {blank_threshold} is outside (0, 1]")
    backend = check_score_backend(backend, encoder_out.is_cuda)
    if encoder_out.dim() != 3 or ctc_probs.dim() != 3 or ctc_probs.shape[:2] != encoder_out.shape[:2]:
        raise ValueError(f"joint_decoding: ctc_probs {tuple(ctc_probs.shape)} for encoder_out {tuple(encoder_out.shape)}")
    B, T, V = ctc_probs.shape
    lens = [int(n) for n in (encoder_lens.tolist() if torch.is_tensor(encoder_lens) else encoder_lens)]
    if len(lens) != B or any(not 0 <= n <= T for n in lens):
        raise ValueError(f"joint_decoding: encoder_lens {lens} for {B} utterances of {T} frames")
    if not 0 <= blank_id < V:
        raise ValueError(f"joint_decoding: blank_id = {blank_id} for a vocabulary of {V}")
    pre_beam = int(pre_beam_ratio * beam_size)
    if beam_size < 1 or pre_beam < 1 or pre_beam > V:
        raise ValueError(f"joint_decoding: a beam of {beam_size} and pre_beam_size = int({pre_beam_ratio} * {beam_size}) = "
                         f"{pre_beam} for a vocabulary of {V} (both at least 1, pre_beam_size at most V)")
    if backend == "kernels":
        from .._lib import PafcError
        if not 1 <= beam_size <= MAX_BEAM:
            raise PafcError(f"joint_decoding(backend='kernels'): a beam of {beam_size} (the frame kernel takes 1..{MAX_BEAM})")
        if pre_beam > MAX_PRE_BEAM:
            raise PafcError(f"joint_decoding(backend='kernels'): pre_beam_size = {pre_beam} (the frame kernel takes up to "
                            f"{MAX_PRE_BEAM} candidates per frame)")
        unmet = kernels_unmet(model, encoder_out, False)
        if unmet is not None:
            raise PafcError(f"joint_decoding(backend='kernels'): {unmet}")
        if V != model.vocab_size and 1.0 - ctc_weight > 0:
            raise PafcError(f"joint_decoding(backend='kernels'): ctc_probs over {V} tokens for a decoder over {model.vocab_size}")
        return _search_kernels(model, encoder_out, lens, ctc_probs, ctc_weight, beam_size, pre_beam, length_bonus, blank_id,
                               blank_threshold, return_trace)
    dec, _ = left_right(decoder)
    dec_w = 1.0 - ctc_weight
    out = []
    for b in range(B):
        n = lens[b]
        search = _Utterance(dec, encoder_out[b:b + 1, :n], ctc_probs[b, :n], int(model.sos), beam_size, pre_beam, ctc_weight,
                            dec_w, length_bonus, blank_id, blank_threshold, return_trace)
        out.append(search.run())
    return out


class _Utterance:
    """The framework backend's search of one utterance; all state is keyed by the prefix (a tuple that starts with sos)."""

    def __init__(self, dec, memory, lpz, sos, beam, pre_beam, ctc_w, dec_w, bonus, blank, blank_threshold, want_trace):
        self.dec, self.beam, self.pre_beam, self.blank = dec, beam, pre_beam, blank
        self.ctc_w, self.dec_w, self.bonus = ctc_w, dec_w, bonus
        self.log_threshold = math.log(blank_threshold)
        self.memory = memory.to(dec.after_norm.weight.dtype)
        self.memory_mask = torch.ones(1, 1, memory.size(1), dtype=torch.bool, device=memory.device)
        self.lpz = lpz.detach().float().cpu()                      # one read: the utterance's frames
        self.rows_host = self.lpz.tolist()
        root = (sos,)
        self.hyps: List[tuple] = [root]
        self.scores: Dict[tuple, float] = {}
        self.table: Dict[tuple, Tuple[float, float]] = {root: (NEG, 0.0)}
        self.starts, self.ends = {root: [0]}, {root: [0]}
        self.confs = {root: [(NEG, NEG)]}
        self.att = {root: 0.0}
        self.decoded: Dict[tuple, Tuple[list, List[float]]] = {}    # prefix -> (per-layer cache, its row of log-probabilities)
        self.skipped = 0
        self.trace = dict(beam=[], score=[]) if want_trace else None

    def _row(self, prefix: tuple) -> List[float]:
        """log p(. | prefix): one forward_one_step on the parent's cache, at most once per prefix and utterance."""
        hit = self.decoded.get(prefix)
        if hit is None:
            cache = self.decoded[prefix[:-1]][0] if len(prefix) > 1 else None
            tgt = torch.tensor([prefix], dtype=torch.long, device=self.memory.device)
            mask = subsequent_mask(len(prefix), self.memory.device).unsqueeze(0)
            logp, cache = self.dec.forward_one_step(self.memory, self.memory_mask, tgt, mask, cache)
            hit = self.decoded[prefix] = (cache, logp[0].tolist())
        return hit[1]

    def _joint(self, h: tuple, table) -> float:
        score = self.ctc_w * _log_add(*table[h])
        if len(h) > 1 and self.dec_w > 0:
            parent = h[:-1]
            step = self._row(parent)[h[-1]]
            self.att[h] = self.att[parent] + step
            score += self.att[h] * self.dec_w
            self.confs[h][-1] = (self.confs[h][-1][0], step)
        return score + self.bonus * (len(h) - 1)

    def _frame(self, t: int) -> None:
        p, row = self.lpz[t], self.rows_host[t]
        top = int(torch.argmax(p))
        if top == self.blank and row[top] >= self.log_threshold:
            self.skipped += 1
            return
        threshold = torch.sort(p)[0][-self.pre_beam]
        cands = (p >= threshold).nonzero().reshape(-1).tolist()
        prev, nxt, order = self.table, {}, []
        on_beam = set(self.hyps)
        p_blank = row[self.blank]
        for hyp in self.hyps:
            total = _log_add(*prev[hyp])
            for c in cands:
                pc = row[c]
                if c == self.blank:
                    nb, b = nxt.get(hyp, (NEG, NEG))
                    nxt[hyp] = (nb, _log_add(b, pc + total))
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
                ctc_conf, att_conf = self.confs[child][-1]
                self.confs[child][-1] = (max(ctc_conf, pc), att_conf)
                if c == hyp[-1]:
                    # a repeated token: the child through the blank in between, and the prefix itself (which only the blank
                    # branch above puts on the frame's candidate list)
                    nb_prev, b_prev = prev[hyp]
                    nb = _log_add(nb, pc + b_prev)
                    own_nb, own_b = nxt.get(hyp, (NEG, NEG))
                    nxt[hyp] = (_log_add(own_nb, pc + nb_prev), own_b)
                    self.ends[hyp][-1] = t + 1
                    ctc_conf, att_conf = self.confs[hyp][-1]
                    self.confs[hyp][-1] = (max(ctc_conf, pc), att_conf)
                else:
                    nb = _log_add(nb, pc + total)
                if child not in on_beam and child in prev:           # considered before, pruned: last frame's mass counts
                    b = _log_add(b, p_blank + _log_add(*prev[child]))
                    nb = _log_add(nb, pc + prev[child][0])
                nxt[child] = (nb, b)
                if child not in order:
                    order.append(child)
        scores = {h: self._joint(h, nxt) for h in order}
        by_score = {}
        for h in order:                                              # bit-equal scores collapse, the later prefix staying
            by_score[scores[h]] = h
        self.hyps = [by_score[s] for s in sorted(by_score, reverse=True)[:self.beam]]
        self.scores, self.table = scores, nxt

    def run(self) -> DecodeResult:
        for t in range(self.lpz.shape[0]):
            self._frame(t)
            if self.trace is not None:
                self.trace["beam"].append([list(h[1:]) for h in self.hyps])
                self.trace["score"].append([self.scores.get(h, 0.0) for h in self.hyps])
        stats = dict(decoder_evaluations=len(self.decoded), frames=int(self.lpz.shape[0]), frames_skipped=self.skipped,
                     host_reads=1 + len(self.decoded))
        if not self.scores:                                          # every frame skipped (or none at all)
            return DecodeResult(tokens=[], score=0.0, times=[], end_times=[], tokens_confidence=[], nbest=[[]],
                                nbest_scores=[0.0], nbest_times=[[]], stats=stats, trace=self.trace)
        nbest = [list(h[1:]) for h in self.hyps]
        best = self.hyps[0]
        stats["nbest_end_times"] = [self.ends[h][1:] for h in self.hyps]
        stats["nbest_tokens_confidence"] = [[math.exp(max(c)) for c in self.confs[h][1:]] for h in self.hyps]
        return DecodeResult(tokens=nbest[0], score=self.scores[best], times=self.starts[best][1:], end_times=self.ends[best][1:],
                            tokens_confidence=[math.exp(max(c)) for c in self.confs[best][1:]], nbest=nbest,
                            nbest_scores=[self.scores[h] for h in self.hyps],
                            nbest_times=[self.starts[h][1:] for h in self.hyps], stats=stats, trace=self.trace)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels backend
# ---------------------------------------------------------------------------------------------------------------------------

class _Engine(SearchEngine):
    """The device state of one call, its decoder step and its frame.  Nothing here reads the device."""

    def __init__(self, model, encoder_out, lens, ctc_probs, N, C, ctc_w, dec_w, bonus, blank, blank_threshold):
        from .._lib import PafcError
        self.bind_decoder(model, "joint_decoding")
        dec, dtype = self.dec, self.dtype
        self.N, self.blank = N, blank
        self.weights = (ctc_w, dec_w, bonus)
        self.use_dec = dec_w > 0
        dev = encoder_out.device
        B, T, d = encoder_out.shape
        self.B, self.T, self.R, self.V = B, T, B * N, ctc_probs.size(2)
        R = self.R
        self.rows = (T + 1) * R                                   # cache rows; the hidden pool has one more, the dump row
        self.cache_bytes = self.cache_bytes_of(self.rows, d) if self.use_dec else 0
        if self.cache_bytes > CACHE_CAP_BYTES:
            raise PafcError(f"joint_decoding(backend='kernels'): the key/value caches of {len(dec.decoders)} layers x {T + 1} "
                            f"rounds x {R} rows need {self.cache_bytes} bytes, above CACHE_CAP_BYTES = {CACHE_CAP_BYTES}: decode "
                            "fewer utterances per call")
        self.lens = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.state = self.ops.JointSearchState(B, N, C, T, int(model.sos), dev, decode=self.use_dec)
        ctc = ctc_probs if ctc_probs.dtype in (torch.float32, torch.bfloat16) else ctc_probs.float()
        self.ops.joint_candidates(self.state, ctc.contiguous(), self.lens, blank, math.log(blank_threshold))
        self.launches = self.reads = 0
        if not self.use_dec:
            return
        # an utterance without frames asks for no decode, not even of [sos]: its slot rides along and stores nothing
        st = self.state
        has = self.lens > 0
        slot0 = lambda x: x.view(B, N)[:, 0]                                                                    # noqa: E731
        slot0(st.need).mul_(has)
        st.evals.mul_(has)
        slot0(st.store_row).copy_(torch.where(has, slot0(st.store_row), torch.full_like(self.lens, (T + 1) * R)))
        st.row[:, 0].copy_(torch.where(has, st.row[:, 0], torch.full_like(self.lens, -1)))
        self.project_memory(encoder_out, self.lens, N, T + 1)
        self.caches = [torch.empty(self.rows, 2 * d, dtype=dtype, device=dev) for _ in dec.decoders]
        self.hidden = torch.zeros(self.rows + 1, d, dtype=dtype, device=dev)

    def self_attention(self, i, layer, qkv):
        st = self.state
        return self.ops.mha_step_paths(qkv, self.caches[i], st.path, st.in_len, st.new_row, st.need, self.H)

    def decode(self):
        """The decoder step of the R rows at their own positions; rows without `need` ride along and store nothing (their
        hidden row goes to the dump row).  Returns its launches."""
        st = self.state
        x = self.decoder_pass(st.in_token, st.in_pos)
        self.hidden.index_copy_(0, st.store_row.long(), x)         # the masked store: rows without need land in the dump row
        return pass_launches(self.dec) + 2

    def frame(self, t: int, last: bool):
        ops, dec, st = self.ops, self.dec, self.state
        n = 1
        logits = None
        if self.use_dec:
            rows = self.hidden.index_select(0, st.row_of_slot)
            logits = self.proj(rows, dec.output_layer.weight, dec.output_layer.bias)
            n += 2
        ops.joint_frame(st, t, logits, self.V, self.lens, *self.weights, self.blank)
        if self.use_dec and not last:
            n += self.decode()
        self.launches = max(self.launches, n)

    def read(self, packed: torch.Tensor):
        """Every read of the device by a call goes through here and is counted (stats["host_reads"])."""
        self.reads += 1
        return packed.cpu().numpy()


def _search_kernels(model, encoder_out, lens, ctc_probs, ctc_w, N, C, bonus, blank, blank_threshold, return_trace):
    eng = _Engine(model, encoder_out, lens, ctc_probs, N, C, ctc_w, 1.0 - ctc_w, bonus, blank, blank_threshold)
    st, B, T, R = eng.state, eng.B, eng.T, eng.R
    if eng.use_dec:
        eng.decode()                                               # round 0: [sos], once per utterance
    for t in range(T):
        eng.frame(t, t == T - 1)
    got = eng.ops.joint_collect(st)
    ints = [got["len"], got["tok"], got["start"], got["end"], st.evals, st.executed, st.n_nodes]
    if return_trace:
        ints += [st.trace_node, st.trace_exec, st.parent, st.token]
    f64s = [got["att_conf"], got["ctc_conf"].double(), st.score] + ([st.trace_score] if return_trace else [])
    packed = eng.read(torch.cat([x.reshape(-1).double() for x in ints] + [x.reshape(-1) for x in f64s]))         # the one read
    at = 0

    def take(x, kind=np.int64):
        nonlocal at
        out = packed[at:at + x.numel()].reshape(tuple(x.shape))
        at += x.numel()
        return out.astype(kind) if kind is not None else out
    ln, tok, start, end, evals, executed, n_nodes = (take(x) for x in ints[:7])
    if return_trace:
        tnode, texec, parent, token = (take(x) for x in ints[7:])
    att_conf, ctc_conf, score = take(got["att_conf"], None), take(got["ctc_conf"], None), take(st.score, None)
    tscore = take(st.trace_score, None) if return_trace else None
    out = []
    for b in range(B):
        slots = [r for r in range(b * N, b * N + N) if ln[r] >= 0]
        stats = dict(decoder_evaluations=int(evals[b]), frames=int(lens[b]), frames_executed=int(executed[b]),
                     frames_skipped=int(lens[b]) - int(executed[b]), host_reads=eng.reads, launches_per_frame=eng.launches,
                     cache_bytes=eng.cache_bytes, rows=R, nodes=int(n_nodes[b]))
        trace = None
        if return_trace:
            def prefix(n, b=b):
                toks = []
                while n > 0:
                    toks.append(int(token[b, n]))
                    n = int(parent[b, n])
                return toks[::-1]
            trace = dict(beam=[], score=[], executed=[])
            for t in range(int(lens[b])):
                live = [r for r in range(b * N, b * N + N) if tnode[t, r] >= 0]
                trace["beam"].append([prefix(int(tnode[t, r])) for r in live])
                trace["score"].append([float(tscore[t, r]) for r in live])
                trace["executed"].append(bool(texec[t, b] == 1))
        if executed[b] == 0:                                       # every frame skipped (or none at all)
            out.append(DecodeResult(tokens=[], score=0.0, times=[], end_times=[], tokens_confidence=[], nbest=[[]],
                                    nbest_scores=[0.0], nbest_times=[[]], stats=stats, trace=trace))
            continue
        nbest = [tok[r, :ln[r]].tolist() for r in slots]
        conf = [[math.exp(max(float(ctc_conf[r, j]), float(att_conf[r, j]))) for j in range(ln[r])] for r in slots]
        stats["nbest_end_times"] = [end[r, :ln[r]].tolist() for r in slots]
        stats["nbest_tokens_confidence"] = conf
        r0 = slots[0]
        out.append(DecodeResult(tokens=nbest[0], score=float(score[r0]), times=start[r0, :ln[r0]].tolist(),
                                end_times=stats["nbest_end_times"][0], tokens_confidence=conf[0], nbest=nbest,
                                nbest_scores=[float(score[r]) for r in slots],
                                nbest_times=[start[r, :ln[r]].tolist() for r in slots], stats=stats, trace=trace))
    return out
