"""Second pass with the attention decoder (reference: attention_rescoring, wenet/transformer/search.py:364-448;
forward_attention_decoder, asr_model.py:876-986; transducer_attention_rescoring, wenet/transducer/transducer.py:288-425).

score_attention gives, for every hypothesis y of every utterance, the left-to-right score
    sum_j log p(y_j | y_<j, x) + log p(eos | y, x)
of the left decoder, the same over the reversed hypothesis from the right decoder, and the per-token log-probabilities.

backend "framework" is the reference's recipe as framework ops: per utterance the memory repeated once per hypothesis, the
hypotheses padded to the longest, masks, the full (beam, L + 1, V) log-softmax, a gather.

backend "kernels" packs instead.  All hypotheses of all utterances are rows without padding -- hypothesis i owns L_i + 1 rows
([sos] + y) -- and the encoder output is never repeated: per layer the cross-attention K | V of an utterance is ONE projection
of its T'_b rows by the stacked [linear_k; linear_v] weight, shared by all its hypotheses.  The layer body is
decoder_rows.decoder_layers (which the two searches run too); this module supplies the tables and the causal self-attention.
Every nn.Linear runs on this library's GEMMs (decoder_rows.proj: hip_ops.linear_fused / linear_bias_act / gemm_f32 / gemm_bf16,
and gemm_ph_ex for long fp32 inputs with a residual: the framework's fp32 GEMM is the two-stream stall of DESIGN.md section 4),
every LayerNorm on hip_ops.add_layernorm, both attentions on hip_ops.mha_rows (one launch per attention for all hypotheses and heads; on packed
rows `causal` equals the reference's pad-and-subsequent mask for every row that is scored), and hip_ops.logp_gather_rows reads
log p(target) of a row straight from the logits: the (rows, V) log-softmax is never formed, and the output_layer GEMM runs
over chunks of utterances so the logits never exceed LOGITS_CAP_BYTES.  One upload (the int32 tables) and one read of the
device (the rows' log-probabilities) per call."""
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .decoder_rows import (KERNEL_ACTS, CrossAttention, decoder_layers, decoder_proj, embed_rows,    # noqa: F401 (re-exports)
                           kernels_unmet, left_right, position_table, upload_tables)
from .search import DecodeResult

ATTN_RESCORING_MODES = ("attention_rescoring", "ctc_beam_td_attn_rescoring", "rnnt_beam_attn_rescoring")
LOGITS_CAP_BYTES = 64 << 20        # the logits of one output_layer chunk: 3355 fp32 rows at V = 5000


class AttentionScores:
    """Per utterance b and hypothesis i: l2r[b][i] the left decoder's score and l2r_logp[b][i] its L + 1 terms (the tokens
    in order, then eos); r2l / r2l_logp the right decoder's (None when reverse_weight is 0), r2l_logp[b][i][j] being the term
    of token y_j -- the hypothesis' order, as the reference pairs the two directions -- and the last one eos.
    stats: what the kernels backend counted for this call (rows, hypotheses, memory_rows, chunks, logits_peak_bytes); None from
    the framework backend."""

    def __init__(self, l2r, l2r_logp, r2l=None, r2l_logp=None, stats: Optional[dict] = None):
        self.l2r, self.l2r_logp, self.r2l, self.r2l_logp, self.stats = l2r, l2r_logp, r2l, r2l_logp, stats

    def attn(self, reverse_weight: float) -> List[List[float]]:
        """attn_i = l2r_i, or (1 - rw) l2r_i + rw r2l_i (search.py:434)."""
        if reverse_weight > 0 and self.r2l is not None:
            return [[a * (1 - reverse_weight) + r * reverse_weight for a, r in zip(la, lr)] for la, lr in zip(self.l2r, self.r2l)]
        return [list(la) for la in self.l2r]


def check_tokens(hyps: Sequence[Sequence[Sequence[int]]], vocab_size: int) -> None:
    """ValueError, naming utterance and hypothesis, for a token outside [0, vocab_size).  (No length limit: the 2558 tokens of
    transducer.search.rescoring.check_hypotheses are the lattice kernel's, and attention has no blank to refuse.)"""
    for b, nbest in enumerate(hyps):
        for i, h in enumerate(nbest):
            if not len(h):
                continue
            toks = np.asarray(h, dtype=np.int64)
            bad = toks[(toks < 0) | (toks >= vocab_size)]
            if bad.size:
                raise ValueError(f"utterance {b}, hypothesis {i}: token {int(bad[0])} outside the vocabulary [0, {vocab_size})")


def _regroup(flat: list, hyps) -> list:
    out, at = [], 0
    for nbest in hyps:
        out.append(flat[at:at + len(nbest)])
        at += len(nbest)
    return out


@torch.no_grad()
def score_attention(model, encoder_out: torch.Tensor, encoder_lens, hyps: Sequence[Sequence[Sequence[int]]],
                    reverse_weight: float = 0.0, backend: Optional[str] = None) -> AttentionScores:
    from ..transducer.search.rescoring import check_score_backend
    decoder = getattr(model, "decoder", None)
    if decoder is None:
        raise NotImplementedError("score_attention: the model has no attention decoder (init_model builds one with "
                                  "args.attention_decoder)")
    _, right = left_right(decoder)
    if reverse_weight > 0 and right is None:
        raise ValueError(f"reverse_weight = {reverse_weight} needs the right_decoder of a bitransformer decoder")
    backend = check_score_backend(backend, encoder_out.is_cuda)
    lens = [int(v) for v in (encoder_lens.tolist() if isinstance(encoder_lens, torch.Tensor) else encoder_lens)]
    if len(hyps) != encoder_out.size(0) or len(lens) != encoder_out.size(0):
        raise ValueError(f"{encoder_out.size(0)} utterances, {len(hyps)} n-best lists, {len(lens)} lengths")
    check_tokens(hyps, model.vocab_size)
    for b, nbest in enumerate(hyps):
        if len(nbest) and not 1 <= lens[b] <= encoder_out.size(1):
            raise ValueError(f"utterance {b}: {lens[b]} frames of {encoder_out.size(1)}")
    use_right = reverse_weight > 0
    stats = None
    if backend == "framework":
        l_lp, r_lp = _score_framework(model, encoder_out, lens, hyps, reverse_weight)
    else:
        l_lp, r_lp, stats = _score_kernels(model, encoder_out, lens, hyps, use_right)
    l2r = [[math.fsum(t) for t in nb] for nb in l_lp]
    if not use_right:
        return AttentionScores(l2r, l_lp, stats=stats)
    return AttentionScores(l2r, l_lp, [[math.fsum(t) for t in nb] for nb in r_lp], r_lp, stats)


def _score_framework(model, encoder_out, lens, hyps, reverse_weight):
    decoder, sos, eos = model.decoder, model.sos, model.eos
    dev = encoder_out.device
    dtype = next(decoder.parameters()).dtype
    l_all, r_all = [], []
    for b, nbest in enumerate(hyps):              # one utterance at a time: its hypotheses are the reference's batch
        n = len(nbest)
        if not n:
            l_all.append([])
            r_all.append([])
            continue
        Ls = [len(h) for h in nbest]
        W = max(Ls) + 1
        ys_in = torch.full((n, W), eos, dtype=torch.int64)              # add_sos_eos pads the decoder's input with eos
        r_ys_in = torch.full((n, W), eos, dtype=torch.int64)
        tgt = torch.full((n, W), eos, dtype=torch.int64)                # y_0 .. y_{L-1}, eos at L
        r_tgt = torch.full((n, W), eos, dtype=torch.int64)
        ys_in[:, 0] = sos
        r_ys_in[:, 0] = sos
        for i, h in enumerate(nbest):
            if Ls[i]:
                t = torch.tensor(list(h), dtype=torch.int64)
                ys_in[i, 1:Ls[i] + 1] = t
                tgt[i, :Ls[i]] = t
                r_ys_in[i, 1:Ls[i] + 1] = t.flip(0)
                r_tgt[i, :Ls[i]] = t.flip(0)
        memory = encoder_out[b:b + 1, :lens[b]].to(dtype).repeat(n, 1, 1)
        mask = torch.ones(n, 1, lens[b], dtype=torch.bool, device=dev)
        l_x, r_x, _ = decoder(memory, mask, ys_in.to(dev), (torch.tensor(Ls) + 1).to(dev), r_ys_in.to(dev), reverse_weight)
        lp = torch.log_softmax(l_x, dim=-1).gather(2, tgt.to(dev).unsqueeze(-1)).squeeze(-1).tolist()
        l_all.append([lp[i][:Ls[i] + 1] for i in range(n)])
        if reverse_weight > 0:
            rp = torch.log_softmax(r_x, dim=-1).gather(2, r_tgt.to(dev).unsqueeze(-1)).squeeze(-1).tolist()
            r_all.append([rp[i][:Ls[i]][::-1] + [rp[i][Ls[i]]] for i in range(n)])
    return l_all, r_all


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels backend
# ---------------------------------------------------------------------------------------------------------------------------

def _logits_chunks(utt_row_end: List[int], cap_rows: int) -> List[tuple]:
    """Row ranges for the output_layer GEMM: whole utterances while they fit under cap_rows, an utterance that alone exceeds
    the cap in pieces of cap_rows."""
    chunks, a = [], 0
    for i, e in enumerate(utt_row_end):
        nxt = utt_row_end[i + 1] if i + 1 < len(utt_row_end) else None
        if nxt is not None and nxt - a <= cap_rows:
            continue                                        # the next utterance still fits: keep growing
        while e - a > cap_rows:
            chunks.append((a, a + cap_rows))
            a += cap_rows
        if e > a:
            chunks.append((a, e))
            a = e
    return chunks


def _score_kernels(model, encoder_out, lens, hyps, use_right: bool):
    from .. import hip_ops
    from .._lib import PafcError
    unmet = kernels_unmet(model, encoder_out, use_right)
    if unmet is not None:
        raise PafcError(f"score_attention(backend='kernels'): {unmet}")
    left, right = left_right(model.decoder)
    sos, eos = model.sos, model.eos
    dev = encoder_out.device
    flat = [(b, list(h)) for b, nbest in enumerate(hyps) for h in nbest]
    if not flat:
        return [[] for _ in hyps], [[] for _ in hyps], dict(rows=0, hypotheses=0, memory_rows=0, chunks=0,
                                                            logits_peak_bytes=0)
    # the memory rows of the utterances that have hypotheses, without padding
    used = [b for b, nbest in enumerate(hyps) if len(nbest)]
    T = encoder_out.size(1)
    dtype = left.after_norm.weight.dtype
    if all(lens[b] == T for b in used) and encoder_out.is_contiguous():
        memory = encoder_out.reshape(-1, encoder_out.size(2))
        mem_row = {b: b * T for b in used}
    else:
        memory = torch.cat([encoder_out[b, :lens[b]] for b in used])
        mem_row, at = {}, 0
        for b in used:
            mem_row[b] = at
            at += lens[b]
    memory = memory.to(dtype)
    # the tables: one int32 array, one upload
    G = len(flat)
    Ls = np.array([len(h) for _, h in flat], dtype=np.int64)
    q_off = np.concatenate([[0], np.cumsum(Ls + 1)])
    R = int(q_off[-1])
    tok_l, tok_r, tgt_l, tgt_r = (np.empty(R, dtype=np.int64) for _ in range(4))
    pos = np.empty(R, dtype=np.int64)
    for n, (_, h) in enumerate(flat):
        a, e = int(q_off[n]), int(q_off[n + 1])
        tok_l[a] = tok_r[a] = sos
        tok_l[a + 1:e] = tgt_l[a:e - 1] = h
        tok_r[a + 1:e] = tgt_r[a:e - 1] = h[::-1]
        tgt_l[e - 1] = tgt_r[e - 1] = eos
        pos[a:e] = np.arange(e - a)
    fields = [tok_l, tok_r, tgt_l, tgt_r, pos, q_off, Ls + 1, [mem_row[b] for b, _ in flat], [lens[b] for b, _ in flat]]
    tok_l, tok_r, tgt_l, tgt_r, pos, q_off_d, self_len, mem_off, mem_len = upload_tables(fields, dev)
    utt_row_end, n = [], 0
    for b in used:
        n += len(hyps[b])
        utt_row_end.append(int(q_off[n]))
    V = left.output_layer.weight.size(0)
    cap_rows = max(1, LOGITS_CAP_BYTES // (V * memory.element_size()))
    chunks = _logits_chunks(utt_row_end, cap_rows)
    proj = decoder_proj(model, "score_attention")
    d, H = memory.size(1), left.attention_heads
    cross = CrossAttention(q_off_d, mem_off, mem_len, memory=memory)     # K | V once per utterance row, for all its hypotheses
    self_attention = lambda i, layer, qkv: hip_ops.mha_rows(        # causal over a hypothesis' own rows          # noqa: E731
        qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], q_off_d, q_off_d[:-1], self_len, H, True)
    logp = torch.empty((2 if use_right else 1) * R, dtype=torch.float32, device=dev)
    peak = 0
    for i, (dec, tok, tgt) in enumerate([(left, tok_l, tgt_l)] + ([(right, tok_r, tgt_r)] if use_right else [])):
        pe = position_table(dec, int(Ls.max()) + 1, dev, dtype)
        x = decoder_layers(dec, embed_rows(dec, pe, tok, pos), self_attention, cross, proj)
        for a, e in chunks:
            logits = proj(x[a:e], dec.output_layer.weight, dec.output_layer.bias)
            peak = max(peak, logits.numel() * logits.element_size())
            hip_ops.logp_gather_rows(logits, tgt[a:e], out=logp[i * R + a:i * R + e])
    host = logp.tolist()                                                   # the one read of the device
    stats = dict(rows=R, hypotheses=G, memory_rows=memory.size(0), chunks=len(chunks), logits_peak_bytes=peak)
    l_flat = [host[int(q_off[n]):int(q_off[n + 1])] for n in range(G)]
    r_flat = []
    if use_right:
        for n in range(G):
            t = host[R + int(q_off[n]):R + int(q_off[n + 1])]
            r_flat.append(t[:-1][::-1] + t[-1:])
    return _regroup(l_flat, hyps), (_regroup(r_flat, hyps) if use_right else []), stats


# ---------------------------------------------------------------------------------------------------------------------------
# the decode modes
# ---------------------------------------------------------------------------------------------------------------------------

def attention_rescore(first_pass: List[DecodeResult], scores: AttentionScores, reverse_weight: float, ctc_weight: float,
                      attn_weight: float = 1.0, td_scores: Optional[List[List[float]]] = None,
                      transducer_weight: float = 0.0) -> List[DecodeResult]:
    """final_i = attn_weight * attn_i + ctc_weight * first_pass_score_i + transducer_weight * td_i with attn_i of
    AttentionScores.attn (search.py:413-440 is attn_weight = 1 without td; transducer.py:401-420 the general form); the n-best
    list re-ordered by final, descending and stable, so on ties the earlier first-pass rank wins, as
    transducer.search.rescoring.rescore does.  Per result confidence = exp(attn / (len + 1)) and tokens_confidence =
    exp(logp_j), averaged with the right-to-left value when reverse_weight > 0 (search.py:415-447); nbest_attn_scores holds the
    raw attn_i (nbest_td_scores the raw td_i) in the new order."""
    attn_all = scores.attn(reverse_weight)
    both = reverse_weight > 0 and scores.r2l_logp is not None
    out = []
    for b, r in enumerate(first_pass):
        nbest = r.nbest if r.nbest is not None else [r.tokens]
        first = r.nbest_scores if r.nbest_scores is not None else [r.score]
        attn = attn_all[b]
        td = td_scores[b] if td_scores is not None else None
        assert len(attn) == len(nbest) == len(first) and (td is None or len(td) == len(nbest))
        if not nbest:
            out.append(DecodeResult(tokens=[], score=r.score, nbest=[], nbest_scores=[], nbest_attn_scores=[],
                                    nbest_td_scores=None if td is None else []))
            continue
        # (a zero weight drops its term: 0 * -inf of an unreachable first-pass entry must not turn the sum into NaN)
        final = [(attn_weight * a if attn_weight != 0 else 0.0) + (ctc_weight * s if ctc_weight != 0 else 0.0)
                 + (transducer_weight * td[i] if (td is not None and transducer_weight != 0) else 0.0)
                 for i, (a, s) in enumerate(zip(attn, first))]
        order = sorted(range(len(nbest)), key=lambda i: -final[i])          # (sorted is stable)
        best = order[0]
        tc = [math.exp(v) for v in scores.l2r_logp[b][best][:-1]]
        if both:
            tc = [(c + math.exp(v)) / 2 for c, v in zip(tc, scores.r2l_logp[b][best][:-1])]
        ntimes = None if r.nbest_times is None else [r.nbest_times[i] for i in order]
        out.append(DecodeResult(tokens=nbest[best], score=final[best], confidence=math.exp(attn[best] / (len(nbest[best]) + 1)),
                                tokens_confidence=tc, times=None if ntimes is None else ntimes[0],
                                nbest=[nbest[i] for i in order], nbest_scores=[final[i] for i in order], nbest_times=ntimes,
                                nbest_td_scores=None if td is None else [td[i] for i in order],
                                nbest_attn_scores=[attn[i] for i in order]))
    return out
