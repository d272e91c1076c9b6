"""Float64 restatement of the attention decoder's beam search (attention_beam_search, wenet/transformer/search.py:251-360) on
tests/attn_decoder_ref.decoder_forward.  It imports nothing of the product and keeps no cache: every step runs the full forward
of all prefixes and takes the last row's log-softmax, which is what forward_one_step is defined to give.  The loop is the
reference's, line for line -- the memory repeated per beam, scores [0, -inf, ...], mask_finished_scores / mask_finished_preds,
two topk, the cap range(1, maxlen + 1) on the padded length, lengths = hyps.ne(eos).sum(1) as float32 -- split in two (the loop,
and the final selection for a length penalty) so that one search serves several penalties, and it records, per step, what the
tests need to see that the search was exercised."""
import torch

from tests import attn_decoder_ref as REF


def step_logp(sd, prefix, conf, memory, memory_mask, hyps, dtype=torch.float64):
    """log p(next | prefix) (rows, V) of the prefixes hyps (rows, i), all of length i."""
    lens = torch.full((hyps.size(0),), hyps.size(1), dtype=torch.int64)
    logits = REF.decoder_forward(sd, prefix, conf, memory, memory_mask, hyps, lens)
    return torch.log_softmax(logits[:, -1], dim=-1)


def _mask_finished_scores(score, flag):
    n = score.size(-1)
    zero = torch.zeros_like(flag, dtype=torch.bool)
    if n > 1:
        unfinished = torch.cat((zero, flag.repeat([1, n - 1])), dim=1)
        finished = torch.cat((flag, zero.repeat([1, n - 1])), dim=1)
    else:
        unfinished, finished = zero, flag
    score.masked_fill_(unfinished, -float("inf"))
    score.masked_fill_(finished, 0)
    return score


def _mask_finished_preds(pred, flag, eos):
    return pred.masked_fill_(flag.repeat([1, pred.size(-1)]), eos)


def search(state_dict, conf, encoder_out, encoder_mask, sos, eos, beam_size=10, max_len=None, dtype=torch.float64):
    """Steps 1 and 2 of the reference's function.  state_dict / conf as attn_decoder_ref.score_attention takes them.  Returns
    dict(hyps (B, N, steps + 1) with the sos column; raw (B, N) the unpenalised scores; steps; flags: per step the (B, N) end
    flags AFTER the step; parent / token / score: per step (B * N) lists)."""
    sd = {k: v.detach().to(dtype) for k, v in state_dict.items()}
    prefix = "left_decoder." if conf["bidirectional"] else ""
    batch_size, maxlen, encoder_dim = encoder_out.shape
    cap = maxlen if max_len is None else min(maxlen, max_len)
    running_size = batch_size * beam_size
    memory = encoder_out.to(dtype).unsqueeze(1).repeat(1, beam_size, 1, 1).view(running_size, maxlen, encoder_dim)
    memory_mask = encoder_mask.unsqueeze(1).repeat(1, beam_size, 1, 1).view(running_size, 1, maxlen)
    hyps = torch.ones([running_size, 1], dtype=torch.long).fill_(sos)
    prefix_len = hyps.size(1)
    scores = torch.tensor([0.0] + [-float("inf")] * (beam_size - 1), dtype=torch.float)
    scores = scores.repeat([batch_size]).unsqueeze(1)
    end_flag = torch.zeros_like(scores, dtype=torch.bool)
    flags, parents, tokens, step_scores = [], [], [], []
    for i in range(prefix_len, cap + 1):
        if end_flag.sum() == running_size:
            break
        logp = step_logp(sd, prefix, conf, memory, memory_mask, hyps, dtype)
        top_k_logp, top_k_index = logp.topk(beam_size)
        top_k_logp = _mask_finished_scores(top_k_logp, end_flag)
        top_k_index = _mask_finished_preds(top_k_index, end_flag, eos)
        scores = scores + top_k_logp
        scores = scores.view(batch_size, beam_size * beam_size)
        scores, offset_k_index = scores.topk(k=beam_size)
        scores = scores.view(-1, 1)
        base_k_index = torch.arange(batch_size).view(-1, 1).repeat([1, beam_size])
        base_k_index = base_k_index * beam_size * beam_size
        best_k_index = base_k_index.view(-1) + offset_k_index.view(-1)
        best_k_pred = torch.index_select(top_k_index.view(-1), dim=-1, index=best_k_index)
        best_hyps_index = best_k_index // beam_size
        last_best_k_hyps = torch.index_select(hyps, dim=0, index=best_hyps_index)
        hyps = torch.cat((last_best_k_hyps, best_k_pred.view(-1, 1)), dim=1)
        end_flag = torch.eq(hyps[:, -1], eos).view(-1, 1)
        flags.append(end_flag.view(batch_size, beam_size).clone())
        parents.append((offset_k_index // beam_size).view(-1).tolist())
        tokens.append(best_k_pred.tolist())
        step_scores.append(scores.view(-1).tolist())
    return dict(hyps=hyps.view(batch_size, beam_size, -1), raw=scores.view(batch_size, beam_size), steps=len(flags), flags=flags,
                parent=parents, token=tokens, score=step_scores)


def finish(ref, eos, length_penalty):
    """Step 3 of the reference's function on search()'s result (prefix_len = 1): best, the token lists it returns; and, beyond
    it, nbest / nbest_scores: all beams of an utterance by penalised score, descending, ties to the lower slot."""
    hyps, raw = ref["hyps"], ref["raw"]
    batch_size, beam_size = raw.shape
    hyps = hyps.reshape(batch_size * beam_size, -1)
    prefix_len = 1
    lengths = hyps.ne(eos).sum(dim=1).view(batch_size, beam_size).float()
    scores = raw / lengths.pow(length_penalty)
    best_scores, best_index = scores.max(dim=-1)
    best_hyps_index = best_index + torch.arange(batch_size, dtype=torch.long) * beam_size
    best_hyps = torch.index_select(hyps, dim=0, index=best_hyps_index)
    best_hyps = best_hyps[:, prefix_len:]
    best = []
    for i in range(batch_size):
        hyp = best_hyps[i]
        hyp = hyp[hyp != eos]
        best.append(hyp.tolist())
    nbest, nbest_scores = [], []
    for b in range(batch_size):
        left, order = list(range(beam_size)), []
        while left:                                    # repeated strict-> selection: the lower slot wins a tie
            top = left[0]
            for i in left[1:]:
                if scores[b, i] > scores[b, top]:
                    top = i
            order.append(top)
            left.remove(top)
        rows = hyps.view(batch_size, beam_size, -1)[b, :, prefix_len:]
        nbest.append([[t for t in rows[i].tolist() if t != eos] for i in order])
        nbest_scores.append([scores[b, i].item() for i in order])
    return dict(best=best, nbest=nbest, nbest_scores=nbest_scores, scores=scores)
