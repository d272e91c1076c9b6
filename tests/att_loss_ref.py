"""Float64 restatement of the attention decoder's training loss in plain torch, written from the definitions (the reference's
_calc_att_loss, wenet/transformer/asr_model.py:251-292, LabelSmoothingLoss and th_accuracy).  It imports nothing of the
product: the decoder is tests/attn_decoder_ref.decoder_forward over a state dict, the loss is the KL sum against the smoothed
one-hot distribution over the full log-softmax.  `dtype` runs the same arithmetic in another precision."""
import torch

from tests.attn_decoder_ref import decoder_forward

IGNORE = -1


def lsm_rows(x, target, smoothing):
    """Per row of x (rows, V): the label-smoothing KL sum against target (ignored rows: 0), logsumexp, and whether the first
    index of the row's maximum is the target.  Differentiable in x; runs in x's dtype."""
    rows, V = x.shape
    logp = torch.log_softmax(x, dim=1)
    ignore = target == IGNORE
    dist = torch.full((rows, V), smoothing / (V - 1), dtype=x.dtype)
    dist[torch.arange(rows), target.masked_fill(ignore, 0)] = 1.0 - smoothing
    kl = torch.special.xlogy(dist, dist) - dist * logp                    # dist (log dist - logp), 0 log 0 = 0
    loss = kl.sum(1).masked_fill(ignore, 0.0)
    top = x.detach() == x.detach().max(1, keepdim=True).values
    first = torch.where(top, torch.arange(V)[None, :], torch.full((1, 1), V)).min(1).values
    return {"loss": loss, "lse": torch.logsumexp(x, dim=1), "correct": (first == target) & ~ignore}


def pad_tokens(texts, sos, eos):
    """texts: list of token lists -> (ys_in padded with eos, ys_out padded with IGNORE, the same for the reversed transcripts,
    in_lens)."""
    B, W = len(texts), max(len(t) for t in texts) + 1
    ys_in = torch.full((B, W), eos, dtype=torch.int64)
    r_in = torch.full((B, W), eos, dtype=torch.int64)
    ys_out = torch.full((B, W), IGNORE, dtype=torch.int64)
    r_out = torch.full((B, W), IGNORE, dtype=torch.int64)
    for b, t in enumerate(texts):
        L = len(t)
        ys_in[b, 0] = r_in[b, 0] = sos
        for j, w in enumerate(t):
            ys_in[b, 1 + j] = ys_out[b, j] = w
            r_in[b, 1 + j] = r_out[b, j] = t[L - 1 - j]
        ys_out[b, L] = r_out[b, L] = eos
    return ys_in, ys_out, r_in, r_out, torch.tensor([len(t) + 1 for t in texts])


def att_loss(sd, conf, encoder_out, lens, texts, sos, eos, reverse_weight, smoothing, length_normalized):
    """(loss, accuracy) from a decoder state dict `sd` (tensors of the dtype to run in, requires_grad where gradients are
    wanted; keys left_decoder.* / right_decoder.* when conf["bidirectional"]), conf as decoder_forward takes it plus
    r_num_blocks, encoder_out (B, T, D), lens (list) and the transcripts as token lists."""
    B, T, _ = encoder_out.shape
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1)
    ys_in, ys_out, r_in, r_out, in_lens = pad_tokens(texts, sos, eos)
    lp = "left_decoder." if conf["bidirectional"] else ""
    denom = int((ys_out != IGNORE).sum()) if length_normalized else B

    def term(prefix, blocks, tok, tgt):
        logits = decoder_forward(sd, prefix, dict(conf, num_blocks=blocks), encoder_out, mask, tok, in_lens)
        res = lsm_rows(logits.reshape(-1, logits.shape[-1]), tgt.reshape(-1), smoothing)
        return res["loss"].sum() / denom, res["correct"]

    loss, correct = term(lp, conf["num_blocks"], ys_in, ys_out)
    if reverse_weight > 0:
        r_loss, _ = term("right_decoder.", conf["r_num_blocks"], r_in, r_out)
        loss = loss * (1 - reverse_weight) + r_loss * reverse_weight
    return loss, correct.sum().item() / int((ys_out != IGNORE).sum())
