"""Float64 restatement of the attention decoder's second pass in plain torch, written from the definitions (the published WeNet
BiTransformerDecoder; attention_rescoring, wenet/transformer/search.py:364-448; forward_attention_decoder,
asr_model.py:876-986).  It imports nothing of the product: it reads a state dict by the upstream key names and runs the
reference's own recipe -- the memory repeated once per hypothesis, the hypotheses padded to the longest, pad and subsequent
masks, the full log-softmax, a gather.  `dtype` runs the same arithmetic in another precision (the float32 run is the
yardstick of the GPU tests' bounds)."""
import math

import torch


def _linear(sd, name, x):
    y = x @ sd[name + ".weight"].T
    return y + sd[name + ".bias"] if name + ".bias" in sd else y


def _layer_norm(sd, name, x, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * sd[name + ".weight"] + sd[name + ".bias"]


def mha(sd, name, heads, query, key, value, mask):
    """MultiHeadedAttention: mask (B, 1 or L, S) bool, True where the key is visible; hidden keys get -inf before the softmax
    and 0 after it."""
    B, L, D = query.shape
    dk = D // heads
    q = _linear(sd, name + ".linear_q", query).view(B, L, heads, dk).transpose(1, 2)
    k = _linear(sd, name + ".linear_k", key).view(B, -1, heads, dk).transpose(1, 2)
    v = _linear(sd, name + ".linear_v", value).view(B, -1, heads, dk).transpose(1, 2)
    scores = q @ k.transpose(-2, -1) / math.sqrt(dk)
    hidden = ~mask.unsqueeze(1)
    attn = torch.softmax(scores.masked_fill(hidden, -float("inf")), dim=-1).masked_fill(hidden, 0.0)
    x = (attn @ v).transpose(1, 2).reshape(B, L, D)
    return _linear(sd, name + ".linear_out", x)


def positional_encoding(length, d, dtype):
    """The sinusoid table is a float32 table by definition (wenet/transformer/embedding.py:47-56 builds it so), whatever
    precision the decoder then runs in."""
    pos = torch.arange(length, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(length, d, dtype=torch.float32)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.to(dtype)


def decoder_forward(sd, prefix, conf, memory, memory_mask, ys_in, ys_in_lens):
    """One TransformerDecoder: logits (B, L, V).  conf: heads, num_blocks (of this decoder), normalize_before, activation."""
    heads, pre = conf["heads"], conf["normalize_before"]
    act = {"relu": torch.relu, "swish": torch.nn.functional.silu, "tanh": torch.tanh}[conf.get("activation", "relu")]
    emb = sd[prefix + "embed.0.weight"]
    B, L = ys_in.shape
    d = emb.shape[1]
    x = emb[ys_in] * math.sqrt(d) + positional_encoding(L, d, emb.dtype)
    pad = torch.arange(L).unsqueeze(0) >= ys_in_lens.unsqueeze(1)                        # True on padding
    tgt_mask = ~pad[:, None, :] & torch.ones(L, L, dtype=torch.bool).tril()[None]
    for n in range(conf["num_blocks"]):
        p = f"{prefix}decoders.{n}."
        ff = lambda t: _linear(sd, p + "feed_forward.w_2", act(_linear(sd, p + "feed_forward.w_1", t)))      # noqa: E731
        if pre:
            y = _layer_norm(sd, p + "norm1", x)
            x = x + mha(sd, p + "self_attn", heads, y, y, y, tgt_mask)
            x = x + mha(sd, p + "src_attn", heads, _layer_norm(sd, p + "norm2", x), memory, memory, memory_mask)
            x = x + ff(_layer_norm(sd, p + "norm3", x))
        else:
            x = _layer_norm(sd, p + "norm1", x + mha(sd, p + "self_attn", heads, x, x, x, tgt_mask))
            x = _layer_norm(sd, p + "norm2", x + mha(sd, p + "src_attn", heads, x, memory, memory, memory_mask))
            x = _layer_norm(sd, p + "norm3", x + ff(x))
    if pre:
        x = _layer_norm(sd, prefix + "after_norm", x)
    return _linear(sd, prefix + "output_layer", x)


def score_attention(state_dict, conf, encoder_out, lens, hyps, sos, eos, reverse_weight, dtype=torch.float64):
    """state_dict: the decoder's own (keys left_decoder.* / right_decoder.* when conf["bidirectional"], else bare).
    Returns (l_logp, r_logp): [b][i] the L + 1 log-probabilities of hypothesis i of utterance b -- its tokens in order, then eos
    -- from the left decoder and (reverse_weight > 0; else None) from the right decoder over the reversed hypothesis, brought
    back into the hypothesis' order."""
    sd = {k: v.detach().to(dtype) for k, v in state_dict.items()}
    lp = "left_decoder." if conf["bidirectional"] else ""
    l_all, r_all = [], []
    for b, nbest in enumerate(hyps):
        n = len(nbest)
        if not n:
            l_all.append([])
            r_all.append([])
            continue
        Ls = [len(h) for h in nbest]
        W = max(Ls) + 1
        ys_in = torch.full((n, W), eos, dtype=torch.int64)
        r_ys_in = torch.full((n, W), eos, dtype=torch.int64)
        ys_in[:, 0] = r_ys_in[:, 0] = sos
        for i, h in enumerate(nbest):
            for j, w in enumerate(h):
                ys_in[i, 1 + j] = w
                r_ys_in[i, 1 + j] = h[len(h) - 1 - j]
        memory = encoder_out[b:b + 1, :lens[b]].to(dtype).repeat(n, 1, 1)
        memory_mask = torch.ones(n, 1, lens[b], dtype=torch.bool)
        in_lens = torch.tensor(Ls) + 1
        out = torch.log_softmax(decoder_forward(sd, lp, dict(conf, num_blocks=conf["num_blocks"]), memory, memory_mask, ys_in,
                                                in_lens), dim=-1)
        l_all.append([[out[i, j, w].item() for j, w in enumerate(h)] + [out[i, len(h), eos].item()] for i, h in enumerate(nbest)])
        if reverse_weight > 0:
            r_out = torch.log_softmax(decoder_forward(sd, "right_decoder.", dict(conf, num_blocks=conf["r_num_blocks"]), memory,
                                                      memory_mask, r_ys_in, in_lens), dim=-1)
            r_all.append([[r_out[i, len(h) - j - 1, w].item() for j, w in enumerate(h)] + [r_out[i, len(h), eos].item()]
                          for i, h in enumerate(nbest)])
    return l_all, (r_all if reverse_weight > 0 else None)


def rescore(first_scores, l_logp, r_logp, reverse_weight, ctc_weight, attn_weight=1.0, td=None, transducer_weight=0.0):
    """One utterance by hand (search.py:413-447; transducer.py:401-420): returns (final, attn, order, confidence,
    tokens_confidence), each per hypothesis in first-pass order; order by final, ties to the earlier rank (strict >)."""
    final, attn, conf, tcs = [], [], [], []
    for i, lt in enumerate(l_logp):
        score = sum(lt)
        tc = [math.exp(s) for s in lt[:-1]]
        if reverse_weight > 0:
            tc = [(c + math.exp(s)) / 2 for c, s in zip(tc, r_logp[i][:-1])]
            score = score * (1 - reverse_weight) + sum(r_logp[i]) * reverse_weight
        attn.append(score)
        conf.append(math.exp(score / len(lt)))
        tcs.append(tc)
        f = 0.0
        if attn_weight != 0:
            f += attn_weight * score
        if ctc_weight != 0:
            f += ctc_weight * first_scores[i]
        if td is not None and transducer_weight != 0:
            f += transducer_weight * td[i]
        final.append(f)
    left = list(range(len(final)))
    order = []
    while left:                                    # repeated strict-> selection: the earlier rank wins a tie
        best = left[0]
        for i in left[1:]:
            if final[i] > final[best]:
                best = i
        order.append(best)
        left.remove(best)
    return final, attn, order, conf, tcs
