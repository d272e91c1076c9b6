"""Limited-context attention with the positional term (`limited_rel_selfattn`, global_tokens = 0), restated densely in plain
torch from its definition -- test infrastructure, imports nothing of the product.

With w the context on either side, T frames and t_pad >= T (the reference pads to the next multiple of 2 w), query i sees
the keys j with |j - i| <= w and 0 <= j < t_pad.  A real key (j < T) scores
    s_ij = ((q_i + u_h) . k_j + (q_i + v_h) . p_j) / sqrt(d_k)            p_j: the KEY's position row, no relative shift
and the keys of [T, t_pad) are zero padding that is NOT masked: score 0, value 0 -- each adds exp(0 - max) to the denominator
of the queries that see it and nothing to the numerator.  No length mask is applied: padded frames of a batch row are keys.
Everything runs in the dtype of the inputs (float64 for the truth, float32 for the yardstick of a tolerance)."""
import math

import torch


def reference_t_pad(T: int, w: int) -> int:
    return -(-T // (2 * w)) * 2 * w


def band_attention(q, k, v, p, u, vb, w: int, t_pad: int, round_biased_q=None):
    """q, k, v (B, T, H, dk); p (T, H, dk); u, vb (H, dk) -> (B, T, H, dk).  round_biased_q: a function applied to q + u and
    q + v (a bf16 module rounds them once more)."""
    B, T, H, dk = q.shape
    qu, qv = q + u, q + vb
    if round_biased_q is not None:
        qu, qv = round_biased_q(qu), round_biased_q(qv)
    s = (torch.einsum("bihd,bjhd->bhij", qu, k) + torch.einsum("bihd,jhd->bhij", qv, p)) / math.sqrt(dk)
    i = torch.arange(T).unsqueeze(1)
    j = torch.arange(T).unsqueeze(0)
    s = s.masked_fill(((j - i).abs() > w).to(s.device), -float("inf"))
    # the unmasked padding keys of query i: those of [T, t_pad) within w of it
    n0 = (torch.clamp(torch.arange(T) + w, max=t_pad - 1) - T + 1).clamp(min=0).to(device=s.device, dtype=s.dtype)
    n0 = n0.view(1, 1, T, 1)
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(n0 > 0, m.clamp(min=0.0), m)
    e = torch.exp(s - m)
    den = e.sum(dim=-1, keepdim=True) + n0 * torch.exp(-m)
    return torch.einsum("bhij,bjhd->bihd", e / den, v)


def lca_attention(x, pos_emb, sd, heads: int, w: int, t_pad=None):
    """The module: x (B, T, D), pos_emb (1, T, D), sd the state dict (linear_q/k/v/out, linear_pos, pos_bias_u/v) in x's
    dtype -> (out (B, T, D), cache (B, H, T, 2 dk) = cat(k, v))."""
    B, T, D = x.shape
    dk = D // heads
    lin = lambda t, n: t @ sd[n + ".weight"].T + (sd[n + ".bias"] if n + ".bias" in sd else 0)
    q = lin(x, "linear_q").view(B, T, heads, dk)
    k = lin(x, "linear_k").view(B, T, heads, dk)
    v = lin(x, "linear_v").view(B, T, heads, dk)
    p = (pos_emb[0] @ sd["linear_pos.weight"].T).view(T, heads, dk)
    att = band_attention(q, k, v, p, sd["pos_bias_u"], sd["pos_bias_v"], w, reference_t_pad(T, w) if t_pad is None else t_pad)
    out = lin(att.reshape(B, T, D), "linear_out")
    return out, torch.cat((k.transpose(1, 2), v.transpose(1, 2)), dim=-1)


def position_rows(offset: int, size: int, d: int, dtype=torch.float64):
    """Rows [offset, offset + size) of the sinusoid table, (1, size, d), computed in float32 as the reference's table is."""
    pos = torch.arange(offset, offset + size, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(size, d)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.unsqueeze(0).to(dtype)
