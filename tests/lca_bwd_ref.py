"""The backward of limited-context attention with the positional term (tests/lca_ref.band_attention), written out densely in
plain torch from its formulas -- test infrastructure, imports nothing of the product.

Per batch row b and head h, with qu_i = q_i + u_h, qv_i = q_i + vb_h and the band |j - i| <= w over the real keys j < T:
    s_ij  = (qu_i . k_j + qv_i . p_j) / sqrt(dk)
    n0_i  = max(0, min(t_pad - 1, i + w) - T + 1)            the unmasked padding keys of query i: score 0, value 0
    lse_i = log(sum_j exp(s_ij) + n0_i),  P_ij = exp(s_ij - lse_i),  out_i = sum_j P_ij v_j
    delta_i = dout_i . out_i,  dS_ij = P_ij (dout_i . v_j - delta_i)                 (no gradient flows to a padding key)
    dqu_i = sum_j dS_ij k_j / sqrt(dk),  dqv_i = sum_j dS_ij p_j / sqrt(dk),  dq_i = dqu_i + dqv_i
    dk_j  = sum_i dS_ij qu_i / sqrt(dk),  dv_j = sum_i P_ij dout_i
    dp_j  = sum_b sum_i dS_ij qv_i / sqrt(dk)               the position rows are shared by the batch
    du_h  = sum_{b,i} dqu_i,  dvb_h = sum_{b,i} dqv_i
`fault` plants one of four mistakes, so that the test of this file can show it would notice them."""
import math

import torch

H, DK = 2, 64
FAULTS = ("n0_left_out_of_lse", "dp_not_summed_over_batch", "du_from_dq", "band_off_by_one")

# (B, T, w, t_pad); None: the reference's t_pad (T rounded up to a multiple of 2 w)
CASES = [
    (1, 1, 2, None),        # a single frame
    (2, 5, 2, None),        # small batch, padding keys
    (1, 16, 4, None),       # T a multiple of 2 w: no padding keys
    (1, 33, 0, 33),         # w = 0: self only
    (2, 67, 16, None),      # t_pad 96, padding keys
    (3, 131, 5, None),      # band narrower than a tile, three query tiles, three-way dp sum
    (1, 97, 16, 97),        # explicit t_pad = T
    (1, 200, 40, None),     # band wider than a bf16 key tile, t_pad 240
    (2, 70, 100, None),     # w >= T: full attention, every query has padding keys
]


def t_pad_of(T: int, w: int, t_pad):
    if t_pad is not None:
        return t_pad
    return -(-T // (2 * w)) * 2 * w if w > 0 else T


def case_inputs(B: int, T: int, seed: int):
    """float64 (q, k, v (B, T, H, dk), p (T, H, dk), u, vb (H, dk), dout (B, T, H, dk)); p, u and vb smaller than q, as the
    position rows and the biases of a model are."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)         # noqa: E731
    return (rnd(B, T, H, DK), rnd(B, T, H, DK), rnd(B, T, H, DK), rnd(T, H, DK) * 0.7, rnd(H, DK) * 0.5, rnd(H, DK) * 0.5,
            rnd(B, T, H, DK))


def band_attention_bwd(q, k, v, p, u, vb, dout, w: int, t_pad: int, round_biased_q=None, fault=None):
    """q, k, v, dout (B, T, H, dk); p (T, H, dk); u, vb (H, dk) -> (dq, dk, dv (B, T, H, dk), dp (T, H, dk), du, dvb (H, dk),
    lse (B, T, H)) in the dtype of the inputs.  round_biased_q as in lca_ref.band_attention (its rounding is treated as the
    identity by the backward)."""
    assert fault is None or fault in FAULTS
    B, T, _, dk = q.shape
    scale = 1.0 / math.sqrt(dk)
    qu, qv = q + u, q + vb
    if round_biased_q is not None:
        qu, qv = round_biased_q(qu), round_biased_q(qv)
    s = (torch.einsum("bihd,bjhd->bhij", qu, k) + torch.einsum("bihd,jhd->bhij", qv, p)) * scale
    i = torch.arange(T).unsqueeze(1)
    j = torch.arange(T).unsqueeze(0)
    reach = w - 1 if fault == "band_off_by_one" else w
    s = s.masked_fill((j - i).abs() > reach, -float("inf"))
    n0 = (torch.clamp(torch.arange(T) + w, max=t_pad - 1) - T + 1).clamp(min=0).to(s.dtype).view(1, 1, T)
    if fault == "n0_left_out_of_lse":
        n0 = torch.zeros_like(n0)
    m = s.max(dim=-1).values
    m = torch.where(n0 > 0, m.clamp(min=0.0), m)
    lse = m + torch.log(torch.exp(s - m.unsqueeze(-1)).sum(dim=-1) + n0 * torch.exp(-m))            # (B, H, T)
    P = torch.exp(s - lse.unsqueeze(-1))
    out = torch.einsum("bhij,bjhd->bihd", P, v)
    delta = (dout * out).sum(dim=-1).permute(0, 2, 1)                                                 # (B, H, T)
    dS = P * (torch.einsum("bihd,bjhd->bhij", dout, v) - delta.unsqueeze(-1))
    dqu = torch.einsum("bhij,bjhd->bihd", dS, k) * scale
    dqv = torch.einsum("bhij,jhd->bihd", dS, p) * scale
    dq = dqu + dqv
    dk_ = torch.einsum("bhij,bihd->bjhd", dS, qu) * scale
    dv_ = torch.einsum("bhij,bihd->bjhd", P, dout)
    dp_b = torch.einsum("bhij,bihd->bjhd", dS, qv) * scale
    dp_ = dp_b[0] if fault == "dp_not_summed_over_batch" else dp_b.sum(dim=0)
    du = (dq if fault == "du_from_dq" else dqu).sum(dim=(0, 1))
    dvb = dqv.sum(dim=(0, 1))
    return dq, dk_, dv_, dp_, du, dvb, lse.permute(0, 2, 1)
