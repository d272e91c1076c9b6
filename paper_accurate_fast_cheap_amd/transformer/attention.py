"""MultiHeadedAttention of the attention decoder (reference: wenet/transformer/attention.py:28-200): scaled dot-product
attention, parameters linear_q / linear_k / linear_v / linear_out.  Masked keys get -inf before the softmax and 0 after it
(:112-118), so a query without a visible key yields zeros.  This module is the definition and the "framework" backend; the
second pass on the GPU packs the rows and runs hip_ops.mha_rows instead (transformer/attn_rescore.py)."""
import math
from typing import Optional

import torch


class MultiHeadedAttention(torch.nn.Module):
    def __init__(self, n_head: int, n_feat: int, dropout_rate: float, key_bias: bool = True):
        super().__init__()
        assert n_feat % n_head == 0
        self.d_k = n_feat // n_head
        self.h = n_head
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat, bias=key_bias)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)
        self.dropout = torch.nn.Dropout(p=dropout_rate)

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
        """query (B, L, D), key / value (B, S, D); mask (B, 1, S) or (B, L, S) bool, True where a key is visible, or None."""
        B = query.size(0)
        q = self.linear_q(query).view(B, -1, self.h, self.d_k).transpose(1, 2)
        k = self.linear_k(key).view(B, -1, self.h, self.d_k).transpose(1, 2)
        v = self.linear_v(value).view(B, -1, self.h, self.d_k).transpose(1, 2)
        scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(self.d_k)
        if mask is not None and mask.size(-1) > 0:
            hidden = ~mask.unsqueeze(1)[..., :scores.size(-1)]                   # (B, 1, 1 or L, S)
            attn = torch.softmax(scores.masked_fill(hidden, -float("inf")), dim=-1).masked_fill(hidden, 0.0)
        else:
            attn = torch.softmax(scores, dim=-1)
        x = torch.matmul(self.dropout(attn), v)
        x = x.transpose(1, 2).contiguous().view(B, -1, self.h * self.d_k)
        return self.linear_out(x)
