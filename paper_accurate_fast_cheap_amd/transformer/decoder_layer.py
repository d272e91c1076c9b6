"""DecoderLayer of the attention decoder (the published WeNet layer, wenet/transformer/decoder_layer.py, which the reference's
release omits): self-attention, source attention over the encoder memory and a feed-forward block, each with a residual.
Pre-norm (normalize_before) applies norm1 / norm2 / norm3 to a block's input, post-norm to its residual sum."""
from typing import Optional

import torch


class DecoderLayer(torch.nn.Module):
    def __init__(self, size: int, self_attn: torch.nn.Module, src_attn: torch.nn.Module, feed_forward: torch.nn.Module,
                 dropout_rate: float, normalize_before: bool = True):
        super().__init__()
        self.size = size
        self.self_attn = self_attn
        self.src_attn = src_attn
        self.feed_forward = feed_forward
        self.norm1 = torch.nn.LayerNorm(size, eps=1e-5)
        self.norm2 = torch.nn.LayerNorm(size, eps=1e-5)
        self.norm3 = torch.nn.LayerNorm(size, eps=1e-5)
        self.dropout = torch.nn.Dropout(dropout_rate)
        self.normalize_before = normalize_before

    def forward(self, tgt: torch.Tensor, tgt_mask: torch.Tensor, memory: torch.Tensor, memory_mask: torch.Tensor,
                cache: Optional[torch.Tensor] = None):
        """tgt (B, L, D), tgt_mask (B, L, L), memory (B, S, D), memory_mask (B, 1, S) -> (tgt, tgt_mask, memory, memory_mask).
        cache (B, L - 1, D), the layer's output for the rows before the last (forward_one_step): only the last query row is
        computed -- its keys and values are still those of all L rows -- and the result is concatenated behind the cache."""
        if cache is not None:
            return self._forward_last_row(tgt, tgt_mask, memory, memory_mask, cache)
        x = tgt
        if self.normalize_before:
            y = self.norm1(x)
            x = x + self.dropout(self.self_attn(y, y, y, tgt_mask))
            x = x + self.dropout(self.src_attn(self.norm2(x), memory, memory, memory_mask))
            x = x + self.dropout(self.feed_forward(self.norm3(x)))
        else:
            x = self.norm1(x + self.dropout(self.self_attn(x, x, x, tgt_mask)))
            x = self.norm2(x + self.dropout(self.src_attn(x, memory, memory, memory_mask)))
            x = self.norm3(x + self.dropout(self.feed_forward(x)))
        return x, tgt_mask, memory, memory_mask

    def _forward_last_row(self, tgt, tgt_mask, memory, memory_mask, cache):
        assert cache.shape == (tgt.shape[0], tgt.shape[1] - 1, self.size), f"{tuple(cache.shape)} for tgt {tuple(tgt.shape)}"
        x, q_mask = tgt[:, -1:], tgt_mask[:, -1:]
        if self.normalize_before:
            y = self.norm1(tgt)
            x = x + self.dropout(self.self_attn(y[:, -1:], y, y, q_mask))
            x = x + self.dropout(self.src_attn(self.norm2(x), memory, memory, memory_mask))
            x = x + self.dropout(self.feed_forward(self.norm3(x)))
        else:
            x = self.norm1(x + self.dropout(self.self_attn(x, tgt, tgt, q_mask)))
            x = self.norm2(x + self.dropout(self.src_attn(x, memory, memory, memory_mask)))
            x = self.norm3(x + self.dropout(self.feed_forward(x)))
        return torch.cat([cache, x], dim=1), tgt_mask, memory, memory_mask
