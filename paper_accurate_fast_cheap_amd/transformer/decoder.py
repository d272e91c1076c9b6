"""Attention decoders of the second pass: TransformerDecoder and BiTransformerDecoder (the published WeNet decoders,
wenet/transformer/decoder.py, which the reference's release omits while every YAML it ships asks for `decoder:
bitransformer`).  Parameter names and constructor keys are upstream's, so reference checkpoints load:
  [left_decoder. | right_decoder.] embed.0.weight, decoders.N.{self_attn,src_attn}.linear_{q,k,v,out}.*,
  decoders.N.feed_forward.w_{1,2}.*, decoders.N.norm{1,2,3}.*, after_norm.*, output_layer.*
These modules are the definition and the "framework" backend of ASRModel.score_attention; on the GPU the second pass runs
the same weights over packed rows through the library's kernels (transformer/attn_rescore.py)."""
from typing import List, Optional, Tuple

import torch

from ..utils.mask import make_pad_mask
from .attention import MultiHeadedAttention
from .decoder_layer import DecoderLayer
from .embedding import PositionalEncoding
from .positionwise_feed_forward import PositionwiseFeedForward

ACTIVATIONS = {"hardtanh": torch.nn.Hardtanh, "tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "selu": torch.nn.SELU,
               "swish": torch.nn.SiLU, "gelu": torch.nn.GELU}


def subsequent_mask(size: int, device=None) -> torch.Tensor:
    """(size, size) bool, True where column <= row (wenet/utils/mask.py:23-55)."""
    return torch.ones(size, size, dtype=torch.bool, device=device).tril()


class TransformerDecoder(torch.nn.Module):
    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4, linear_units: int = 2048,
                 num_blocks: int = 6, dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1,
                 self_attention_dropout_rate: float = 0.0, src_attention_dropout_rate: float = 0.0,
                 input_layer: str = "embed", use_output_layer: bool = True, normalize_before: bool = True,
                 key_bias: bool = True, activation_type: str = "relu", **_unused_decoder_conf):
        super().__init__()
        if input_layer != "embed":
            raise ValueError(f"only 'embed' input_layer is supported: {input_layer}")
        d = encoder_output_size
        self.vocab_size = vocab_size
        self.attention_heads = attention_heads
        self.activation_type = activation_type
        self.embed = torch.nn.Sequential(torch.nn.Embedding(vocab_size, d), PositionalEncoding(d, positional_dropout_rate))
        self.normalize_before = normalize_before
        self.after_norm = torch.nn.LayerNorm(d, eps=1e-5)
        self.use_output_layer = use_output_layer
        self.output_layer = torch.nn.Linear(d, vocab_size) if use_output_layer else torch.nn.Identity()
        self.num_blocks = num_blocks
        self.decoders = torch.nn.ModuleList([
            DecoderLayer(d, MultiHeadedAttention(attention_heads, d, self_attention_dropout_rate, key_bias),
                         MultiHeadedAttention(attention_heads, d, src_attention_dropout_rate, key_bias),
                         PositionwiseFeedForward(d, linear_units, dropout_rate, ACTIVATIONS[activation_type]()),
                         dropout_rate, normalize_before) for _ in range(num_blocks)])

    def forward(self, memory: torch.Tensor, memory_mask: torch.Tensor, ys_in_pad: torch.Tensor, ys_in_lens: torch.Tensor,
                r_ys_in_pad: Optional[torch.Tensor] = None, reverse_weight: float = 0.0
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """memory (B, S, D), memory_mask (B, 1, S), ys_in_pad (B, L) token ids, ys_in_lens (B) -> (logits (B, L, V),
        tensor(0.0), olens (B, L): the visible keys per query)."""
        L = ys_in_pad.size(1)
        tgt_mask = ~make_pad_mask(ys_in_lens, L)[:, None, :] & subsequent_mask(L, ys_in_pad.device)[None]
        x, _ = self.embed(ys_in_pad)
        for layer in self.decoders:
            x, tgt_mask, memory, memory_mask = layer(x, tgt_mask, memory, memory_mask)
        if self.normalize_before:
            x = self.after_norm(x)
        if self.use_output_layer:
            x = self.output_layer(x)
        return x, torch.tensor(0.0), tgt_mask.sum(1)

    def forward_one_step(self, memory: torch.Tensor, memory_mask: torch.Tensor, tgt: torch.Tensor, tgt_mask: torch.Tensor,
                         cache: Optional[List[torch.Tensor]] = None) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """One step of autoregressive decoding (upstream's method, which search.py:304 of the reference calls): tgt (B, L)
        the prefixes, tgt_mask (B, L, L), cache the per-layer outputs (B, L - 1, D) of the previous step or None ->
        (log p(next token | prefix) (B, V), the per-layer outputs (B, L, D)).  With a cache a layer computes its last row
        only."""
        x, _ = self.embed(tgt)
        new_cache = []
        for i, layer in enumerate(self.decoders):
            x, tgt_mask, memory, memory_mask = layer(x, tgt_mask, memory, memory_mask, cache=None if cache is None else cache[i])
            new_cache.append(x)
        y = self.after_norm(x[:, -1]) if self.normalize_before else x[:, -1]
        if self.use_output_layer:
            y = torch.log_softmax(self.output_layer(y), dim=-1)
        return y, new_cache


class BiTransformerDecoder(torch.nn.Module):
    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4, linear_units: int = 2048,
                 num_blocks: int = 6, r_num_blocks: int = 0, **decoder_conf):
        super().__init__()
        self.left_decoder = TransformerDecoder(vocab_size, encoder_output_size, attention_heads, linear_units, num_blocks,
                                               **decoder_conf)
        self.right_decoder = TransformerDecoder(vocab_size, encoder_output_size, attention_heads, linear_units, r_num_blocks,
                                                **decoder_conf)

    def forward(self, memory: torch.Tensor, memory_mask: torch.Tensor, ys_in_pad: torch.Tensor, ys_in_lens: torch.Tensor,
                r_ys_in_pad: Optional[torch.Tensor] = None, reverse_weight: float = 0.0
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        l_x, _, olens = self.left_decoder(memory, memory_mask, ys_in_pad, ys_in_lens)
        r_x = torch.tensor(0.0)
        if reverse_weight > 0.0:
            r_x, _, olens = self.right_decoder(memory, memory_mask, r_ys_in_pad, ys_in_lens)
        return l_x, r_x, olens

    def forward_one_step(self, memory: torch.Tensor, memory_mask: torch.Tensor, tgt: torch.Tensor, tgt_mask: torch.Tensor,
                         cache: Optional[List[torch.Tensor]] = None) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """The left decoder's step: hypotheses grow left to right."""
        return self.left_decoder.forward_one_step(memory, memory_mask, tgt, tgt_mask, cache)


DECODER_CLASSES = {"transformer": TransformerDecoder, "bitransformer": BiTransformerDecoder}
