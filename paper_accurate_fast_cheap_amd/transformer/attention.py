"""MultiHeadedAttention of the attention decoder (reference: wenet/transformer/attention.py:28-200): scaled dot-product
attention, parameters linear_q / linear_k / linear_v / linear_out.  Masked keys get -inf before the softmax and 0 after it
(:112-118), so a query without a visible key yields zeros.  This module is the definition and the "framework" backend; the
second pass on the GPU packs the rows and runs hip_ops.mha_rows instead (transformer/attn_rescore.py).

LimitedRelPositionMultiHeadedAttention is the encoder slot of the Conformer baseline (reference: attention.py:406-645,
`selfattention_layer_type: limited_rel_selfattn`): self-attention over a band of +-w frames with the key's position row as a
second score term, on hip_ops.mha_band and this package's GEMMs.  Inference on the GPU; with `trainable` set (ConformerEncoder
sets it on the slots it builds) also training, through hip_ops.mha_band_train."""
import math
from typing import Optional, Tuple

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


class LimitedRelPositionMultiHeadedAttention(torch.nn.Module):
    """Limited-context attention with positional encoding, global_tokens = 0.  With w = att_context_size[0] =
    att_context_size[1] and T_pad = T rounded up to a multiple of 2 w, query i sees the keys j with |j - i| <= w, 0 <= j < T_pad:
        s_ij = ((q_i + pos_bias_u) . k_j + (q_i + pos_bias_v) . p_j) / sqrt(d_k),   p = linear_pos(pos_emb)   for j < T,
    p_j being the KEY's position row (no relative shift).  The keys of [T, T_pad) are the zero padding of the reference's
    blocked layout and are not masked (score 0, value 0), and `mask` does not reach the output (attention.py:552 is commented
    out): padded frames of a batch row are keys like any other.  Trained checkpoints have seen both, so both are kept.
    Parameter names are the reference's: a checkpoint loads with strict=True."""

    # with gradients enabled: run the training path (hip_ops.mha_band_train, differentiable projections) instead of refusing.
    # Set by an encoder that builds the slot (ConformerEncoder, next to own_gemm); a bare module keeps the inference-only error.
    trainable: bool = False

    def __init__(self, n_head: int, n_feat: int, dropout_rate: float, key_bias: bool = True, att_context_size=(500, 500),
                 global_tokens: int = 0, global_tokens_spacing: int = 1, global_attn_separate: bool = False, layer_id: int = 0):
        super().__init__()
        assert n_feat % n_head == 0
        ctx = tuple(int(c) for c in att_context_size)
        if len(ctx) != 2 or ctx[0] != ctx[1]:
            raise ValueError(f"att_context_size={list(att_context_size)}: the two sides must be equal (the reference fails on a "
                             f"shape mismatch otherwise, attention.py:529)")
        if ctx[0] < 2:
            raise ValueError(f"att_context_size={list(att_context_size)}: the context must be at least 2 (the reference's blocked "
                             f"layout fails for 1, attention.py:1009, and refuses 0)")
        if global_tokens > 0 or global_attn_separate:
            raise NotImplementedError(
                f"global_tokens={global_tokens}, global_attn_separate={global_attn_separate}: global attention tokens (conf/"
                f"conformer/giga.conformer_ds4k31nc_12le.trans.FT-LF-LA256-GT.yaml) are not implemented; global_tokens: 0 is")
        self.d_k = n_feat // n_head
        self.h = n_head
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat, bias=key_bias)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)
        self.dropout = torch.nn.Dropout(p=dropout_rate)
        self.linear_pos = torch.nn.Linear(n_feat, n_feat, bias=False)
        self.pos_bias_u = torch.nn.Parameter(torch.empty(self.h, self.d_k))
        self.pos_bias_v = torch.nn.Parameter(torch.empty(self.h, self.d_k))
        torch.nn.init.xavier_uniform_(self.pos_bias_u)
        torch.nn.init.xavier_uniform_(self.pos_bias_v)
        self.att_context_size = list(ctx)
        self.global_tokens = global_tokens
        self.global_tokens_spacing = global_tokens_spacing
        self.global_attn_separate = global_attn_separate
        self.layer_id = layer_id
        self._qkv = None           # (stamp, stacked [Wq; Wk; Wv], stacked bias, fill): rebuilt when a parameter changes

    def __getstate__(self):        # the stacked copy is derived: never copied or pickled with the module
        st = self.__dict__.copy()
        st["_qkv"] = None
        return st

    def _stacked_qkv(self):
        from .. import hip_ops
        ps = [self.linear_q.weight, self.linear_k.weight, self.linear_v.weight, self.linear_q.bias, self.linear_k.bias,
              self.linear_v.bias]
        stamp = (hip_ops.param_epoch(),) + tuple((p.data_ptr(), p._version, p.dtype) for p in ps if p is not None)
        if self._qkv is None or self._qkv[0] != stamp:
            with torch.no_grad():
                w = torch.cat([p.detach() for p in ps[:3]]).contiguous()
                kb = ps[4].detach() if ps[4] is not None else torch.zeros_like(ps[3])
                b = torch.cat([ps[3].detach(), kb, ps[5].detach()]).contiguous()
            self._qkv = (stamp, w, b, hip_ops.DerivedFill(w.device))
        else:
            self._qkv[3].use(self._qkv[1].device)
        return self._qkv[1], self._qkv[2]

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                mask: torch.Tensor = torch.ones((0, 0, 0), dtype=torch.bool), pos_emb: torch.Tensor = torch.empty(0),
                cache: torch.Tensor = torch.zeros((0, 0, 0, 0))) -> Tuple[torch.Tensor, torch.Tensor]:
        """query / key / value (B, T, D), pos_emb (1, T, D): the position rows of the T frames -> (out (B, T, D), new_cache
        (B, H, T, 2 d_k) = cat(k, v)).  `mask` is accepted and, as in the reference, not applied."""
        from .. import hip_ops
        if cache.numel() > 0:
            raise ValueError("cache: limited-context attention takes no key/value cache (the reference asserts q.size() == "
                             "k.size(), so it fails for a non-empty one too); pass the empty cache")
        train = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or (
            self.trainable and (query.requires_grad or key.requires_grad or value.requires_grad)))   # (frozen slot, live input)
        if train and not self.trainable:
            raise NotImplementedError("limited_rel_selfattn is inference only: call it under torch.no_grad() (a module built "
                                      "outside ConformerEncoder trains only with its `trainable` attribute set)")
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("limited_rel_selfattn: attention dropout is a training feature; call .eval() first")
        if self.d_k != 64:
            raise NotImplementedError(f"limited_rel_selfattn: head size {self.d_k}; the attention kernel takes 64")
        hip_ops._lib.require_gpu(query, key, value, pos_emb)
        B, T, D = query.shape
        if key.shape != query.shape or value.shape != query.shape:
            raise ValueError("key / value: self-attention takes key and value of the query's shape")
        if pos_emb.dim() != 3 or pos_emb.size(0) != 1 or pos_emb.size(1) != T or pos_emb.size(2) != D:
            raise ValueError(f"pos_emb: expected the (1, {T}, {D}) position rows of the input's frames, got {tuple(pos_emb.shape)}")
        if train:
            return self._forward_train(query, key, value, pos_emb)
        lin = lambda x, w, b: hip_ops.linear_fused(x, w, b, "none", split_ok=False)       # exact fp32 products in an fp32 model
        if key is query and value is query:
            w_qkv, b_qkv = self._stacked_qkv()
            qkv = lin(query.reshape(B * T, D), w_qkv, b_qkv)                             # (B T, 3 D): one product
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        else:
            q = lin(query.reshape(B * T, D), self.linear_q.weight, self.linear_q.bias)
            kv = torch.empty(B * T, 2 * D, dtype=q.dtype, device=q.device)               # k and v share a row pitch
            kv[:, :D] = lin(key.reshape(B * T, D), self.linear_k.weight, self.linear_k.bias)
            kv[:, D:] = lin(value.reshape(B * T, D), self.linear_v.weight, self.linear_v.bias)
            k, v = kv[:, :D], kv[:, D:]
        p = lin(pos_emb.reshape(T, D).to(q.dtype), self.linear_pos.weight, None)
        att = hip_ops.mha_band(q, k, v, p, self.pos_bias_u, self.pos_bias_v, B, self.h, self.att_context_size[0])
        new_cache = torch.cat((k.view(B, T, self.h, self.d_k).transpose(1, 2), v.view(B, T, self.h, self.d_k).transpose(1, 2)),
                              dim=-1)
        out = lin(att, self.linear_out.weight, self.linear_out.bias)
        return out.view(B, T, D), new_cache

    def _forward_train(self, query, key, value, pos_emb):
        """The same computation under autograd: the projections through hip_ops.linear_own (this package's GEMMs forward and
        backward; under bf16 autocast hip_ops.linear's bf16 training GEMMs), the attention through hip_ops.mha_band_train.
        The stacked [Wq; Wk; Wv] of the inference path is a detached copy, so the self-attention case stacks the three
        weights with a differentiable cat instead: still one product.  (mha_band_train writes dq | dk | dv into one (B T, 3 D)
        buffer; q, k, v reach it as three slice views, so autograd still adds three zero-padded thirds in front of the GEMM's
        backward, as it does for mha_rows_train.)"""
        from .. import hip_ops
        B, T, D = query.shape
        lin = hip_ops.linear_own
        if key is query and value is query:
            w_qkv = torch.cat((self.linear_q.weight, self.linear_k.weight, self.linear_v.weight))
            kb = self.linear_k.bias if self.linear_k.bias is not None else torch.zeros_like(self.linear_q.bias)
            b_qkv = torch.cat((self.linear_q.bias, kb, self.linear_v.bias))
            qkv = lin(query.reshape(B * T, D), w_qkv, b_qkv)
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        else:
            q = lin(query.reshape(B * T, D), self.linear_q.weight, self.linear_q.bias)
            kv = torch.cat((lin(key.reshape(B * T, D), self.linear_k.weight, self.linear_k.bias),
                            lin(value.reshape(B * T, D), self.linear_v.weight, self.linear_v.bias)), dim=1)
            k, v = kv[:, :D], kv[:, D:]                                                   # k and v share a row pitch
        p = lin(pos_emb.reshape(T, D).to(query.dtype), self.linear_pos.weight, None)
        if p.dtype != q.dtype:                                                           # (a short T under autocast: F.linear's dtype)
            p = p.to(q.dtype)
        att = hip_ops.mha_band_train(q, k, v, p, self.pos_bias_u, self.pos_bias_v, B, self.h, self.att_context_size[0])
        new_cache = torch.cat((k.view(B, T, self.h, self.d_k).transpose(1, 2), v.view(B, T, self.h, self.d_k).transpose(1, 2)),
                              dim=-1)
        out = lin(att, self.linear_out.weight, self.linear_out.bias)
        return out.view(B, T, D), new_cache
