"""The attention decoder on this library's kernels, stated once for its four callers, which keep their tables, state, search
logic and results: attn_rescore.py (packed rows), attn_search.py, joint_search.py and attn_train.py (under autograd).

Here: what the kernels take (kernels_unmet for inference, att_loss_unmet for training); proj, every nn.Linear on the library's
GEMMs; stacked, the q | k | v and k | v weights of a layer as one tensor each; decoder_layers, the inference body, to which a
caller supplies a layer's self-attention (hip_ops.mha_rows causal, mha_step or mha_step_paths) and a CrossAttention;
pass_launches, what such a pass launches; SearchEngine, the set-up of the two search engines; decoder_rows_train, the stack under
autograd, whose ops differ (hip_ops.linear, layer_norm, residual_dropout, mha_rows_train, the feed-forward as a module)."""
import collections
import functools
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import hip_ops
from .._lib import PafcError
from .decoder import BiTransformerDecoder

KERNEL_ACTS = {"relu": "relu", "swish": "silu", "tanh": "tanh"}        # the epilogues the GEMMs fuse


def left_right(decoder):
    if isinstance(decoder, BiTransformerDecoder):
        return decoder.left_decoder, decoder.right_decoder
    return decoder, None


def _decoder_unmet(dec) -> Optional[str]:
    """The checks inference and training share, for one TransformerDecoder."""
    if any(not p.is_cuda for p in dec.parameters()):
        return "the decoder is not on the GPU"
    d = dec.after_norm.normalized_shape[0]
    if d != dec.attention_heads * 64:
        return f"attention heads of {d // dec.attention_heads if d % dec.attention_heads == 0 else d / dec.attention_heads} " \
               "dimensions (the attention kernel takes 64)"
    if dec.activation_type not in KERNEL_ACTS:
        return f"activation_type {dec.activation_type!r} (the GEMM epilogues have {sorted(KERNEL_ACTS)})"
    if not dec.use_output_layer:
        return "a decoder without output_layer"
    return None


def kernels_unmet(model, encoder_out: torch.Tensor, use_right: bool) -> Optional[str]:
    """What keeps the decoder's inference paths from running on the library's kernels, or None."""
    if not encoder_out.is_cuda:
        return "the operands are not on the GPU"
    left, right = left_right(model.decoder)
    for dec in [left] + ([right] if use_right else []):
        dts = {p.dtype for p in dec.parameters()}
        if len(dts) != 1 or next(iter(dts)) not in (torch.float32, torch.bfloat16):
            return "the decoder's parameters are not all float32 or all bfloat16"
        unmet = _decoder_unmet(dec)
        if unmet is not None:
            return unmet
    return None


def att_loss_unmet(decoders, x: torch.Tensor) -> Optional[str]:
    """What keeps the attention decoder's loss from running on packed rows over the library's kernels, or None.  decoders: the
    TransformerDecoder modules that will run (left, and right when reverse_weight > 0); x: the encoder output."""
    if not x.is_cuda:
        return "the operands are not on the GPU"
    if not torch.is_grad_enabled():
        return "gradients are disabled"
    if not hip_ops.train_kernels_enabled():
        return "PAFC_TRAIN_KERNELS=0"
    autocast_bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
    for dec in decoders:
        unmet = _decoder_unmet(dec)
        if unmet is not None:
            return unmet
        params = list(dec.parameters())
        bf16_model = x.dtype == torch.bfloat16 and all(p.dtype == torch.bfloat16 for p in params)
        if not (bf16_model or (autocast_bf16 and all(p.dtype in (torch.float32, torch.bfloat16) for p in params))):
            return "neither bf16 autocast nor a bf16 module"
        if any(l.self_attn.dropout.p != 0 or l.src_attn.dropout.p != 0 for l in dec.decoders):
            return "attention-probability dropout (self_attention_dropout_rate / src_attention_dropout_rate must be 0)"
    return None


def proj(x, weight, bias, act: str = "none", residual=None, *, who: str, split_ok: bool):
    """act(x weight^T + bias) [+ residual] on the library's GEMMs; PafcError, in the name of the entry point `who`, for operands
    none of them takes.  split_ok (no default: every call site passes the decoder's switch): long fp32 inputs may take the
    split-operand GEMM."""
    N, K = weight.shape
    if x.dtype == torch.float32:
        if act == "none" and residual is None:
            return hip_ops.linear_fused(x, weight, bias, "none", split_ok=split_ok)
        if act == "none" and split_ok and hip_ops.split_gemm_takes(x, weight, bias):
            # linear_fused's own rule for long fp32 inputs, with the residual add in the epilogue (the split-operand GEMM
            # fuses an fp32 residual, not an activation: the feed-forward's first projection stays on exact products)
            planes = hip_ops.split_planes(x if x.is_contiguous() else x.contiguous())
            return hip_ops.gemm_ph_ex(planes, hip_ops.split_weight_cached(weight), bias, residual=residual, a_split=True,
                                      out_kind="f32")
        if hip_ops.gemm_f32_ok(x, weight):
            return hip_ops.gemm_f32(x, weight, bias, act, residual=residual)
    elif K % 64 == 0 and N % 8 == 0:
        return hip_ops.gemm_bf16(x, weight, bias, act, residual=residual)
    elif act == "none" and residual is None and K % 4 == 0:
        return hip_ops.linear_bias_act(x, weight, bias, "none")
    raise PafcError(f"{who}(backend='kernels'): no GEMM of the library takes a ({N}, {K}) {x.dtype} projection "
                    f"with act {act!r}")


def decoder_proj(model, who: str):
    """proj for every projection of a call of `who`, under the decoder's one switch (fp32_split_operands)."""
    return functools.partial(proj, who=who, split_ok=bool(getattr(model.decoder, "fp32_split_operands", True)))


def cat_bias(lins) -> torch.Tensor:
    """The biases of stacked linears as one vector, zeros for a linear without one (key_bias: false)."""
    return torch.cat([l.bias if l.bias is not None else torch.zeros_like(l.weight[:, 0]) for l in lins])


def stacked(layer):
    """[linear_q; linear_k; linear_v] of the self-attention and [linear_k; linear_v] of the source attention as one weight and
    one bias each, cached on the layer for as long as the five weights are the tensors they were made from."""
    sa, ca = layer.self_attn, layer.src_attn
    lins = (sa.linear_q, sa.linear_k, sa.linear_v, ca.linear_k, ca.linear_v)
    stamp = tuple((l.weight.data_ptr(), l.weight._version, None if l.bias is None else l.bias._version) for l in lins) \
        + (hip_ops.param_epoch(),)
    ent = layer.__dict__.get("_pafc_stacked")
    if ent is None or ent[0] != stamp:
        ent = (stamp, torch.cat([l.weight for l in lins[:3]]).detach(), cat_bias(lins[:3]).detach(),
               torch.cat([l.weight for l in lins[3:]]).detach(), cat_bias(lins[3:]).detach(),
               hip_ops.DerivedFill(sa.linear_q.weight.device))
        layer.__dict__["_pafc_stacked"] = ent
    else:
        ent[5].use(sa.linear_q.weight.device)
    return ent[1:5]


def upload_tables(fields: Sequence, device) -> List[torch.Tensor]:
    """The integer tables of one call as ONE int32 tensor and one upload; per field its view."""
    packed = torch.from_numpy(np.concatenate([np.asarray(f, dtype=np.int32) for f in fields])).to(device, non_blocking=True)
    ends = np.cumsum([len(f) for f in fields]).tolist()
    return [packed[e - len(f):e] for f, e in zip(fields, ends)]


def position_table(dec, positions: int, device, dtype) -> torch.Tensor:
    """(positions, d): the decoder's position encoding of the positions [0, positions)."""
    return dec.embed[1].position_encoding(0, positions, False, device=device)[0].to(dtype)


def embed_rows(dec, pe: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """The decoder's input rows (before the positional dropout): tok / pos (rows) int32, pe from position_table."""
    return torch.embedding(dec.embed[0].weight, tok) * dec.embed[1].xscale + pe.index_select(0, pos)


# The source attention of a pass: the rows [q_off[g], q_off[g + 1]) attend to the kv_len[g] memory rows from kv_off[g].  Either
# mem_kv, per layer the memory's K | V made before the pass (the searches), or memory, which each layer projects (rescoring).
CrossAttention = collections.namedtuple("CrossAttention", "q_off kv_off kv_len memory mem_kv", defaults=(None, None))


_ln = lambda t, n: hip_ops.add_layernorm(t, None, 0.0, n.weight, n.bias, eps=n.eps)[1]                        # noqa: E731
_add_ln = lambda t, y, n: hip_ops.add_layernorm(t, y, 1.0, n.weight, n.bias, eps=n.eps, want_x=False)[1]      # noqa: E731


def decoder_layers(dec, x, self_attention, cross: CrossAttention, proj):
    """The decoder stack on the library's kernels: x (rows, d) from embed_rows -> (rows, d), the input of output_layer.
    self_attention(i, layer, qkv) -> (rows, d) is layer i's self-attention over its stacked q | k | v projection; proj from
    decoder_proj.  stacked(layer) is looked up at every call: that is where a side stream waits for the fill."""
    d, H = x.size(1), dec.attention_heads
    act = KERNEL_ACTS[dec.activation_type]
    for i, layer in enumerate(dec.decoders):
        w_qkv, b_qkv, w_kv, b_kv = stacked(layer)
        sa, ca, ff = layer.self_attn, layer.src_attn, layer.feed_forward
        pre = layer.normalize_before
        att = self_attention(i, layer, proj(_ln(x, layer.norm1) if pre else x, w_qkv, b_qkv))
        if pre:
            x = proj(att, sa.linear_out.weight, sa.linear_out.bias, residual=x)
        else:
            x = _add_ln(x, proj(att, sa.linear_out.weight, sa.linear_out.bias), layer.norm1)
        q = proj(_ln(x, layer.norm2) if pre else x, ca.linear_q.weight, ca.linear_q.bias)
        kv = cross.mem_kv[i] if cross.mem_kv is not None else proj(cross.memory, w_kv, b_kv)
        att = hip_ops.mha_rows(q, kv[:, :d], kv[:, d:], cross.q_off, cross.kv_off, cross.kv_len, H, False)
        if pre:
            x = proj(att, ca.linear_out.weight, ca.linear_out.bias, residual=x)
        else:
            x = _add_ln(x, proj(att, ca.linear_out.weight, ca.linear_out.bias), layer.norm2)
        h = proj(_ln(x, layer.norm3) if pre else x, ff.w_1.weight, ff.w_1.bias, act=act)
        if pre:
            x = proj(h, ff.w_2.weight, ff.w_2.bias, residual=x)
        else:
            x = _add_ln(x, proj(h, ff.w_2.weight, ff.w_2.bias), layer.norm3)
    return _ln(x, dec.after_norm) if dec.normalize_before else x


def pass_launches(dec) -> int:
    """The launches of embed_rows + decoder_layers on a mem_kv: per layer three LayerNorms, six projections, two attentions."""
    return 4 + 11 * len(dec.decoders) + (1 if dec.normalize_before else 0)


class SearchEngine:
    """What the two search engines set up of the decoder before their loop and run in it.  A subclass supplies
    self_attention(i, layer, qkv) over its own caches and checks cache_bytes_of against its own cap."""
    ops = hip_ops

    def bind_decoder(self, model, who: str) -> None:
        self.dec, _ = left_right(model.decoder)
        self.H, self.dtype = self.dec.attention_heads, self.dec.after_norm.weight.dtype
        self.proj = decoder_proj(model, who)

    def cache_bytes_of(self, rows: int, d: int) -> int:               # per layer `rows` rows of k | v
        return len(self.dec.decoders) * rows * 2 * d * torch.empty(0, dtype=self.dtype).element_size()

    def project_memory(self, encoder_out: torch.Tensor, kv_len: torch.Tensor, N: int, positions: int) -> None:
        """The source attention's K | V, for the N rows of every utterance and all steps: each layer projects the memory once.
        The padded rows are projected too and never read (kv_len): the utterances' lengths stay on the device."""
        B, T, d = encoder_out.shape
        dev = encoder_out.device
        memory = encoder_out.to(self.dtype).reshape(B * T, d)
        mem_kv = [self.proj(memory, *stacked(layer)[2:]) for layer in self.dec.decoders]
        self.cross = CrossAttention(torch.arange(0, B * N + 1, N, dtype=torch.int32, device=dev),
                                    torch.arange(0, B * T, T, dtype=torch.int32, device=dev), kv_len, mem_kv=mem_kv)
        self.pe = position_table(self.dec, positions, dev, self.dtype)

    def decoder_pass(self, tok: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
        """tok / pos (rows) int32 -> the rows' input of output_layer; pass_launches(self.dec) launches."""
        return decoder_layers(self.dec, embed_rows(self.dec, self.pe, tok, pos), self.self_attention, self.cross, self.proj)


def decoder_rows_train(dec, tok, pos, max_rows, memory, q_off, self_len, mem_off, mem_len):
    """The decoder stack over packed rows under autograd: tok / pos (rows) int32 -> (rows, d), the input of output_layer.  The
    stacked weights are a torch.cat of the parameters at every call (not `stacked`), so autograd reaches each of them."""
    d, H = memory.size(1), dec.attention_heads
    training = dec.training
    pe = position_table(dec, max_rows, memory.device, dec.embed[0].weight.dtype)
    x = dec.embed[1].dropout(embed_rows(dec, pe, tok, pos))
    ln = lambda t, n: hip_ops.layer_norm(t, n.weight, n.bias, n.eps, bf16_out=True)                         # noqa: E731
    ln_sum = lambda t, n: hip_ops.layer_norm(t, n.weight, n.bias, n.eps)        # post-norm: the residual stream keeps its dtype  # noqa: E731
    for layer in dec.decoders:
        sa, ca = layer.self_attn, layer.src_attn
        pre, p = layer.normalize_before, layer.dropout.p
        lins = (sa.linear_q, sa.linear_k, sa.linear_v)
        qkv = hip_ops.linear(ln(x, layer.norm1) if pre else x, torch.cat([l.weight for l in lins]), cat_bias(lins))
        att = hip_ops.mha_rows_train(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], q_off, q_off[:-1], self_len, H, True)
        x = hip_ops.residual_dropout(x, hip_ops.linear(att, sa.linear_out.weight, sa.linear_out.bias), 1.0, p, training)
        if not pre:
            x = ln_sum(x, layer.norm1)
        q = hip_ops.linear(ln(x, layer.norm2) if pre else x, ca.linear_q.weight, ca.linear_q.bias)
        lins = (ca.linear_k, ca.linear_v)
        kv = hip_ops.linear(memory, torch.cat([l.weight for l in lins]), cat_bias(lins))
        if q.dtype != kv.dtype:
            kv = kv.to(q.dtype)
        att = hip_ops.mha_rows_train(q, kv[:, :d], kv[:, d:], q_off, mem_off, mem_len, H, False)
        x = hip_ops.residual_dropout(x, hip_ops.linear(att, ca.linear_out.weight, ca.linear_out.bias), 1.0, p, training)
        if not pre:
            x = ln_sum(x, layer.norm2)
        x = hip_ops.residual_dropout(x, layer.feed_forward(ln(x, layer.norm3) if pre else x), 1.0, p, training)
        if not pre:
            x = ln_sum(x, layer.norm3)
    return ln(x, dec.after_norm) if dec.normalize_before else x
