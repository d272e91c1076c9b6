"""The attention term of the training objective (reference: ASRModel._calc_att_loss, wenet/transformer/asr_model.py:251-292):
    loss_att = (1 - reverse_weight) * lsm(left decoder, [sos] + y -> y + [eos])
             + reverse_weight * lsm(right decoder, [sos] + reversed y -> reversed y + [eos])
with the label-smoothing loss of transformer/label_smoothing_loss.py (divided by the batch size, or by the number of scored
tokens with length_normalized_loss) and the accuracy of the left decoder's argmax.

backend "framework" runs the padded modules as the reference does: add_sos_eos, masks, the (B, L + 1, V) logits,
LabelSmoothingLoss, th_accuracy -- on the CPU and the GPU.

backend "kernels" runs packed rows under autograd, the layout of the second pass (transformer/attn_rescore.py): utterance b
owns L_b + 1 rows ([sos] + y), no padding and no masks.  The memory stays where the encoder left it (kv_off = b * T', kv_len
the device-side encoder lengths): nothing is copied or repeated.  The stack is decoder_rows.decoder_rows_train, next to the
inference body it mirrors, and decoder_rows.att_loss_unmet says what it takes.  Projections run through hip_ops.linear (stacked
q | k | v and k | v weights as a torch.cat of the parameters, so autograd reaches each of them), LayerNorm through layer_norm,
both attentions through hip_ops.mha_rows_train (pafc_mha_rows_lse / pafc_mha_rows_bwd), the residual dropouts through
hip_ops.residual_dropout, and output_layer + loss + accuracy through hip_ops.att_head_loss: the (rows, V) log-softmax is never
formed.  The row tables come from the transcript lengths on the host -- the batch holds them there -- in one upload; with
lengths that live on the device they cost one read of it."""
from typing import Optional, Tuple

import numpy as np
import torch

from ..utils.common import IGNORE_ID, add_sos_eos, reverse_pad_list, th_accuracy
from . import decoder_rows
from .decoder_rows import decoder_rows_train, left_right, upload_tables
from .label_smoothing_loss import LabelSmoothingLoss

BACKENDS = ("framework", "kernels")


def trainable_decoder(model) -> bool:
    """The model has an attention decoder with at least one trainable parameter."""
    dec = getattr(model, "decoder", None)
    return dec is not None and any(p.requires_grad for p in dec.parameters())


def _decoders(model, reverse_weight: float):
    left, right = left_right(model.decoder)
    if reverse_weight > 0 and right is None:
        raise ValueError(f"reverse_weight = {reverse_weight} needs the right_decoder of a bitransformer decoder")
    return [left] + ([right] if reverse_weight > 0 else [])


def att_loss_unmet(model, encoder_out: torch.Tensor) -> Optional[str]:
    """What keeps att_loss(backend='kernels') from running for this model and input, or None (decoder_rows.att_loss_unmet)."""
    return decoder_rows.att_loss_unmet(_decoders(model, float(getattr(model, "reverse_weight", 0.0))), encoder_out)


def att_loss(model, encoder_out: torch.Tensor, encoder_mask: torch.Tensor, text: torch.Tensor, text_lengths: torch.Tensor,
             backend: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss_att, acc_att) for encoder_out (B, T', D), encoder_mask (B, 1, T') bool, text (B, Lmax) padded with IGNORE_ID and
    text_lengths (B), on the host or the device.  The model supplies decoder, sos, eos, vocab_size and (default 0 / 0 / False)
    reverse_weight, lsm_weight and length_normalized_loss.
    backend None: "kernels" when att_loss_unmet is None, else "framework"; "kernels" asked for by name is never a fallback
    (PafcError naming what is unmet)."""
    if getattr(model, "decoder", None) is None:
        raise NotImplementedError("att_loss: the model has no attention decoder")
    if backend is not None and backend not in BACKENDS:
        raise ValueError(f"backend {backend!r}: one of {BACKENDS} or None")
    if backend != "framework":
        unmet = att_loss_unmet(model, encoder_out)
        if backend == "kernels" and unmet is not None:
            from .._lib import PafcError
            raise PafcError(f"att_loss(backend='kernels'): {unmet}")
        backend = "kernels" if unmet is None else "framework"
    if backend == "framework":
        return _att_loss_framework(model, encoder_out, encoder_mask, text, text_lengths)
    return _att_loss_kernels(model, encoder_out, encoder_mask, text, text_lengths)


def _att_loss_framework(model, encoder_out, encoder_mask, text, text_lengths):
    rw = float(getattr(model, "reverse_weight", 0.0))
    _decoders(model, rw)
    dev = encoder_out.device
    text, text_lengths = text.to(dev), text_lengths.to(dev)
    crit = LabelSmoothingLoss(model.vocab_size, IGNORE_ID, float(getattr(model, "lsm_weight", 0.0)),
                              bool(getattr(model, "length_normalized_loss", False)))
    ys_in, ys_out = add_sos_eos(text, model.sos, model.eos, IGNORE_ID)
    r_text = reverse_pad_list(text, text_lengths, float(IGNORE_ID))
    r_ys_in, r_ys_out = add_sos_eos(r_text, model.sos, model.eos, IGNORE_ID)
    l_x, r_x, _ = model.decoder(encoder_out, encoder_mask, ys_in, text_lengths + 1, r_ys_in, rw)
    loss = crit(l_x, ys_out)
    if rw > 0:
        loss = loss * (1 - rw) + crit(r_x, r_ys_out) * rw
    return loss, th_accuracy(l_x.reshape(-1, model.vocab_size), ys_out, IGNORE_ID)


def _tables(lens, Lmax: int, T: int, length_normalized: bool):
    """The int32 table of one call, from the transcript lengths alone: per row its position and the flat indices into text of
    its input and target token for both directions (-1: sos / eos), then q_off, the rows per utterance, the memory offsets and
    the loss' denominator."""
    B = len(lens)
    rows = lens + 1
    q_off = np.concatenate([[0], np.cumsum(rows)])
    R = int(q_off[-1])
    b_of = np.repeat(np.arange(B), rows)
    pos = np.arange(R) - q_off[:-1][b_of]
    L = lens[b_of]
    base = b_of * Lmax
    l_in = np.where(pos > 0, base + pos - 1, -1)
    l_out = np.where(pos < L, base + pos, -1)
    r_in = np.where(pos > 0, base + L - pos, -1)
    r_out = np.where(pos < L, base + L - 1 - pos, -1)
    fields = [pos, l_in, l_out, r_in, r_out, q_off, rows, np.arange(B) * T, [R if length_normalized else B]]
    return R, fields


def _att_loss_kernels(model, encoder_out, encoder_mask, text, text_lengths):
    from .. import hip_ops
    from .._lib import PafcError
    rw = float(getattr(model, "reverse_weight", 0.0))
    decs = _decoders(model, rw)
    dev = encoder_out.device
    B, T, D = encoder_out.shape
    lens = np.asarray(text_lengths.tolist(), dtype=np.int64)            # on the host already when the batch holds them there
    if len(lens) != B or text.size(0) != B or (lens < 0).any() or (B and int(lens.max()) > text.size(1)):
        raise PafcError(f"att_loss: {B} utterances, text {tuple(text.shape)}, lengths {lens.tolist()}")
    Lmax = max(1, text.size(1))
    R, fields = _tables(lens, Lmax, T, bool(getattr(model, "length_normalized_loss", False)))
    pos, l_in, l_out, r_in, r_out, q_off, self_len, mem_off, denom_i = upload_tables(fields, dev)
    denom = denom_i.to(torch.float32)
    flat = text.to(dev).reshape(-1).to(torch.int32)
    if flat.numel() == 0:
        flat = flat.new_zeros(1)
    pick = lambda idx, fill: torch.where(idx < 0, torch.full_like(idx, fill), flat[idx.clamp_min(0).long()])     # noqa: E731
    mem_len = encoder_mask.reshape(B, -1).sum(1).to(torch.int32)
    memory = encoder_out.reshape(B * T, D)
    smoothing = float(getattr(model, "lsm_weight", 0.0))
    loss, acc = None, None
    for i, dec in enumerate(decs):
        tok = pick(l_in if i == 0 else r_in, model.sos)
        tgt = pick(l_out if i == 0 else r_out, model.eos)
        x = decoder_rows_train(dec, tok, pos, int(lens.max()) + 1, memory, q_off, self_len, mem_off, mem_len)
        term, n_correct = hip_ops.att_head_loss(x, dec.output_layer.weight, dec.output_layer.bias, tgt, smoothing, denom)
        if i == 0:
            loss = term * (1 - rw) if rw > 0 else term
            acc = (n_correct / float(R)).detach()
        else:
            loss = loss + term * rw
    return loss, acc
