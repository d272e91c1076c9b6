"""Token helpers of the attention loss (reference semantics: wenet/utils/common.py add_sos_eos, reverse_pad_list,
th_accuracy).  Transcripts arrive as (B, Lmax) id tensors padded with IGNORE_ID."""
from typing import Tuple

import torch

IGNORE_ID = -1


def _pad_rows(rows, pad_value: int, like: torch.Tensor) -> torch.Tensor:
    width = max((len(r) for r in rows), default=0)
    out = torch.full((len(rows), width), pad_value, dtype=rows[0].dtype if rows else like.dtype, device=like.device)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def add_sos_eos(ys_pad: torch.Tensor, sos: int, eos: int, ignore_id: int = IGNORE_ID) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ys_in, ys_out) of a padded batch: per utterance the ids that are not ignore_id, with sos in front (ys_in, padded with
    eos) and with eos behind (ys_out, padded with ignore_id); both (B, Lmax' + 1) int64, Lmax' the longest kept transcript."""
    ys = [y[y != ignore_id].to(torch.int64) for y in ys_pad]
    s = torch.tensor([sos], dtype=torch.int64, device=ys_pad.device)
    e = torch.tensor([eos], dtype=torch.int64, device=ys_pad.device)
    return (_pad_rows([torch.cat([s, y]) for y in ys], eos, ys_pad),
            _pad_rows([torch.cat([y, e]) for y in ys], ignore_id, ys_pad))


def reverse_pad_list(ys_pad: torch.Tensor, ys_lens: torch.Tensor, pad_value: float = -1.0) -> torch.Tensor:
    """Every transcript reversed over its own length, padded with pad_value: (B, max(ys_lens)) int32 (the reference casts the
    ids to int32 here)."""
    rows = [y.to(torch.int32)[:int(n)].flip(0) for y, n in zip(ys_pad, ys_lens)]
    return _pad_rows(rows, int(pad_value), ys_pad.to(torch.int32))


def th_accuracy(pad_outputs: torch.Tensor, pad_targets: torch.Tensor, ignore_label: int = IGNORE_ID) -> torch.Tensor:
    """Share of the targets that are not ignore_label whose row of pad_outputs (B * Lmax, V) has its argmax there (NaN when
    nothing is scored, as 0 / 0 is)."""
    B, L = pad_targets.shape
    pred = pad_outputs.view(B, L, pad_outputs.size(1)).argmax(2)
    scored = pad_targets != ignore_label
    return (((pred == pad_targets) & scored).sum() / scored.sum()).detach()
