"""Label-smoothing loss of the attention decoder (reference: wenet/transformer/label_smoothing_loss.py): the KL divergence
between the smoothed one-hot target -- 1 - smoothing on the label, smoothing / (size - 1) on every other class -- and the
model's softmax, summed over the rows whose target is not padding_idx and divided by the batch size or, with
normalize_length, by the number of such rows.  Framework ops: this module is the definition; on the GPU the training step
computes the same number from the logits with pafc_lsm_loss_rows (hip_ops.att_head_loss)."""
import torch


class LabelSmoothingLoss(torch.nn.Module):
    def __init__(self, size: int, padding_idx: int, smoothing: float, normalize_length: bool = False):
        super().__init__()
        self.size = size
        self.padding_idx = padding_idx
        self.smoothing = smoothing
        self.confidence = 1.0 - smoothing
        self.normalize_length = normalize_length

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """x (B, L, size) logits, target (B, L) ids with padding_idx where nothing is scored -> scalar."""
        assert x.size(2) == self.size
        batch = x.size(0)
        x = x.reshape(-1, self.size)
        target = target.reshape(-1)
        ignore = target == self.padding_idx
        dist = torch.full_like(x, self.smoothing / (self.size - 1))
        dist.scatter_(1, target.masked_fill(ignore, 0).unsqueeze(1), self.confidence)
        kl = torch.nn.functional.kl_div(torch.log_softmax(x, dim=1), dist, reduction="none")       # 0 where dist is 0
        denom = (ignore.numel() - int(ignore.sum().item())) if self.normalize_length else batch
        return kl.masked_fill(ignore.unsqueeze(1), 0).sum() / denom
