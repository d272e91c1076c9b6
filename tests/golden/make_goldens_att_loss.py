"""Capture the attention loss' host functions from the reference (needs the reference tree; see oracle/ref_shim.py):

    python tests/golden/make_goldens_att_loss.py

writes tests/golden/att_loss_host.pt: a batch of transcripts with an empty one, V = 11, and what the reference's own
add_sos_eos, reverse_pad_list, th_accuracy and LabelSmoothingLoss (smoothing 0 and 0.1, both normalisations) return for it
and for float64 logits.  tests/test_att_loss.py holds the product's functions to these."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from oracle import ref_shim
    ref_shim.install()
    from wenet.transformer.label_smoothing_loss import LabelSmoothingLoss
    from wenet.utils.common import add_sos_eos, reverse_pad_list, th_accuracy
    torch.manual_seed(23)
    V, sos, eos, ignore = 11, 10, 10, -1
    lens = torch.tensor([4, 0, 1, 6])
    text = torch.full((4, 6), ignore, dtype=torch.int64)
    for b, n in enumerate(lens.tolist()):
        text[b, :n] = torch.randint(0, V - 1, (n,))
    ys_in, ys_out = add_sos_eos(text, sos, eos, ignore)
    r_text = reverse_pad_list(text, lens, float(ignore))
    r_ys_in, r_ys_out = add_sos_eos(r_text, sos, eos, ignore)
    logits = torch.randn(4, ys_out.size(1), V, dtype=torch.float64) * 2
    for b in range(4):                                  # some rows right, so that the accuracy is neither 0 nor 1
        for j in range(0, int(lens[b]) + 1, 2):
            logits[b, j, ys_out[b, j]] = 9.0
    losses = {}
    for smoothing in (0.0, 0.1):
        for norm in (False, True):
            losses[(smoothing, norm)] = LabelSmoothingLoss(V, ignore, smoothing, norm)(logits, ys_out)
            losses[(smoothing, norm, "r")] = LabelSmoothingLoss(V, ignore, smoothing, norm)(logits, r_ys_out)
    acc = th_accuracy(logits.view(-1, V), ys_out, ignore_label=ignore)
    out = dict(V=V, sos=sos, eos=eos, ignore=ignore, text=text, lens=lens, ys_in=ys_in, ys_out=ys_out, r_text=r_text,
               r_ys_in=r_ys_in, r_ys_out=r_ys_out, logits=logits, losses=losses, acc=acc)
    path = os.path.join(ROOT, "tests", "golden", "att_loss_host.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
