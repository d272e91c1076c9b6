"""Capture the gradient fixture of the limited-context attention from the reference (needs the reference tree; see
oracle/ref_shim.py):

    python tests/golden/make_goldens_lca_train.py

tests/golden/lca_attention_grad.pt -- the reference's LimitedRelPositionMultiHeadedAttention in float64 on the CPU, weights,
inputs and position rows exactly those of two cases of tests/golden/lca_attention.pt, (w, B, T) = (16, 2, 67) (t_pad 96: padding
keys) and (16, 2, 32) (T a multiple of 2 w: none), with the reference's own t_pad.  The loss is sum(out * g), g drawn from
seed + GRAD_SEED_OFFSET; kept per case: the gradients with respect to x, pos_bias_u, pos_bias_v and linear_pos.weight."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import synth  # noqa: E402
from tests.golden.make_goldens import load_synth, save  # noqa: E402
from tests.golden.make_goldens_lca import D, HEADS, POS_OFFSET, WEIGHT_SEED, cases_of  # noqa: E402

GRAD_SEED_OFFSET = 500
PICK = ((16, 2, 67), (16, 2, 32))
KEPT = ("pos_bias_u", "pos_bias_v", "linear_pos.weight")


def main():
    ref_shim.install()
    torch.set_num_threads(4)
    from wenet.transformer.attention import LimitedRelPositionMultiHeadedAttention
    from wenet.transformer.embedding import RelPositionalEncoding
    table = RelPositionalEncoding(D, 0.0).position_encoding(POS_OFFSET, 67, False)             # (1, 67, D) float32
    out = dict(d=D, heads=HEADS, weight_seed=WEIGHT_SEED, grad_seed_offset=GRAD_SEED_OFFSET, cases=[])
    for w, B, T in PICK:
        n, lens = next((n, c[2]) for n, c in enumerate(cases_of(w)) if (c[0], c[1]) == (B, T))
        seed = 1000 * w + n                                                                       # make_goldens_lca's input seed
        m = LimitedRelPositionMultiHeadedAttention(HEADS, D, 0.0, True, [w, w], 0, 1, False, 0).eval()
        load_synth(m, WEIGHT_SEED)
        m = m.double()
        x = synth.randn((B, T, D), seed).double().requires_grad_(True)
        g = synth.randn((B, T, D), seed + GRAD_SEED_OFFSET).double()
        mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1)
        y, _ = m(x, x, x, mask, table[:, :T].double(), torch.zeros((0, 0, 0, 0)))
        params = dict(m.named_parameters())
        grads = torch.autograd.grad((y * g).sum(), [x] + [params[k] for k in KEPT])
        case = dict(w=w, B=B, T=T, seed=seed, dx=grads[0].clone())
        case.update({k: t.clone() for k, t in zip(KEPT, grads[1:])})
        out["cases"].append(case)
    save("lca_attention_grad", out)


if __name__ == "__main__":
    main()
