"""Capture a MultiHeadedAttention fixture from the reference (needs the reference tree; see oracle/ref_shim.py):

    python tests/golden/make_goldens_mha.py

writes tests/golden/mha_decoder.pt: d = 64, 4 heads, the module's weights, query / memory inputs, a mask with padded keys and
a lower-triangular one, and the reference's outputs, all float64.  tests/test_attn_rescore.py holds the float64 restatement
and the product module to it."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from oracle import ref_shim
    ref_shim.install()
    from wenet.transformer.attention import MultiHeadedAttention
    torch.manual_seed(17)
    d, heads, B, L, S = 64, 4, 3, 5, 9
    m = MultiHeadedAttention(heads, d, 0.0).double().eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    query, memory = torch.randn(B, L, d, dtype=torch.float64), torch.randn(B, S, d, dtype=torch.float64)
    key_lens = torch.tensor([9, 4, 1])
    memory_mask = (torch.arange(S)[None, :] < key_lens[:, None]).unsqueeze(1)             # (B, 1, S): padded keys hidden
    q_lens = torch.tensor([5, 3, 1])
    tgt_mask = (torch.arange(L)[None, :] < q_lens[:, None]).unsqueeze(1) & torch.ones(L, L, dtype=torch.bool).tril()[None]
    with torch.no_grad():
        cross, _ = m(query, memory, memory, memory_mask)
        self_out, _ = m(query, query, query, tgt_mask)
    out = dict(heads=heads, state_dict={k: v.clone() for k, v in m.state_dict().items()}, query=query, memory=memory,
               memory_mask=memory_mask, tgt_mask=tgt_mask, cross=cross, self_out=self_out)
    path = os.path.join(ROOT, "tests", "golden", "mha_decoder.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
