"""The seeded model and n-best lists that tests/test_attn_rescore.py (CPU) and tests/test_attn_rescore_gpu.py share: d = 128,
2 heads, linear_units 256, V = 53, 1 + 1 blocks; three utterances with T' = 1, 17, 70 frames carrying 1, 3 and 4 hypotheses of
the lengths 0, 1, 15, 16, 17, 40 (an empty one, one token, and both sides of the 16-row tile of the attention kernel)."""
import random

import torch

V, D, HEADS, UNITS = 53, 128, 2, 256
LENS = [1, 17, 70]
CONF = dict(attention_heads=HEADS, linear_units=UNITS, num_blocks=1, r_num_blocks=1, dropout_rate=0.0,
            positional_dropout_rate=0.0)


class FixedEncoder(torch.nn.Module):
    def __init__(self, enc_out):
        super().__init__()
        self.register_buffer("enc_out", enc_out)

    def output_size(self):
        return self.enc_out.shape[-1]

    def forward(self, x, lens, *a, **k):
        mask = (torch.arange(self.enc_out.shape[1], device=lens.device)[None, :] < lens[:, None]).unsqueeze(1)
        return self.enc_out[:x.shape[0]], mask


def hypotheses():
    rng = random.Random(11)
    mk = lambda n: [rng.randrange(1, V - 1) for _ in range(n)]              # noqa: E731
    return [[mk(0)], [mk(1), mk(15), mk(16)], [mk(17), mk(40), mk(16), mk(0)]]


def encoder_out():
    g = torch.Generator().manual_seed(21)
    return torch.randn(3, max(LENS), D, generator=g, dtype=torch.float64)


def model(normalize_before: bool, dtype=torch.float64, bidirectional: bool = True, seed: int = 7, enc_out=None, **conf_kw):
    """ASRModel(fixed encoder, CTC, seeded attention decoder).  The LayerNorm gains / biases and the linear biases are perturbed
    so that none of them is its trivial initial value.  enc_out / conf_kw: another memory (its last dimension is d) and decoder
    keys instead of the shared case's."""
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder, TransformerDecoder
    torch.manual_seed(seed)
    conf = dict(CONF, normalize_before=normalize_before, **conf_kw)
    enc_out = encoder_out() if enc_out is None else enc_out
    D = enc_out.shape[-1]
    if bidirectional:
        dec = BiTransformerDecoder(V, D, **conf)
    else:
        conf.pop("r_num_blocks")
        dec = TransformerDecoder(V, D, **conf)
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if "norm" in name:
                p.add_(torch.randn_like(p) * 0.1)
            elif name.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.05)
    m = ASRModel(V, FixedEncoder(enc_out), CTC(V, D), decoder=dec).eval()
    return m.to(dtype)


def ref_conf(normalize_before: bool, bidirectional: bool = True, heads: int = HEADS):
    return dict(heads=heads, num_blocks=1, r_num_blocks=1, normalize_before=normalize_before, bidirectional=bidirectional,
                activation="relu")


def flatten(nested):
    return [v for nb in nested for h in nb for v in h]
