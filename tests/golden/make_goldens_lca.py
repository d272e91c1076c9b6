"""Capture the limited-context attention fixtures from the reference (needs the reference tree; see oracle/ref_shim.py):

    python tests/golden/make_goldens_lca.py

tests/golden/lca_attention.pt -- the reference's LimitedRelPositionMultiHeadedAttention in float64: d = 128, 2 heads,
w in {2, 5, 16}, (B, T) in {(1, 1), (2, 2w), (3, 2w + 1), (2, 4w + 3), (1, 67)} with rows shorter than T in the batched
cases (the mask the reference is handed; it does not reach the output), pos_emb = rows [POS_OFFSET, POS_OFFSET + T) of the
reference's sinusoid table, synthetic weights (tests/synth.py: spec + seed, pos_bias_u / v non-zero) drawn in float32, so an
fp32 load of them is exact.  Inputs are regenerated from their seeds.  Per case: the output, the returned cache's shape and
the cache at the frames CACHE_FRAMES(T) (whole, the 645 rows of cat(k, v) would take the file past its size limit).

tests/golden/encoder_lca.pt -- the reference's ConformerEncoder in float32 with the reduced configuration of
encoder_reduced_f32 except selfattention_layer_type: limited_rel_selfattn, att_context_size: [4, 4], cnn_module_norm:
layer_norm: forward on (3, 135, 80) with lengths [135, 90, 37] (T' = 33, T_pad = 40) and forward_chunk at offset 7 with
required_cache_size -1 and 4."""
import os
import sys

import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import synth  # noqa: E402
from tests.golden.make_goldens import REDUCED, YAML, load_synth, save  # noqa: E402

D, HEADS, POS_OFFSET, WEIGHT_SEED = 128, 2, 5, 91
CONTEXTS = (2, 5, 16)


def cases_of(w):
    """(B, T, lengths, input seed) per case of one context size."""
    return [(1, 1, [1]), (2, 2 * w, [2 * w, w]), (3, 2 * w + 1, [2 * w + 1, w + 1, 1]), (2, 4 * w + 3, [4 * w + 3, 2 * w + 2]),
            (1, 67, [67])]


def cache_frames(T):
    return sorted({0, T // 2, T - 1})


def attention_golden():
    from wenet.transformer.attention import LimitedRelPositionMultiHeadedAttention
    from wenet.transformer.embedding import RelPositionalEncoding
    table = RelPositionalEncoding(D, 0.0).position_encoding(POS_OFFSET, 67, False)             # (1, 67, D) float32
    out = dict(d=D, heads=HEADS, pos_offset=POS_OFFSET, pos_rows=table.clone(), weight_seed=WEIGHT_SEED, cases=[])
    for w in CONTEXTS:
        m = LimitedRelPositionMultiHeadedAttention(HEADS, D, 0.0, True, [w, w], 0, 1, False, 0).eval()
        spec, cs = load_synth(m, WEIGHT_SEED)
        out["spec"], out["checksum"] = spec, cs
        m = m.double()
        for n, (B, T, lens) in enumerate(cases_of(w)):
            seed = 1000 * w + n
            x = synth.randn((B, T, D), seed).double()
            mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1)
            y, cache = m(x, x, x, mask, table[:, :T].double(), torch.zeros((0, 0, 0, 0)))
            assert y.dtype == torch.float64 and tuple(cache.shape) == (B, HEADS, T, 2 * D // HEADS)
            out["cases"].append(dict(w=w, B=B, T=T, lens=lens, seed=seed, out=y.clone(), cache_shape=tuple(cache.shape),
                                     cache_frames=cache_frames(T), cache_at=cache[:, :, cache_frames(T)].clone()))
    save("lca_attention", out)


def encoder_golden():
    from wenet.transformer.cmvn import GlobalCMVN
    from wenet.transformer.encoder import ConformerEncoder
    cfg = yaml.safe_load(open(os.path.join(ref_shim.REFERENCE_ROOT, YAML)))
    conf = dict(cfg["encoder_conf"])
    conf.update(REDUCED)
    conf.update(rwkv_do_bfloat16=False, selfattention_layer_type="limited_rel_selfattn", att_context_size=[4, 4],
                cnn_module_norm="layer_norm")
    mean = synth.randn((80,), 40)
    istd = torch.rand(80, generator=torch.Generator().manual_seed(41)) + 0.5
    enc = ConformerEncoder(80, global_cmvn=GlobalCMVN(mean, istd), **conf).eval()
    spec, cs = load_synth(enc, 92)
    xs = synth.randn((3, 135, 80), 93, 2.0)
    lens = torch.tensor([135, 90, 37])
    xc = synth.randn((1, 63, 80), 94, 2.0)                # 15 frames after subsampling: T_pad = 16
    y, masks = enc(xs, lens)
    assert y.shape[1] == 33
    # (the reference's own default att_mask, (0, 0, 0), fails inside its blocked layout: it is handed a real one)
    empty, ones = torch.zeros((0, 0, 0, 0)), torch.ones((1, 1, 15), dtype=torch.bool)
    full = enc.forward_chunk(xc, 7, -1, empty, empty, ones)                 # (xs, [layer outputs,] att_cache, cnn_cache)
    last4 = enc.forward_chunk(xc, 7, 4, empty, empty, ones)
    assert full[0].shape[1] == 15
    assert torch.equal(full[0], last4[0])
    save("encoder_lca", dict(spec=spec, seed=92, checksum=cs, conf=conf, xs_seed=93, lens=lens, chunk_seed=94, chunk_offset=7,
                             out=y, masks=masks, chunk_y=full[0], chunk_att_cache=full[-2].clone(),
                             chunk_att_cache_r4=last4[-2].clone(), cnn_cache_shape=tuple(full[-1].shape)))


def main():
    ref_shim.install()
    torch.set_grad_enabled(False)
    torch.set_num_threads(4)
    attention_golden()
    encoder_golden()


if __name__ == "__main__":
    main()
