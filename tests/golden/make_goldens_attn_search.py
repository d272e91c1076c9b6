"""Record what the reference's own attention_beam_search (wenet/transformer/search.py:251-360) decodes on this project's
attention decoder (needs the reference tree; see oracle/ref_shim.py):

    python tests/golden/make_goldens_attn_search.py

writes tests/golden/attn_search_tokens.json: for the shared case of tests/test_attn_search.py (tests/attn_rescore_cases.py's
models in float64 with the eos bias raised by EOS_BOOST, the three utterances batched), pre- and post-norm, beams 1, 4 and 10,
length_penalty 0 and 0.6, the token lists the reference returns.  The reference's loop calls decoder.forward_one_step with a
sixth argument (cat_embs, None here) that this project's method does not take: the adapter below drops it and changes nothing
else.  tests/test_attn_search.py holds the framework backend to these lists."""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from oracle import ref_shim
    ref_shim.install()
    from wenet.transformer.search import attention_beam_search
    from tests import attn_rescore_cases as C
    from tests.test_attn_search import EOS_BOOST, search_model, batch_mask
    out = dict(eos_boost=EOS_BOOST, cases=[])
    for pre in (True, False):
        model = search_model(pre)
        dec = model.decoder
        adapter = types.SimpleNamespace(
            sos=model.sos, eos=model.eos, special_tokens=None, ignore_id=-1,
            decoder=types.SimpleNamespace(forward_one_step=lambda m, mm, t, tm, cache, cat_embs=None: dec.forward_one_step(
                m, mm, t, tm, cache)))
        for beam in (1, 4, 10):
            for lp in (0.0, 0.6):
                with torch.no_grad():
                    res = attention_beam_search(adapter, model.encoder.enc_out, batch_mask(), beam, lp)
                out["cases"].append(dict(normalize_before=pre, beam=beam, length_penalty=lp, tokens=[r.tokens for r in res]))
    path = os.path.join(ROOT, "tests", "golden", "attn_search_tokens.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
