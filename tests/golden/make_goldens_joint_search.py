"""Record what the reference's own time-synchronous beam search (BeamSearchTimeSync, wenet/espnet/beam_search_timesync.py, the
class behind joint_decoding, wenet/transformer/search.py:450-496) decodes on this project's attention decoder (needs the
reference tree; see oracle/ref_shim.py):

    python tests/golden/make_goldens_joint_search.py

writes tests/golden/joint_search.json: for the shared case of tests/test_joint_search.py (tests/attn_rescore_cases.py's models
in float64, the blank logit of the CTC head raised as that module says, each of the three utterances at its own length), pre-
and post-norm, beams 1, 4 and 10 and three settings of (ctc_weight, length_bonus, blank_threshold), what the class returns
for its best hypothesis: tokens, score, start and end frames and the per-token confidences exp(max(ctc, att)).  The class
runs unmodified with sos = model.sos; it calls decoder.forward_one_step_with_attn with a sixth argument (cat_embs, None here)
and expects a third result (the attention weights, unused): the adapter below maps that onto this project's forward_one_step
and changes nothing else (the class builds its memory mask as float ones; this project's attention takes a bool mask, so
the adapter casts it).  The class hands scores and confidences back as float32 tensors; a score of -inf is stored as null."""
import json
import math
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SETTINGS = ((0.5, 0.5, 1.0), (0.3, 0.0, 0.9), (1.0, 0.5, 1.0))


def main():
    from oracle import ref_shim
    ref_shim.install()
    from wenet.espnet.beam_search_timesync import BeamSearchTimeSync
    from tests import attn_rescore_cases as C
    from tests.test_joint_search import BLANK_BOOST, SKIP_BOOST, SKIP_FRAMES, ctc_case, joint_model
    out = dict(blank_boost=BLANK_BOOST, skip_boost=SKIP_BOOST, skip_frames=list(SKIP_FRAMES), cases=[])
    enc = C.encoder_out()
    for pre in (True, False):
        model = joint_model(pre)
        dec = model.decoder.left_decoder
        adapter = types.SimpleNamespace(forward_one_step_with_attn=lambda m, mm, t, tm, cache, cat_embs: (
            *dec.forward_one_step(m, mm.bool(), t, tm, cache), None))
        ctc = ctc_case(pre)
        for beam in (1, 4, 10):
            for ctc_w, bonus, thr in SETTINGS:
                utts = []
                for b, n in enumerate(C.LENS):
                    search = BeamSearchTimeSync(sos=model.sos, beam_size=beam, ctc_probs=ctc[b, :n], decoder=adapter,
                                                weights=dict(decoder=1.0 - ctc_w, ctc=ctc_w, length_bonus=bonus),
                                                pre_beam_ratio=1.5, blank=0, blank_threshold=thr)
                    with torch.no_grad():
                        hyps, scores, starts, ends, confs = search(x=enc[b:b + 1, :n], cat_embs=None)
                    score = scores[0].item()
                    utts.append(dict(tokens=hyps[0][1:].tolist(), score=None if math.isinf(score) else score,
                                     times=starts[0][0, 1:].tolist(), end_times=ends[0][0, 1:].tolist(),
                                     tokens_confidence=[math.exp(c) for c in confs[0][1:].tolist()]))
                out["cases"].append(dict(normalize_before=pre, beam=beam, ctc_weight=ctc_w, length_bonus=bonus,
                                         blank_threshold=thr, utterances=utts))
    path = os.path.join(ROOT, "tests", "golden", "joint_search.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
