"""Two-pass decoding on the batch of tools/bench_decode.py (B = 8, T' <= 250, V = 5000, LSTM 2 x 640, joint 640, beam 8): a CTC
prefix beam search as the first pass, then the n-best lists re-scored with the transducer's full-sum score over their prefix
tries (Transducer.score_hypotheses, backend "kernels").  Reports, in one JSON line: ms of the first pass, of the second pass,
of the second pass with sharing disabled (every hypothesis its own utterance: the rows the reference's repeat computes, through
the same entry), of rnnt_beam_search with frame_body="kernels" for comparison, the joint rows with and without sharing, and how
often the re-scored winner differs from the first-pass winner.  Random weights and synthetic posteriors: the times are the
point, not the hypotheses.  One process; each timed section ends in a synchronise."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paper_accurate_fast_cheap_amd import hip_ops  # noqa: E402
from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint  # noqa: E402
from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor  # noqa: E402
from paper_accurate_fast_cheap_amd.transducer.search.rescoring import build_arc_tables, rescore  # noqa: E402
from paper_accurate_fast_cheap_amd.transducer.transducer import IGNORE_ID, Transducer, add_blank  # noqa: E402
from paper_accurate_fast_cheap_amd.transformer import search as S  # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.ctc import CTC  # noqa: E402

B, T, D, V, BEAM = 8, 250, 512, 5000, 8


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n):
        r = fn()
    torch.cuda.synchronize()
    return (time.time() - t0) / n * 1e3, r


def main():
    torch.manual_seed(777)
    dev = "cuda"
    pred = RNNPredictor(V, embed_size=640, output_size=640, embed_dropout=0.1, hidden_size=640, num_layers=2)
    joint = TransducerJoint(V, enc_output_size=D, pred_output_size=640, join_dim=640)
    model = Transducer(V, 0, torch.nn.Identity(), pred, joint, ctc=CTC(V, D)).eval().to(dev, torch.bfloat16)
    enc = (torch.randn(B, T, D, device=dev) * 3).to(torch.bfloat16)
    lens = torch.tensor([250, 240, 231, 200, 180, 150, 120, 100], device=dev)
    host_lens = lens.tolist()
    out = {"workload": f"B={B}, T'<={T}, V={V}, beam {BEAM}, predictor LSTM 2x640, joint 640, bf16"}
    with torch.no_grad():
        logp = model.ctc.log_softmax(enc)
        ms, first = timed(lambda: S.ctc_prefix_beam_search(logp, lens, BEAM), 5)
        out["first_pass_ctc_prefix_beam_ms"] = round(ms, 2)
        hyps = [r.nbest for r in first]
        ms, td = timed(lambda: model.score_hypotheses(enc, host_lens, hyps, backend="kernels"), 5)
        out["second_pass_kernels_ms"] = round(ms, 2)

        # the kernels alone, with and without sharing, on the same predictor rows
        flat = [h for nbest in hyps for h in nbest]
        pad = torch.full((len(flat), max(max(len(h) for h in flat), 1)), IGNORE_ID, dtype=torch.int64)
        for n, h in enumerate(flat):
            pad[n, :len(h)] = torch.tensor(h, dtype=torch.int64)
        P = joint.pred_ffn(pred(add_blank(pad.to(dev), 0, IGNORE_ID)))
        E = joint.enc_ffn(enc)
        w, b = joint.ffn_out.weight, joint.ffn_out.bias
        scores = {}
        for name, share in (("shared", True), ("unshared", False)):
            tb = build_arc_tables(hyps, host_lens, V, 0, pred_stride=P.shape[1], share=share)
            ms, sc = timed(lambda: hip_ops.rnnt_score_hypotheses(E, P, w, b, None, tb, 0), 5)
            out[f"score_kernels_{name}_ms"] = round(ms, 2)
            out[f"rows_{name}"] = tb.rows
            scores[name] = sc
        out["row_ratio"] = round(out["rows_shared"] / max(out["rows_unshared"], 1), 3)
        out["shared_equals_unshared_bitwise"] = bool(torch.equal(scores["shared"], scores["unshared"]))
        model.init_bs()
        kw = dict(beam_size=BEAM, ctc_weight=0.3, transducer_weight=0.7)
        ms, _ = timed(lambda: model.bs.prefix_beam_search_decode(enc, lens, logp, frame_body="kernels", **kw), 2)
        out["rnnt_beam_search_kernels_ms"] = round(ms, 1)
        second = rescore(first, td, 0.3, 0.7)
        out["hypotheses"] = len(flat)
        out["winner_changed"] = sum(list(a.tokens) != list(c.tokens) for a, c in zip(first, second))
        out["utterances"] = B
    print(json.dumps(out))


if __name__ == "__main__":
    main()
