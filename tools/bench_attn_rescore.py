"""Attention rescoring on the decode-tail batch of tools/bench_decode.py (B = 8, T' <= 250, D = 512, V = 5000, beam 8): the
second pass of a bitransformer decoder (8 heads, 2048 units, 3 + 3 blocks, reverse_weight 0.3) over the n-best lists of a CTC
prefix beam search, through score_attention(backend="kernels") next to backend="framework" on the same GPU.  Reports the time
per call, the kernel launches per call (torch.profiler) and the peak of the logits buffer: the kernels backend's largest
output_layer chunk (AttentionScores.stats) against the framework's largest (beam, L + 1, V) log-softmax input.  Random
weights and peaky synthetic posteriors; prints one JSON line.  --dtype fp32 | bf16 (default fp32)."""
import json
import sys
import time

import torch
from torch.profiler import ProfilerActivity, profile

from paper_accurate_fast_cheap_amd.transformer import attn_rescore
from paper_accurate_fast_cheap_amd.transformer import search as S
from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder

torch.manual_seed(777)
dev = "cuda"
dtype = torch.bfloat16 if "bf16" in sys.argv[1:] else torch.float32
B, T, D, V, beam, rw = 8, 250, 512, 5000, 8, 0.3
ctc = CTC(V, D).eval().to(dev)
enc = torch.randn(B, T, D, device=dev) * 3
lens = torch.tensor([250, 240, 231, 200, 180, 150, 120, 100], device=dev)
decoder = BiTransformerDecoder(V, D, attention_heads=8, linear_units=2048, num_blocks=3, r_num_blocks=3)
model = ASRModel(V, torch.nn.Identity(), ctc, decoder=decoder).eval().to(dev)
model.decoder.to(dtype)


def timed(fn, n=5):
    fn(); torch.cuda.synchronize(); t0 = time.time()
    for _ in range(n): r = fn()
    torch.cuda.synchronize(); return (time.time() - t0) / n, r


def launches(fn):
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


with torch.no_grad():
    first = S.ctc_prefix_beam_search(ctc.log_softmax(enc), lens, beam)
    hyps = [[list(h) for h in r.nbest] for r in first]
    lens_h = lens.tolist()
    n_hyp, n_rows = sum(len(nb) for nb in hyps), sum(len(h) + 1 for nb in hyps for h in nb)
    out = {"workload": f"B={B}, T'<={T}, D={D}, V={V}, beam {beam}: {n_hyp} hypotheses, {n_rows} packed rows, "
                       f"3+3 blocks, reverse_weight {rw}, {str(dtype).split('.')[-1]}"}
    run = lambda backend: model.score_attention(enc, lens_h, hyps, rw, backend=backend)      # noqa: E731
    dt_k, sk = timed(lambda: run("kernels"))
    dt_f, sf = timed(lambda: run("framework"))
    out["kernels_ms"], out["framework_ms"] = round(dt_k * 1e3, 2), round(dt_f * 1e3, 2)
    out["kernels_launches"], out["framework_launches"] = launches(lambda: run("kernels")), launches(lambda: run("framework"))
    out["kernels_logits_peak_bytes"] = sk.stats["logits_peak_bytes"]
    widest = max(len(nb) * (max(len(h) for h in nb) + 1) for nb in hyps if nb)          # rows of the recipe's largest batch
    out["framework_logits_peak_bytes"] = widest * V * (2 if dtype == torch.bfloat16 else 4)
    out["logits_cap_bytes"] = attn_rescore.LOGITS_CAP_BYTES
    best = lambda s: [max(range(len(nb)), key=lambda i: nb[i]) if nb else -1 for nb in s.attn(rw)]    # noqa: E731
    out["same_best"] = sum(a == b for a, b in zip(best(sk), best(sf)))
    out["max_abs_score_diff"] = max(abs(a - b) for x, y in zip(sk.attn(rw), sf.attn(rw)) for a, b in zip(x, y))
print(json.dumps(out))
