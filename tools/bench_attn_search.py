"""Attention beam search on the decode-tail batch of tools/bench_decode.py (B = 8, T' <= 250, V = 5000, d = 512, 8 heads, a left
decoder of 3 blocks), beams 8 and 10, fp32 and bf16: backend "kernels" against backend "framework" on the same GPU -- ms per
call (eager, and with step_graph=True), steps, launches per step (counted by torch.profiler), host reads, cache bytes, the share of pafc_mha_step / mha_rows /
pafc_attn_beam_select in the kernel time, and whether both backends decode the same best hypothesis.

The weights are random, so a beam rarely emits eos and every run goes to the cap of 250 steps: the numbers are the cost of 250
steps, the longest a batch of this shape can take, not of a trained decoder that stops at a transcript's length.  Random
weights also make near-ties common, so "same best" is reported, not asserted.  Prints one JSON line.

    python tools/bench_attn_search.py [--reps 3] [--max-len N]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel                # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search  # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.ctc import CTC                            # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder       # noqa: E402


class _NoEncoder(torch.nn.Module):
    def output_size(self):
        return 512


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n):
        r = fn()
    torch.cuda.synchronize()
    return (time.time() - t0) / n, r


def kernel_profile(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        r = fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.key_averages() if getattr(e, "device_time_total", 0) > 0]
    total = sum(e.device_time_total for e in evs)
    launches = sum(e.count for e in evs)

    def share(word):
        return round(sum(e.device_time_total for e in evs if word in e.key) / total, 4) if total else None
    return r, launches, total / 1e3, {"mha_step": share("mha_step_kernel"), "mha_rows": share("mha_rows_kernel"),
                                     "attn_beam_select": share("beam_rows_kernel") + share("beam_utt_kernel")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=None)
    args = ap.parse_args()
    torch.manual_seed(777)
    dev = "cuda"
    B, T, D, V = 8, 250, 512, 5000
    dec = BiTransformerDecoder(V, D, attention_heads=8, linear_units=2048, num_blocks=3, r_num_blocks=0, dropout_rate=0.0,
                               positional_dropout_rate=0.0)
    model = ASRModel(V, _NoEncoder(), CTC(V, D), decoder=dec).eval().to(dev)
    enc = torch.randn(B, T, D, device=dev)
    lens = torch.tensor([250, 240, 231, 200, 180, 150, 120, 100], device=dev)
    mask = (torch.arange(T, device=dev)[None, :] < lens[:, None]).unsqueeze(1)
    out = {"workload": f"B={B}, T'<={T}, V={V}, d={D}, 8 heads, 3 decoder blocks; random weights: every run goes to the cap",
           "device": torch.cuda.get_device_name(0), "runs": []}
    with torch.no_grad():
        for dtype in (torch.float32, torch.bfloat16):
            model.decoder.to(dtype)
            for beam in (8, 10):
                run = lambda backend: attention_beam_search(model, enc, mask, beam, 0.0, backend=backend,     # noqa: E731
                                                            max_len=args.max_len)
                dt_k, rk = timed(lambda: run("kernels"), args.reps)
                dt_g, rg = timed(lambda: attention_beam_search(model, enc, mask, beam, 0.0, backend="kernels",
                                                               max_len=args.max_len, step_graph=True), args.reps)
                dt_f, rf = timed(lambda: run("framework"), 1)
                _, launches, kernel_ms, shares = kernel_profile(lambda: run("kernels"))
                st = rk[0].stats
                out["runs"].append({
                    "dtype": str(dtype).replace("torch.", ""), "beam": beam, "kernels_ms": round(dt_k * 1e3, 1),
                    "kernels_step_graph_ms": round(dt_g * 1e3, 1), "step_graph": rg[0].stats["step_graph"],
                    "step_graph_same_nbest": [r.nbest for r in rg] == [r.nbest for r in rk],
                    "framework_ms": round(dt_f * 1e3, 1), "speedup": round(dt_f / dt_k, 2), "steps": st["steps"],
                    "launches_per_step_profiled": round(launches / max(1, st["steps_issued"]), 1),
                    "launches_per_step_counted": st["launches_per_step"], "host_reads": st["host_reads"],
                    "cache_bytes": st["cache_bytes"], "kernel_time_ms": round(kernel_ms, 1), "kernel_time_share": shares,
                    "same_best": sum(a.tokens == b.tokens for a, b in zip(rk, rf)), "utterances": B})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
