"""Joint CTC/attention decoding on the decode-tail batch of tools/bench_decode.py (B = 8, T' <= 250, V = 5000, d = 512, 8 heads,
a left decoder of 3 blocks), beams 4 and 10, fp32 and bf16: backend "kernels" against backend "framework" on the same GPU -- ms
per call, executed frames, launches per frame (counted by the engine and by torch.profiler), decoder evaluations per
utterance, host reads, cache bytes, the share of pafc_joint_frame / pafc_mha_step_paths / mha_rows in the kernel time, and
whether both backends decode the same best hypothesis.

The weights are random: the CTC head's blank logit is raised by --blank-bias so that the search is blank-dominated as a trained
model's is (without it every frame emits a token and every prefix is new).  Random weights also make near-ties common, so
"same best" is reported, not asserted.  Prints one JSON line.

    python tools/bench_joint_decoding.py [--reps 3] [--frames N] [--blank-bias 6.0] [--skip-framework]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel                # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.ctc import CTC                            # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder       # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding        # noqa: E402


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
    return r, launches, total / 1e3, {"joint_frame": share("frame_kernel"), "mha_step_paths": share("mha_step_paths_kernel"),
                                     "mha_rows": share("mha_rows_kernel"), "candidates": share("candidates_kernel")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--blank-bias", type=float, default=6.0)
    ap.add_argument("--skip-framework", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(777)
    dev = "cuda"
    B, T, D, V = 8, args.frames, 512, 5000
    dec = BiTransformerDecoder(V, D, attention_heads=8, linear_units=2048, num_blocks=3, r_num_blocks=0, dropout_rate=0.0,
                               positional_dropout_rate=0.0)
    model = ASRModel(V, _NoEncoder(), CTC(V, D), decoder=dec).eval().to(dev)
    with torch.no_grad():
        model.ctc.ctc_lo.bias[0] += args.blank_bias
    enc = torch.randn(B, T, D, device=dev)
    lens = [max(1, int(T * f)) for f in (1.0, 0.96, 0.924, 0.8, 0.72, 0.6, 0.48, 0.4)]
    out = {"workload": f"B={B}, T'<={T}, V={V}, d={D}, 8 heads, 3 decoder blocks; random weights, blank logit + {args.blank_bias}",
           "device": torch.cuda.get_device_name(0), "runs": []}
    with torch.no_grad():
        ctc = model.ctc.log_softmax(enc)
        for dtype in (torch.float32, torch.bfloat16):
            model.decoder.to(dtype)
            for beam in (4, 10):
                run = lambda backend: joint_decoding(model, enc, lens, ctc, 0.5, beam, backend=backend)       # noqa: E731
                dt_k, rk = timed(lambda: run("kernels"), args.reps)
                _, launches, kernel_ms, shares = kernel_profile(lambda: run("kernels"))
                st = rk[0].stats
                executed = max(r.stats["frames_executed"] for r in rk)
                row = {"dtype": str(dtype).replace("torch.", ""), "beam": beam, "kernels_ms": round(dt_k * 1e3, 1),
                       "frames": T, "frames_executed_max": executed,
                       "launches_per_frame_profiled": round(launches / T, 1), "launches_per_frame_counted": st["launches_per_frame"],
                       "decoder_evaluations_per_utterance": [r.stats["decoder_evaluations"] for r in rk],
                       "host_reads": st["host_reads"], "cache_bytes": st["cache_bytes"], "kernel_time_ms": round(kernel_ms, 1),
                       "kernel_time_share": shares, "best_lengths": [len(r.tokens) for r in rk], "utterances": B}
                if not args.skip_framework:
                    dt_f, rf = timed(lambda: run("framework"), 1)
                    row.update(framework_ms=round(dt_f * 1e3, 1), speedup=round(dt_f / dt_k, 2),
                               framework_decoder_evaluations=[r.stats["decoder_evaluations"] for r in rf],
                               same_best=sum(a.tokens == b.tokens for a, b in zip(rk, rf)))
                out["runs"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
