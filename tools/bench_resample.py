"""The resampler in front of the fbank (dataset.resample: pafc_resample_batch, pafc_resample_rows).

    python tools/bench_resample.py [--utts 64] [--iters 200] [--repeats 5] [--rates 44100 48000 8000] [--streams 1 8 64]     one JSON line

(a) `--utts` synthetic utterances of 1-20 s (seeded) at each of `--rates`, lying in a (B, S_max) buffer with their lengths on
    the device, to 16 kHz: ONE resample_batch launch, next to the same definition written with the framework on the same GPU
    -- zero padding, a strided conv1d with the dense float32 filter (new, 1, 2 W + orig), a transpose and a mask behind every
    row's length.
(b) a 0.64 s packet per stream at 1 / 8 / 64 streams through ResampleSlotStreamer.feed_rows in the steady state (one small
    upload and 2 launches per feed).

Every figure is device ms between two events around `--iters` calls after 3 warm-up calls, median (min .. max) over
`--repeats`; for (b) the host issues the calls, so a feed that the device finishes faster than Python issues it measures the
issue rate.  Each GPU step runs in a child process of its own under its own time limit; the tool stops at the first step that
fails or runs out of time and exits non-zero.  It asserts no speed."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

PACKET_S = 0.64
STEP_LIMIT_S = {"batch": 240, "stream": 240}


def timed(fn, iters, repeats):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def framework_resample(padded, lens, plan, dense):
    """The definition as framework ops: (out (B, N_max), out_lengths)."""
    import torch
    B, S = padded.shape
    N = (plan.new * S + plan.orig - 1) // plan.orig
    frames = (N + plan.new - 1) // plan.new
    right = max(0, (frames - 1) * plan.orig + plan.taps - plan.W - S)
    x = torch.nn.functional.pad(padded, (plan.W, right)).unsqueeze(1)
    y = torch.nn.functional.conv1d(x, dense.unsqueeze(1), stride=plan.orig)[:, :, :frames]
    y = y.transpose(1, 2).reshape(B, -1)[:, :N]
    n = (plan.new * lens + plan.orig - 1) // plan.orig
    return y * (torch.arange(N, device=y.device).unsqueeze(0) < n.unsqueeze(1)), n


def step_batch(a):
    import torch
    from paper_accurate_fast_cheap_amd.dataset.resample import resample_batch, resample_plan
    rows = []
    for rate in a.rates:
        rng = random.Random(1)
        secs = [20.0] + [rng.uniform(1.0, 20.0) for _ in range(a.utts - 1)]
        samples = [int(s * rate) for s in secs]
        g = torch.Generator(device="cuda").manual_seed(rate)
        padded = (torch.randn(a.utts, max(samples), device="cuda", generator=g) * 3000).round()
        lens = torch.tensor(samples, dtype=torch.int64, device="cuda")
        padded *= torch.arange(padded.size(1), device="cuda").unsqueeze(0) < lens.unsqueeze(1)
        plan = resample_plan(rate, 16000)
        dense = torch.zeros(plan.new, plan.taps)
        dense.scatter_(1, plan.first.long().unsqueeze(1) + torch.arange(plan.span).unsqueeze(0), plan.coef)
        dense = dense.cuda()
        out, n = resample_batch(padded, lens, rate, 16000)
        ref, n_ref = framework_resample(padded, lens, plan, dense)
        assert torch.equal(n, n_ref)
        rows.append(dict(rate=rate, utts=a.utts, audio_s=round(sum(secs), 1), in_mb=round(padded.numel() * 4 / 1e6, 1),
                         out_mb=round(out.numel() * 4 / 1e6, 1), launches=1,
                         kernel_ms=timed(lambda: resample_batch(padded, lens, rate, 16000), a.iters, a.repeats),
                         framework_conv1d_ms=timed(lambda: framework_resample(padded, lens, plan, dense), a.iters, a.repeats),
                         max_abs_diff_vs_framework=float((out - ref).abs().max()), checksum=float(out.double().sum())))
    return dict(mode="batch", results=rows)


def step_stream(a):
    import torch
    from paper_accurate_fast_cheap_amd.dataset.resample import ResampleSlotStreamer
    rows = []
    for rate in a.rates:
        n = int(PACKET_S * rate)
        for S in a.streams:
            g = torch.Generator(device="cuda").manual_seed(S)
            pk = (torch.randn(S, n, device="cuda", generator=g) * 3000).round()
            st = ResampleSlotStreamer(S, rate, 16000)
            ids = list(range(S))
            st.feed_rows(ids, pk)                              # the first packet fills the carry
            rows.append(dict(rate=rate, streams=S, packet_samples=n, launches_per_feed=2,
                             ms_per_feed=timed(lambda: st.feed_rows(ids, pk), a.iters, a.repeats)))
    return dict(mode="stream", packet_s=PACKET_S, results=rows)


STEPS = {"batch": step_batch, "stream": step_stream}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rates", type=int, nargs="*", default=[44100, 48000, 8000])
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--step", choices=sorted(STEPS), help=argparse.SUPPRESS)       # (a child process of this tool: one GPU step)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step](a)))
        return 0
    out = dict(bench="resample", steps=[])
    for name in ("batch", "stream"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--utts", str(a.utts), "--iters", str(a.iters),
               "--repeats", str(a.repeats), "--rates"] + [str(r) for r in a.rates] + ["--streams"] + [str(s) for s in a.streams]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(out, failed=name, why=f"no result within {STEP_LIMIT_S[name]} s")))
            return 1
        if done.returncode != 0:
            print(json.dumps(dict(out, failed=name, returncode=done.returncode, stderr=done.stderr[-2000:])))
            return 1
        out["steps"].append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
