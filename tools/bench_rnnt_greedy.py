"""Batched RNN-T greedy search on the lockstep kernels (hip_ops.rnnt_greedy_search) against the reference's per-utterance loop
(basic_greedy_search) on the same GPU.  Prints one JSON line.

    python tools/bench_rnnt_greedy.py [--steps K] [--warmup W] [--seed S] [--no-basic]

Shapes: c5 of tools/bench_decode.py (B = 8, T' <= 250, V = 5000, LSTM 2 x 640, joint 640, D = 512) and a B = 64 batch, fp32
and whole-model bf16.  Random weights decode degenerately (a frame goes blank at once or repeats one token up to the cap), so
the model is seeded as the golden fixture is (tests/golden/make_goldens_rnnt_greedy.py): encoder dimension 0 drives the blank
logit through enc_ffn, set per frame from a seeded uniform draw, and LSTM unit 0 carries a per-token blank push of the last
emitted token to pred_ffn.  It still emits far more than a trained model: most emitting frames run to the n_steps cap, about
10 tokens per frame.

Per configuration: kernel_ms (median of K calls, E = enc_ffn included), basic_ms (basic_greedy_search per utterance, one call,
c5 only), audio_sec_per_sec (40 ms per encoder frame: 4x subsampling of 10 ms hops), tokens_per_frame, steps (lockstep steps
of one call), host_reads (per call) and same_tokens (utterances whose tokens agree on both paths)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paper_accurate_fast_cheap_amd import hip_ops  # noqa: E402

FRAME_SEC = 0.04


def make_model(V=5000, D=512, E=640, H=640, P=640, J=640, layers=2, seed=0, drive=1.0, beta=7.0, kappa=1.0):
    """A Transducer-shaped namespace (predictor, joint, blank) with seeded weights wired for a realistic emission rate."""
    import types
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    torch.manual_seed(seed)
    pred = RNNPredictor(V, E, P, 0.1, H, layers, True, "lstm", 0.1).eval()
    joint = TransducerJoint(V, D, P, J, True, False, "add", "tanh").eval()
    with torch.no_grad():
        u = torch.sign(joint.ffn_out.weight[0])
        r = pred.rnn
        for l in range(layers):
            wih, whh = getattr(r, f"weight_ih_l{l}"), getattr(r, f"weight_hh_l{l}")
            bih, bhh = getattr(r, f"bias_ih_l{l}"), getattr(r, f"bias_hh_l{l}")
            for gate, b in ((0, 10.0), (1, -10.0), (3, 10.0)):     # unit 0: memoryless, gates open
                wih[gate * H] = 0.0
                bih[gate * H] = b
            for gate in range(4):
                whh[gate * H] = 0.0
                bhh[gate * H] = 0.0
            if l > 0:                                              # unit 0 reads unit 0 of the layer below
                wih[2 * H] = 0.0
                wih[2 * H, 0] = kappa
                bih[2 * H] = 0.0
        g = torch.Generator().manual_seed(seed)                    # embedding dimension 0: > 0 for every token but blank
        pred.embed.weight[:, 0] = 1.5 * (torch.rand(V, generator=g) * 0.8 + 0.2)
        pred.embed.weight[0, 0] = -1.5
        r.weight_ih_l0[2 * H] = 0.0                                # unit 0 of layer 0 reads it
        r.weight_ih_l0[2 * H, 0] = 1.0
        r.bias_ih_l0[2 * H] = 0.0
        pred.projection.weight[0] = 0.0
        pred.projection.weight[0, 0] = 1.0
        pred.projection.bias[0] = 0.0
        joint.pred_ffn.weight[:, 0] = beta * u
        joint.enc_ffn.weight[:, 0] = drive * u
    return types.SimpleNamespace(predictor=pred, joint=joint, blank=0)


def make_batch(B, T, D=512, seed=0, lo=-4.5, hi=1.0, zero_row=False):
    """(B, T, D) encoder output with ragged lengths (the longest = T) and the per-frame blank drive in dimension 0."""
    g = torch.Generator().manual_seed(1000 + seed)
    enc = torch.randn(B, T, D, generator=g)
    enc[:, :, 0] = torch.rand(B, T, generator=g) * (hi - lo) + lo
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    lens[0] = T
    if zero_row:
        lens[B - 1] = 0
    return enc, lens


def to(model, device, dtype):
    model.predictor.to(device=device, dtype=dtype)
    model.joint.to(device=device, dtype=dtype)
    return model


def kernel_call(model, enc, lens, n_steps=64):
    return hip_ops.rnnt_greedy_search(model.predictor, model.joint, enc, lens, model.blank, n_steps)


def count_steps(tokens, frames, lens, n_steps):
    """Decisions of the longest utterance (= lockstep steps needed): tokens + frames that ended in blank."""
    best = 0
    for tk, fr, T in zip(tokens, frames, lens):
        per = {}
        for f in fr:
            per[f] = per.get(f, 0) + 1
        best = max(best, len(tk) + T - sum(1 for c in per.values() if c >= n_steps))
    return best


def host_reads(steps, T, chunk=hip_ops.RNNT_GREEDY_CHUNK):
    return 2 + (max(0, steps - T) + chunk - 1) // chunk


def bench(name, B, T, dtype, steps, warmup, seed, basic):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import basic_greedy_search
    model = to(make_model(seed=seed), "cuda", dtype)
    enc, lens = make_batch(B, T, seed=seed)
    enc, lens_d = enc.to("cuda", dtype), lens.cuda()
    with torch.no_grad():
        for _ in range(warmup):
            kernel_call(model, enc, lens_d)
        torch.cuda.synchronize()
        times = []
        for _ in range(steps):
            t0 = time.perf_counter()
            toks, frames, scores = kernel_call(model, enc, lens_d)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(times)
        lens_h = lens.tolist()
        nsteps = count_steps(toks, frames, lens_h, 64)
        res = dict(config=name, B=B, T=T, dtype=str(dtype).replace("torch.", ""), kernel_ms=round(ms, 3),
                   audio_sec_per_sec=round(sum(lens_h) * FRAME_SEC / (ms / 1e3), 1),
                   tokens_per_frame=round(sum(len(t) for t in toks) / max(1, sum(lens_h)), 3),
                   steps=T + ((max(0, nsteps - T) + hip_ops.RNNT_GREEDY_CHUNK - 1) // hip_ops.RNNT_GREEDY_CHUNK)
                   * hip_ops.RNNT_GREEDY_CHUNK, decisions_longest=nsteps, host_reads=host_reads(nsteps, T))
        if basic:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = [basic_greedy_search(model, enc[b:b + 1], lens_h[b], 64)[0] for b in range(B)]
            torch.cuda.synchronize()
            res["basic_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            res["speedup"] = round(res["basic_ms"] / ms, 1)
            res["same_tokens"] = sum(int(a == b) for a, b in zip(toks, ref))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-basic", action="store_true")
    a = ap.parse_args()
    out = []
    for dt in (torch.float32, torch.bfloat16):
        out.append(bench("c5", 8, 250, dt, a.steps, a.warmup, a.seed, not a.no_basic))
        out.append(bench("b64", 64, 250, dt, a.steps, a.warmup, a.seed, False))
    print(json.dumps(dict(bench="rnnt_greedy", results=out)))


if __name__ == "__main__":
    main()
