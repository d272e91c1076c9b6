"""The fused RNN-T joint + loss (hip_ops.rnnt_joint_loss) against the restated path on the same input, at the training shape:
32 utterances, T' uniform in [60, 499], U uniform in [0, 160], join_dim 640, V = 5000 (the paper's YAML).  Prints one JSON line.

    python tools/bench_rnnt_loss.py [--steps K] [--warmup W] [--no-restated] [--seed S]

fused_ms: forward + backward of the fused path (median of K timed calls); restated_ms: forward_optimized's arithmetic
(per-utterance join, host reads of the lengths, the (rows, V) joint output) + transducer.loss.transducer_loss(mean) and
their autograd under bf16 autocast, timed once; *_peak_bytes: peak allocated bytes beyond the inputs during one call;
launches: kernels of one fused call (torch.profiler); tflops: 4 products of 2 R J V flops (forward; backward's recomputed
logits, dH, dW) over fused_ms."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paper_accurate_fast_cheap_amd import hip_ops  # noqa: E402
from paper_accurate_fast_cheap_amd.transducer.loss import transducer_loss  # noqa: E402


def make_inputs(seed, B=32, J=640, V=5000):
    g = torch.Generator().manual_seed(seed)
    Ts = torch.randint(60, 500, (B,), generator=g).tolist()
    Us = torch.randint(0, 161, (B,), generator=g).tolist()
    Us[0] = 0
    T, Up1 = max(Ts), max(Us) + 1
    E = (torch.randn(B, T, J, generator=g) * 0.6).to(torch.bfloat16).cuda().requires_grad_(True)
    P = (torch.randn(B, Up1, J, generator=g) * 0.6).to(torch.bfloat16).cuda().requires_grad_(True)
    W = (torch.randn(V, J, generator=g) * 3.0 / J ** 0.5).cuda().requires_grad_(True)
    b = (torch.randn(V, generator=g) * 0.5).cuda().requires_grad_(True)
    ys = torch.zeros(B, max(Us), dtype=torch.int64)
    for n, u in enumerate(Us):
        ys[n, :u] = torch.randint(1, V, (u,), generator=g)
    return Ts, Us, E, P, W, b, torch.tensor(Ts).cuda(), ys.cuda(), torch.tensor(Us).cuda()


def fused_call(E, P, W, b, hl, ys, yl):
    for x in (E, P, W, b):
        x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        nll = hip_ops.rnnt_joint_loss(E, P, W, b, hl, ys, yl, 0)
    (nll.sum() / hl.sum()).backward()


def restated_call(E, P, W, b, hl, ys, yl):
    for x in (E, P, W, b):
        x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        rows = []
        for i in range(E.shape[0]):                  # TransducerJoint.forward_optimized after its pre-join projections
            e = E[i, :int(hl[i])].unsqueeze(1)
            d = P[i, :int(yl[i]) + 1].unsqueeze(0)
            rows.append((e + d).reshape(-1, E.shape[-1]))
        logits = torch.nn.functional.linear(torch.tanh(torch.cat(rows)), W, b)
        loss = transducer_loss(logits, ys.to(torch.int32), hl, yl, 0, reduction="mean")
    loss.backward()


def timed(fn, *a):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn(*a)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def peak_of(fn, *a):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(*a)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def count_launches(fn, *a):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(*a)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:                                   # (a profiler without device activity on this build)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-restated", action="store_true")
    args = ap.parse_args()
    Ts, Us, E, P, W, b, hl, ys, yl = make_inputs(args.seed)
    J, V = E.shape[-1], W.shape[0]
    R = sum(t * (u + 1) for t, u in zip(Ts, Us))
    inp = (E, P, W, b, hl, ys, yl)
    for _ in range(args.warmup):
        fused_call(*inp)
    torch.cuda.synchronize()
    ms = [timed(fused_call, *inp) for _ in range(args.steps)]
    fused_ms = statistics.median(ms)
    out = dict(metric="rnnt_joint_loss_fwd_bwd", B=len(Ts), R=R, J=J, V=V, fused_ms=round(fused_ms, 3),
               fused_ms_min=round(min(ms), 3), fused_peak_bytes=peak_of(fused_call, *inp),
               dense_fp32_logits_bytes=R * V * 4, launches=count_launches(fused_call, *inp),
               tflops=round(4 * 2.0 * R * J * V / (fused_ms * 1e-3) / 1e12, 1))
    if not args.no_restated:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out["restated_ms"] = round(timed(restated_call, *inp), 1)
        out["restated_peak_bytes"] = torch.cuda.max_memory_allocated() - base
        out["speedup"] = round(out["restated_ms"] / fused_ms, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
