"""Forward + backward of the Mamba-2 selective scan at a training shape, on its two differentiable routes:
  * ssd: hip_ops.mamba2_scan_train -- the SSD scan kernel and its backward kernel (csrc/mamba2_scan.hip, mamba2_scan_bwd.hip);
  * wkv: what Mamba2.forward does without the SSD kernel -- the fp32 operand planes (C, a B, dt x and the decay broadcast over
    heads / channels), two WKV-6 scans of 64 state dimensions each with the WKV-6 backward behind them, and the diagonal term;
both from the same xbc (bf16), dt and log a, with the gradient flowing back into those three.
Shapes: train = B 32, L 499, H 16 (d_model 512); chunked = B 1, L 3000, H 16 (the scans split the sequence into chunks).

    python tools/bench_mamba_train.py                    one JSON line of device-event times per (shape, route), us per fwd + bwd
    python tools/bench_mamba_train.py --profile          each (shape, route) in a child of its own under
                                                         rocprofv3 --kernel-trace: the median time of every kernel of the loop times
                                                         its launches per iteration, summed (all kernels, and the scan kernels alone)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"train": (32, 499, 16), "chunked": (1, 3000, 16)}
SCAN_KERNELS = ("mamba2_ssd", "wkv6")


def make_inputs(B, L, H):
    import torch
    g = torch.Generator().manual_seed(1)
    xbc = (torch.randn(B, L, H * 64 + 256, generator=g) * 0.5).to(torch.bfloat16).cuda().requires_grad_()
    dt = (torch.rand(B, L, H, generator=g) * 0.2 + 0.01).cuda().requires_grad_()
    la = (-dt.detach().cpu() * (torch.rand(H, generator=g) * 8 + 0.5)).cuda().requires_grad_()
    gy = torch.randn(B, L, H * 64, generator=g).cuda()
    return xbc, dt, la, gy


def ssd_route(xbc, dt, la, H):
    from paper_accurate_fast_cheap_amd import hip_ops
    return hip_ops.mamba2_scan_train(xbc, dt, la, H)


def wkv_route(xbc, dt, la, H):
    """The scan of Mamba2.forward's WKV-6 route (transformer/mamba2.py) on the kernel's operands."""
    import torch
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6
    Bsz, L, _ = xbc.shape
    d = H * 64
    x, Bm, Cm = xbc[..., :d], xbc[..., d:d + 128], xbc[..., d + 128:d + 256]
    nxt = torch.cat([la[:, 1:], torch.zeros_like(la[:, :1])], dim=1)
    a_next = torch.exp(nxt)
    w = torch.log((-nxt).clamp_min(1e-30))
    xf = x.float().view(Bsz, L, H, 64)
    v = (xf * dt.unsqueeze(-1)).reshape(Bsz, L, d).contiguous()
    wk = w.unsqueeze(-1).expand(Bsz, L, H, 64).reshape(Bsz, L, d).contiguous()
    u0 = torch.zeros(H, 64, dtype=torch.float32, device=xbc.device)
    y = torch.zeros(Bsz, L, d, dtype=torch.float32, device=xbc.device)
    for half in range(2):
        Bh, Ch = Bm[..., half * 64:(half + 1) * 64].float(), Cm[..., half * 64:(half + 1) * 64].float()
        k = (a_next.unsqueeze(-1) * Bh.unsqueeze(2)).reshape(Bsz, L, d).contiguous()
        r = Ch.unsqueeze(2).expand(Bsz, L, H, 64).reshape(Bsz, L, d).contiguous()
        y = y + wkv6(r, k, v, wk, u0)
        y = y + ((Bh * Ch).sum(-1, keepdim=True).unsqueeze(-1) * v.view(Bsz, L, H, 64)).reshape(Bsz, L, d)
    return y


ROUTES = {"ssd": ssd_route, "wkv": wkv_route}


def run(shape, route, iters, warmup):
    """us per forward + backward by device events (launches included)."""
    import torch
    B, L, H = SHAPES[shape]
    xbc, dt, la, gy = make_inputs(B, L, H)

    def step():
        for t in (xbc, dt, la):
            t.grad = None
        ROUTES[route](xbc, dt, la, H).backward(gy)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters * 1e3, 1)


def kernel_medians(trace_dir, steps):
    """{kernel name: (launches per step, median us)} of the kernels launched at least once per step."""
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (len(v) / steps, statistics.median(v)) for k, v in rows.items() if len(v) >= steps}


def profile(shape, route, iters, warmup, timeout):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--shape", shape, "--route", route, "--iters", str(iters), "--warmup", str(warmup)]
        subprocess.run(cmd, check=True, timeout=timeout, stdout=subprocess.DEVNULL)
        med = kernel_medians(tmp, iters + warmup)
    total = sum(n * us for n, us in med.values())
    scan = sum(n * us for k, (n, us) in med.items() if any(s in k for s in SCAN_KERNELS))
    short = lambda k: k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][-56:]
    top = sorted(((round(n * us, 1), short(k)) for k, (n, us) in med.items()), reverse=True)[:8]
    return {"kernels_us": round(total, 1), "scan_kernels_us": round(scan, 1), "launches": round(sum(n for n, _ in med.values()), 1),
            "top": top}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES) + ["both"], default="both")
    ap.add_argument("--route", choices=list(ROUTES) + ["both"], default="both")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="kernel-trace medians, each (shape, route) in a child under rocprofv3")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per profiled child")
    args = ap.parse_args(argv)
    shapes = list(SHAPES) if args.shape == "both" else [args.shape]
    routes = list(ROUTES) if args.route == "both" else [args.route]
    out = {"workload": "Mamba-2 scan forward + backward, us per step; (B, L, H): " + str({s: SHAPES[s] for s in shapes})}
    for s in shapes:
        for r in routes:
            out[f"{s}_{r}"] = (profile(s, r, args.iters, args.warmup, args.timeout) if args.profile
                               else {"events_us": run(s, r, args.iters, args.warmup)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
