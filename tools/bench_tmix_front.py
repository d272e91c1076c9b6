"""The three LDS-/register-resident kernels of the time-mix front end at the 30-minute shape (B 1, T 44 998, C 512, two
directions), plain loop (PAFC_TMIX_PIPE=0) against the loop with the next tile's loads in flight, alternating call by call in
one process; device events, median of 20 calls per form, three repeats.  One JSON line per kernel with the achieved TB/s on the
bytes the kernel must move; a kernel's spread is max - min of its plain-form medians over the repeats.

    python tools/bench_tmix_front.py [--out profiles/tmix_front_pipe_shapes.jsonl] [--waves 8|16]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paper_accurate_fast_cheap_amd import hip_ops  # noqa: E402

B, T, C, ND = 1, 44998, 512, 2
CALLS, REPEATS = 20, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--waves", default=None, help="PAFC_LORA_DOWN_WAVES for tmix_lora_down")
    args = ap.parse_args()
    if args.waves:
        os.environ["PAFC_LORA_DOWN_WAVES"] = args.waves
    bf, dev = torch.bfloat16, "cuda"
    rows = B * T
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s, scale=1.0: (torch.randn(s, device=dev, generator=g) * scale).to(bf)
    x, maa_x, w1n = rnd(B, T, C), rnd(ND, C, scale=0.5), rnd(ND, 128, C, scale=1.5 / C ** 0.5)
    w2t, maa = rnd(ND, 4, C, 32, scale=0.2), rnd(ND, 4, C, scale=0.5)
    d1n, d2n, td = rnd(ND, 64, C, scale=2 / C ** 0.5), rnd(ND, C, 64, scale=0.3), rnd(ND, C) - 3
    t = hip_ops.tmix_lora_down(x, maa_x, w1n, one_pass=True)
    zw = hip_ops.tmix_lora_mix4(x, t, w2t, maa)[3].contiguous()
    kernels = {
        "tmix_lora_down": (lambda: hip_ops.tmix_lora_down(x, maa_x, w1n, one_pass=True), rows * C * 2 + ND * rows * 128 * 2),
        "tmix_lora_mix4_ws": (lambda: hip_ops.tmix_lora_mix4(x, t, w2t, maa), rows * C * 2 + ND * rows * 128 * 2 + 4 * ND * rows * C * 2),
        "decay_lora": (lambda: hip_ops.decay_lora(zw, d1n, d2n, td, one_pass=True), 2 * ND * rows * C * 2),
    }
    forms = (("plain", "0"), ("pipe", "1"))
    lines = []
    for name, (run, nbytes) in kernels.items():
        outs = {}
        for form, v in forms:                    # warm up, and the two forms must agree bit for bit
            os.environ["PAFC_TMIX_PIPE"] = v
            for _ in range(3):
                outs[form] = run()
        torch.cuda.synchronize()
        assert torch.equal(outs["plain"], outs["pipe"]), name
        del outs
        med = {form: [] for form, _ in forms}
        for _ in range(REPEATS):
            ev = {form: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
                  for form, _ in forms}
            for i in range(CALLS):
                for form, v in forms:
                    os.environ["PAFC_TMIX_PIPE"] = v
                    ev[form][i][0].record()
                    run()
                    ev[form][i][1].record()
            torch.cuda.synchronize()
            for form, _ in forms:
                med[form].append(statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev[form]))
        rec = {"kernel": name, "shape": {"B": B, "T": T, "C": C, "ndir": ND}, "bytes": nbytes, "calls": CALLS,
               "plain_us_medians": [round(v, 2) for v in med["plain"]], "pipe_us_medians": [round(v, 2) for v in med["pipe"]],
               "plain_us": round(statistics.median(med["plain"]), 2), "pipe_us": round(statistics.median(med["pipe"]), 2),
               "plain_spread_us": round(max(med["plain"]) - min(med["plain"]), 2)}
        rec["plain_TBps"] = round(nbytes / rec["plain_us"] * 1e-6, 2)
        rec["pipe_TBps"] = round(nbytes / rec["pipe_us"] * 1e-6, 2)
        rec["gain_us"] = round(rec["plain_us"] - rec["pipe_us"], 2)
        rec["pays"] = bool(rec["gain_us"] > rec["plain_spread_us"])
        if args.waves:
            rec["PAFC_LORA_DOWN_WAVES"] = args.waves
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.environ.pop("PAFC_TMIX_PIPE", None)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
