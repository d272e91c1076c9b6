"""CTC forced alignment on the GPU (pafc_ctc_align) at two shapes: the decode-tail batch of tools/bench_decode.py (B = 8,
T' = 250, V = 5000, 40 labels) and one long-form file (B = 1, T' = 45000 -- 30 minutes --, 5000 labels).  Per shape: ms per call
(kernel + the package's host wrapper, device synchronised), the share of the kernel's time spent in the serial backtrace (from
the kernel's own wall-clock stamps in the workspace), the packed back-pointer bytes, and the package's host path on the same
input for scale.  Synthetic peaky posteriors; prints one JSON line per shape.  No threshold anywhere."""
import json
import sys
import time

import torch

from paper_accurate_fast_cheap_amd import _lib, hip_ops
from paper_accurate_fast_cheap_amd.transformer import search as S


def make(B, T, V, L, lens, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn(B, T, V, device="cuda", generator=g)
    logits[:, :, 0] += 3.0
    ys = torch.randint(1, V, (B, L), device="cuda", generator=g)
    for b in range(B):                      # a +6 bump on each label in a frame of its own, evenly spaced over the utterance
        centres = ((torch.arange(L, device="cuda") + 0.5) * (lens[b] / L)).long()
        logits[b, centres, ys[b]] += 6.0
    return logits.log_softmax(-1), torch.tensor(lens, device="cuda"), ys, torch.full((B,), L, device="cuda")


def run(name, B, T, V, L, lens, n, host: bool):
    lp, hl, ys, yl = make(B, T, V, L, lens, 777)
    nws = _lib.lib().pafc_ctc_align_workspace_bytes(B, T, L)
    ws = torch.empty(nws, dtype=torch.uint8, device=lp.device)      # the tool's own: the kernel's stamps are read from it below
    out = hip_ops.ctc_align(lp, hl, ys, yl, 0, workspace=ws)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n):
        out = hip_ops.ctc_align(lp, hl, ys, yl, 0, workspace=ws)
    torch.cuda.synchronize()
    ms = (time.time() - t0) / n * 1e3
    stamps = ws[nws - 32 * B:nws].view(torch.int64).view(B, 4).cpu()
    fwd, back = (stamps[:, 1] - stamps[:, 0]).double(), (stamps[:, 2] - stamps[:, 1]).double()
    slow = int((fwd + back).argmax())       # the block that ends last sets the kernel's time
    rec = {"shape": name, "B": B, "T": T, "V": V, "labels": L, "ok": out[4].tolist() == [1] * B, "ms_per_call": round(ms, 3),
           "backtrace_share": round(float(back[slow] / (fwd[slow] + back[slow])), 3),
           "back_pointer_MB": round((nws - 32 * B) / 1e6, 2), "as_bytes_MB": round(B * T * (2 * L + 1) / 1e6, 2)}
    if host:
        lp_h, hl_h, ys_h, yl_h = lp.cpu(), hl.cpu(), ys.cpu(), yl.cpu()
        t0 = time.time()
        res, ali = S.ctc_forced_align(lp_h, hl_h, ys_h, yl_h, 0, return_alignment=True)
        rec["host_path_ms"] = round((time.time() - t0) * 1e3, 1)
        rec["host_same_alignment"] = bool(torch.equal(ali, out[0].cpu()))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    with torch.no_grad():
        run("decode tail", 8, 250, 5000, 40, [250, 240, 231, 200, 180, 150, 120, 100], 20, True)
        if "--no-long" not in sys.argv:
            run("long form", 1, 45000, 5000, 5000, [45000], 3, "--no-long-host" not in sys.argv)
