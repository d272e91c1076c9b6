"""Cost of context biasing and time stamps in the GPU CTC prefix beam search, on the decode tail's CTC shape
(tools/bench_decode.py: B = 8, T' <= 250, V = 5000, beam 8).  Times one call of
  * the old entry point (pafc_ctc_prefix_beam_search: tokens and scores),
  * the new one without a graph (pafc_ctc_prefix_beam_search_ex: + time stamps),
  * the new one with graphs of 100 / 1 000 / 10 000 phrases (1-6 tokens, shared prefixes, suffix overlaps),
each from the same top-k tensors (the topk itself is not timed), plus the whole ctc_prefix_beam_search call with the
1 000-phrase graph.  Synthetic posteriors with phrases planted just below a decoy, so the graph changes the beams.
Prints one JSON line.  Kernel-only times: run under rocprofv3 --kernel-trace --stats."""
import argparse, json, os, random, sys, tempfile
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paper_accurate_fast_cheap_amd import _lib                                  # noqa: E402
from paper_accurate_fast_cheap_amd.hip_ops import ctc_prefix_beam              # noqa: E402
from paper_accurate_fast_cheap_amd.transformer import search as S               # noqa: E402
from paper_accurate_fast_cheap_amd.utils.context_graph import ContextGraph       # noqa: E402

B, T, V, beam = 8, 250, 5000, 8
LENS = [250, 240, 231, 200, 180, 150, 120, 100]


def phrases_for(n, seed):
    rng = random.Random(seed)
    ids = rng.sample(range(1, V), 1500)
    out = []
    for _ in range(n):
        r = rng.random()
        if out and r < 0.3:
            base = rng.choice(out)
            p = base[:rng.randint(1, len(base))] + [rng.choice(ids) for _ in range(rng.randint(0, 3))]
        elif out and r < 0.5:
            base = rng.choice(out)
            p = base[rng.randint(0, len(base) - 1):] + [rng.choice(ids) for _ in range(rng.randint(0, 2))]
        else:
            p = [rng.choice(ids) for _ in range(rng.randint(1, 6))]
        out.append(p[:6])
    return out


def graph_of(phrases, tmp):
    path = os.path.join(tmp, f"phrases_{len(phrases)}.txt")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join("".join(chr(0x4E00 + t) for t in p) for p in phrases) + "\n")
    return ContextGraph(path, {chr(0x4E00 + i): i for i in range(V)}, None, context_score=3.0)


def logp_with(phrases, seed=1):
    g = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)
    logits = torch.randn(B, T, V, generator=g)
    for b in range(B):
        t = 0
        while t < T:
            k = rng.random()
            if k < 0.3:
                n = rng.randint(1, 3); logits[b, t:t + n, 0] += 8.0; t += n
            elif k < 0.6:
                u, n = rng.randrange(1, V), rng.randint(1, 3); logits[b, t:t + n, u] += 8.0; t += n
            else:
                for tok in rng.choice(phrases):
                    if t + 3 > T:
                        break
                    logits[b, t:t + 2, rng.randrange(1, V)] += 8.0
                    logits[b, t:t + 2, tok] += 8.0 - rng.uniform(0.2, 2.0)
                    logits[b, t + 2, 0] += 6.0
                    t += 3
    return logits.log_softmax(-1)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters * 1e3, 1)       # microseconds per call


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        graphs = {n: graph_of(phrases_for(n, n), tmp) for n in (100, 1000, 10000)}
    logp = logp_with(graphs[1000].context_list).to(dev)
    lens = torch.tensor(LENS, device=dev)
    top_p, top_i = logp.topk(beam, dim=-1)
    top_p, top_i = top_p.contiguous(), top_i.contiguous()
    idx32, lens64 = top_i.to(torch.int32), lens.to(torch.int64)

    L = _lib.lib()
    nws = L.pafc_ctc_prefix_beam_workspace_bytes(B, T, beam)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    toks = torch.empty(B, beam, T, dtype=torch.int32, device=dev)
    ln = torch.empty(B, beam, dtype=torch.int32, device=dev)
    sc = torch.empty(B, beam, dtype=torch.float64, device=dev)
    stream = _lib.stream_of(top_p)

    def old():
        _lib.check(L.pafc_ctc_prefix_beam_search(B, T, beam, _lib.ptr(top_p), _lib.ptr(idx32), _lib.ptr(lens64), beam, 0,
                                                 _lib.ptr(toks), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(ws), nws, stream),
                   "pafc_ctc_prefix_beam_search")

    out = {"workload": f"CTC prefix beam: B={B}, T'<={T}, V={V}, beam {beam}; us per call (launch + kernel, no topk)",
           "old_entry_us": timed(old, args.iters, args.warmup),
           "ex_no_graph_no_times_us": timed(lambda: ctc_prefix_beam(top_p, top_i, lens, beam, 0, None, False),
                                            args.iters, args.warmup),
           "ex_no_graph_us": timed(lambda: ctc_prefix_beam(top_p, top_i, lens, beam, 0, None, True),
                                   args.iters, args.warmup)}
    for n, g in graphs.items():
        tab = g.device_tables(dev)
        out[f"ex_graph_{n}_us"] = timed(lambda: ctc_prefix_beam(top_p, top_i, lens, beam, 0, tab, True),
                                        args.iters, args.warmup)
        out[f"graph_{n}_nodes"] = int(tab["fail"].numel())
    out["search_no_graph_us"] = timed(lambda: S.ctc_prefix_beam_search(logp, lens, beam), 10, 2)
    out["search_graph_1000_us"] = timed(lambda: S.ctc_prefix_beam_search(logp, lens, beam, graphs[1000]), 10, 2)
    plain = S.ctc_prefix_beam_search(logp, lens, beam)
    biased = S.ctc_prefix_beam_search(logp, lens, beam, graphs[1000])
    out["graph_1000_changes_1best"] = sum(a.tokens != b.tokens for a, b in zip(plain, biased))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
