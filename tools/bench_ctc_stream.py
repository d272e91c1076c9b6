"""Streaming CTC prefix beam search (search.CtcStreamer on hip_ops.CtcBeamStream: pafc_ctc_beam_stream_*) at the decode
tail's CTC shape: 16-frame chunks (0.64 s), V = 5000, beam 8, 1 / 8 / 64 streams, with and without the 1 000-phrase graph of
tools/bench_ctc_context.py.  Prints one JSON line.

    python tools/bench_ctc_stream.py [--repeats R] [--long-frames N]
    rocprofv3 --kernel-trace --stats -- python tools/bench_ctc_stream.py --profile-run     (kernel times, a run of its own)

Per configuration, over a stream of 250 frames: wall ms per chunk of CtcStreamer.feed (topk of the chunk, the copies into
the fixed buffers, feed kernel, drain kernel, the host read and the Python that builds the partial results), the device
time of feed + drain kernels per chunk (events around the two launches), bytes read by the host per chunk, and the sum of
the feed launches over the stream against one offline call (hip_ops.ctc_prefix_beam) on the same frames.  Then a stream of
--long-frames frames (the 250-frame block repeated): wall ms, drain device time and bytes per chunk around frame 250 and at
the end, each as the median over the repeats with the repeats' min .. max -- the `from` offset's claim is that these do not
grow with the stream.  --profile-run streams B = 8 once with and once without the graph and calls the offline kernel once
on the same frames, nothing else, so that a kernel trace holds exactly the launches to compare."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bench_ctc_context as BC  # noqa: E402
from paper_accurate_fast_cheap_amd import hip_ops  # noqa: E402
from paper_accurate_fast_cheap_amd.transformer.search import CtcStreamer  # noqa: E402

CHUNK, V, BEAM, BLOCK = 16, BC.V, BC.beam, 250


def logp_block(B, phrases, seed=1):
    """bench_ctc_context.logp_with for B streams of BLOCK frames: blank runs, repeats, phrases planted below a decoy."""
    g = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)
    logits = torch.randn(B, BLOCK, V, generator=g)
    for b in range(B):
        t = 0
        while t < BLOCK:
            k = rng.random()
            if k < 0.3:
                n = rng.randint(1, 3); logits[b, t:t + n, 0] += 8.0; t += n
            elif k < 0.6:
                u, n = rng.randrange(1, V), rng.randint(1, 3); logits[b, t:t + n, u] += 8.0; t += n
            else:
                for tok in rng.choice(phrases):
                    if t + 3 > BLOCK:
                        break
                    logits[b, t:t + 2, rng.randrange(1, V)] += 8.0
                    logits[b, t:t + 2, tok] += 8.0 - rng.uniform(0.2, 2.0)
                    logits[b, t + 2, 0] += 6.0
                    t += 3
    return logits.log_softmax(-1)


def chunk_at(logp, a):
    """Frames [a, a + CHUNK) of the endless stream that repeats the block."""
    idx = torch.arange(a, a + CHUNK, device=logp.device) % BLOCK
    return logp.index_select(1, idx)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def run_stream(logp, graph, frames):
    """One stream of `frames` frames through CtcStreamer; per chunk (wall ms, bytes read, committed tokens of row 0)."""
    B = logp.shape[0]
    s = CtcStreamer(B, CHUNK, "ctc_prefix_beam_search", BEAM, graph, 0, max_total_frames=frames + CHUNK)
    rows = []
    for a in range(0, frames, CHUNK):
        x = chunk_at(logp, a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.feed(x)
        torch.cuda.synchronize()
        rows.append(((time.perf_counter() - t0) * 1e3, s.last_read_bytes, len(s.committed[0])))
    return rows, s


def kernel_times(logp, graph, frames):
    """Device us per chunk of the feed launch and of the drain launch (events), on hip_ops.CtcBeamStream directly, the
    drain from the committed count as CtcStreamer does it."""
    B = logp.shape[0]
    tables = None if graph is None else graph.device_tables(logp.device)
    st = hip_ops.CtcBeamStream(B, CHUNK, BEAM, BEAM, logp.device, 0, tables, frames + CHUNK)
    counts, tail, out = [0] * B, 0, []
    for a in range(0, frames, CHUNK):
        tp, ti = chunk_at(logp, a).topk(BEAM, dim=-1)
        st.load(tp, ti)
        e0, e1 = events()
        e0.record(); st.launch_feed(); e1.record()
        torch.cuda.synchronize()
        feed_us = e0.elapsed_time(e1) * 1e3
        # (drain allocates its output and reads it: time the launch alone through a second, throw-away call)
        d = st.drain(counts, tail + CHUNK)
        e0, e1 = events()
        buf = torch.empty(B * BEAM * (12 + 4 * (tail + CHUNK)) + 12 * B, dtype=torch.uint8, device=logp.device)
        o = [0, B * BEAM * 8]
        for words in (B * BEAM, B, B, B, B * BEAM * (tail + CHUNK)):
            o.append(o[-1] + 4 * words)
        e0.record(); st._drain(buf, o, tail + CHUNK, 0, None, None); e1.record()
        torch.cuda.synchronize()
        out.append((feed_us, e0.elapsed_time(e1) * 1e3))
        counts = d["committed"]
        tail = max(max(l for l in d["len"][b] if l >= 0) - counts[b] for b in range(B))
    return out


def offline_us(logp, graph, iters=20):
    tables = None if graph is None else graph.device_tables(logp.device)
    tp, ti = logp.topk(BEAM, dim=-1)
    tp, ti = tp.contiguous(), ti.contiguous()
    return BC.timed(lambda: hip_ops.ctc_prefix_beam(tp, ti, None, BEAM, 0, tables, True), iters, 3)


def med_spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def config(B, graph, phrases, repeats, long_frames):
    logp = logp_block(B, phrases).cuda()
    run_stream(logp, graph, BLOCK)                                       # warm: binding, allocator, device tables
    short = [run_stream(logp, graph, BLOCK)[0] for _ in range(repeats)]
    wall = [r[0] for rows in short for r in rows]
    kt = kernel_times(logp, graph, BLOCK)
    res = dict(streams=B, graph=graph is not None,
               wall_ms_per_chunk=round(statistics.median(wall), 3), p90_wall_ms_per_chunk=round(sorted(wall)[int(0.9 * (len(wall) - 1))], 3),
               feed_us_per_chunk=round(statistics.median(k[0] for k in kt), 1),
               drain_us_per_chunk=round(statistics.median(k[1] for k in kt), 1),
               bytes_read_per_chunk=round(statistics.mean(r[1] for r in short[0])), max_bytes_read=max(r[1] for r in short[0]),
               sum_feed_us_250_frames=round(sum(k[0] for k in kt), 1), offline_us_250_frames=offline_us(logp, graph))
    res["feed_sum_over_offline"] = round(res["sum_feed_us_250_frames"] / res["offline_us_250_frames"], 2)
    if long_frames:
        near = lambda rows, f: rows[max(0, f // CHUNK - 6):f // CHUNK + 4]    # ten chunks around frame f
        longs = [run_stream(logp, graph, long_frames)[0] for _ in range(repeats)]
        klong = [kernel_times(logp, graph, long_frames) for _ in range(repeats)]
        for name, f in (("at_250", BLOCK), ("at_end", long_frames - 4 * CHUNK)):
            res[name] = dict(frame=f,
                             wall_ms=med_spread([statistics.median(r[0] for r in near(rows, f)) for rows in longs]),
                             drain_us=med_spread([statistics.median(k[1] for k in near(k_, f)) for k_ in klong]),
                             feed_us=med_spread([statistics.median(k[0] for k in near(k_, f)) for k_ in klong]),
                             bytes_read=med_spread([statistics.mean(r[1] for r in near(rows, f)) for rows in longs]),
                             committed_tokens_row0=near(longs[0], f)[-1][2])
    return res


def profile_run(phrases, graph):
    logp = logp_block(8, phrases).cuda()
    for g in (None, graph):
        run_stream(logp, g, BLOCK)
        tables = None if g is None else g.device_tables(logp.device)
        tp, ti = logp.topk(BEAM, dim=-1)
        hip_ops.ctc_prefix_beam(tp.contiguous(), ti.contiguous(), None, BEAM, 0, tables, True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--long-frames", type=int, default=4000)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    phrases = BC.phrases_for(1000, 1000)
    with tempfile.TemporaryDirectory() as tmp:
        graph = BC.graph_of(phrases, tmp)
    if a.profile_run:
        profile_run(phrases, graph)
        return
    out = dict(bench="ctc_beam_stream", chunk_frames=CHUNK, beam=BEAM, vocab=V, long_frames=a.long_frames, repeats=a.repeats,
               results=[config(B, g, phrases, a.repeats, a.long_frames) for B in a.streams for g in (None, graph)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
