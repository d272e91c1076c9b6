"""Streaming CTC-fused RNN-T prefix beam search (BeamStreamer on hip_ops.RnntBeamStream: pafc_rnnt_beam_stream_* and
pafc_rnnt_beam_select_state) at the shipped uni transducer's decoder shape (D = 512, LSTM 2 x 640, join 640, V = 5000),
beam 8.  Prints one JSON line.

    python tools/bench_rnnt_beam_stream.py [--steps K] [--warmup W] [--chunks N] [--offline-frames T]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_rnnt_beam_stream.py --trace-frames

Per configuration (1, 8 and 64 streams, 16 encoder frames = 0.64 s per chunk, fp32): ms per chunk (median over the chunks of
K timed passes over the stream), whether the frame body replayed a captured graph, and the bytes of the one host read.
Then, for B = 8, the sum of the feeds over --offline-frames (250) frames next to the offline rnnt_beam_search
(PrefixBeamSearch._decode_batch_resident) of the same frames.  The model is tools/bench_rnnt_greedy.make_model with a
seeded linear CTC head.  Launches per frame come from a separate run under the profiler: --trace-frames feeds one warm
chunk, then 4 chunks of 16 frames for 8 streams and prints the frame count; divide the profiler's kernel count of that run,
less the count of a run with --trace-frames --chunks 0, by it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bench_rnnt_greedy as BG  # noqa: E402
from paper_accurate_fast_cheap_amd.transducer.search.prefix_beam_search import BeamStreamer, PrefixBeamSearch  # noqa: E402

CHUNK = 16
BEAM = 8
FRAME_SEC = 0.04
WEIGHTS = dict(ctc_weight=0.3, transducer_weight=0.7)


def make(B, T, dtype=torch.float32, seed=1):
    model = BG.to(BG.make_model(seed=0), "cuda", dtype)
    enc, _ = BG.make_batch(B, T, seed=seed)
    enc = enc.to("cuda", dtype)
    torch.manual_seed(seed)
    head = torch.nn.Linear(enc.shape[2], 5000).to("cuda", dtype)
    with torch.no_grad():
        logp = head(enc).float().log_softmax(-1).to(dtype)
    bs = PrefixBeamSearch(None, model.predictor, model.joint, None, model.blank)
    return bs, enc, logp


def bench(B, nchunks, steps, warmup):
    T = nchunks * CHUNK
    bs, enc, logp = make(B, T)
    st = BeamStreamer(bs, B, CHUNK, BEAM, max_total_frames=T, **WEIGHTS)
    per = []
    for rep in range(warmup + steps):
        st.reset()
        for a in range(0, T, CHUNK):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.feed(enc[:, a:a + CHUNK], logp[:, a:a + CHUNK])
            torch.cuda.synchronize()
            if rep >= warmup:
                per.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(per)
    return dict(streams=B, beam=BEAM, ms_per_chunk=round(ms, 3), p90_ms_per_chunk=round(sorted(per)[int(0.9 * (len(per) - 1))], 3),
                ms_per_frame=round(ms / CHUNK, 4), graph=st.graphed, read_bytes_last_feed=st._gpu.last_read_bytes,
                x_real_time=round(CHUNK * FRAME_SEC * 1e3 / ms, 1))


def against_offline(B, T, steps):
    bs, enc, logp = make(B, T)
    lens = torch.full((B,), T, device="cuda")
    st = BeamStreamer(bs, B, CHUNK, BEAM, max_total_frames=T, **WEIGHTS)
    feeds, off = [], []
    for rep in range(1 + steps):
        st.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in range(0, T, CHUNK):
            st.feed(enc[:, a:a + CHUNK], logp[:, a:a + CHUNK])
        res = st.results()
        torch.cuda.synchronize()
        if rep:
            feeds.append((time.perf_counter() - t0) * 1e3)
    for rep in range(1 + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = bs._decode_batch_resident(enc, lens, logp, BEAM, WEIGHTS["ctc_weight"], WEIGHTS["transducer_weight"])
        torch.cuda.synchronize()
        if rep:
            off.append((time.perf_counter() - t0) * 1e3)
    same = all([list(n) for n in r.nbest] == [list(n) for n in o.nbest] and r.nbest_scores == o.nbest_scores
               for r, o in zip(res, ref))
    return dict(streams=B, frames=T, sum_of_feeds_ms=round(statistics.median(feeds), 2),
                offline_rnnt_beam_search_ms=round(statistics.median(off), 2), results_bit_equal=same)


def trace_frames(nchunks):
    bs, enc, logp = make(8, max(1, nchunks) * CHUNK)
    st = BeamStreamer(bs, 8, CHUNK, BEAM, max_total_frames=(nchunks + 1) * CHUNK, **WEIGHTS)
    st.feed(enc[:, :CHUNK], logp[:, :CHUNK])                   # warm: the capture and its warm-up frames
    for c in range(nchunks):
        st.feed(enc[:, c * CHUNK:(c + 1) * CHUNK], logp[:, c * CHUNK:(c + 1) * CHUNK])
    torch.cuda.synchronize()
    return dict(bench="rnnt_beam_stream_trace", streams=8, traced_frames=nchunks * CHUNK, graph=st.graphed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunks", type=int, default=None)
    ap.add_argument("--offline-frames", type=int, default=250)
    ap.add_argument("--trace-frames", action="store_true")
    a = ap.parse_args()
    with torch.no_grad():
        if a.trace_frames:
            print(json.dumps(trace_frames(4 if a.chunks is None else a.chunks)))
            return
        chunks = 10 if a.chunks is None else a.chunks
        out = dict(bench="rnnt_beam_stream", chunk_frames=CHUNK,
                   results=[bench(B, chunks, a.steps, a.warmup) for B in (1, 8, 64)],
                   against_offline=against_offline(8, a.offline_frames, a.steps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
