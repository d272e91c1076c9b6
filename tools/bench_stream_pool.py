"""Independent audio streams out of a slot pool (utils.stream_pool.StreamPool) beside the lock-step AudioStreamer at the same
stream count: the 12-layer uni-directional encoder of tools/bench_streaming.py (causal conv k = 15, whole-model bf16), CTC
prefix beam search (beam 8, V = 5000), 16-frame chunks, 64 slots.  Prints one JSON line.

    python tools/bench_stream_pool.py [--slots 64] [--streams 128] [--phases 4] [--lockstep-feeds 40]

Arrivals are deterministic: `--streams` streams of 10-60 s (a fixed pseudo-random list), the first `slots` of them staggered
over the first ticks, every later one opened when a slot frees.  Every stream brings 0.64 s packets (10 240 samples); the
server loop polls `--phases` times per packet period and a stream's packets arrive at its own phase, so a feed names the
streams of one phase only and a step batches whichever of them completed a window.  --phases 1 is the aligned case (every live
stream in every feed).  Per run (eager and graph-replayed): ms per feed, steps per feed, mean rows per full-window step, the
share of padding rows, audio-sec/sec, the launches of the gather / scatter kernels per step (3 by construction: state + windows
in, state out, output rows out) and, with --profile, the kernel events torch.profiler sees in one eager feed.
The lock-step line feeds (slots, 10 240) packets to one AudioStreamer: every step full, the upper bound."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench as B  # noqa: E402
from paper_accurate_fast_cheap_amd.utils.audio_stream import AudioStreamer  # noqa: E402
from paper_accurate_fast_cheap_amd.utils.init_model import init_model  # noqa: E402
from paper_accurate_fast_cheap_amd.utils.stream_pool import StreamPool  # noqa: E402

CHUNK, PACKET, BEAM = 16, 10240, 8


def build_model(dev):
    torch.manual_seed(777)
    conf = B.encoder_conf()
    conf.update(selfattention_layer_type="rwkv_tmix60", rnn_att_direction="uni", causal=True, cnn_module_kernel=15)
    configs = dict(encoder="conformer", encoder_conf=conf, input_dim=80, output_dim=B.VOCAB, ctc="ctc",
                   ctc_conf={"ctc_blank_id": 0}, model_conf={}, dataset_conf={})

    class A:
        checkpoint = None
    model, _ = init_model(A(), configs)
    return model.eval().to(torch.bfloat16).to(dev)


def stream_lengths(n, seed=11):
    rng = random.Random(seed)
    return [int(rng.uniform(10.0, 60.0) * 16000) for _ in range(n)]


def serve(model, wave, slots, lengths, phases, use_graph):
    """The server loop; -> (per-feed (wall ms, streams), the pool, samples served, ms spent in close).  Stream i reads its
    audio from `wave` at its own offset."""
    pool = StreamPool(model, slots, CHUNK, "ctc_prefix_beam_search", beam_size=BEAM, use_graph=use_graph)
    S = wave.size(1)
    pending = list(enumerate(lengths))
    live = {}                               # sid -> [stream index, samples sent, phase]
    feeds, poll, closed_audio, close_ms = [], 0, 0, 0.0
    while pending or live:
        # staggered arrivals: two new streams per poll until the pool is full, then one per freed slot
        for _ in range(2):
            if pending and len(live) < slots:
                i, _n = pending.pop(0)
                live[pool.open()] = [i, 0, i % phases]
        due = [sid for sid, (_, _, ph) in live.items() if ph == poll % phases]
        if due:
            ns = [min(PACKET, lengths[live[sid][0]] - live[sid][1]) for sid in due]
            buf = torch.zeros(len(due), PACKET, device=wave.device)
            for r, (sid, n) in enumerate(zip(due, ns)):
                i, sent, _ = live[sid]
                a = (i * 48000 + sent) % (S - PACKET)
                buf[r, :n] = wave[0, a:a + n]
                live[sid][1] += n
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pool.feed(due, buf, ns)
            torch.cuda.synchronize()
            feeds.append(((time.perf_counter() - t0) * 1e3, len(due)))
            done = [sid for sid in due if live[sid][1] >= lengths[live[sid][0]]]
            if done:
                t0 = time.perf_counter()
                pool.close(done)
                torch.cuda.synchronize()
                close_ms += (time.perf_counter() - t0) * 1e3
                for sid in done:
                    closed_audio += lengths[live[sid][0]]
                    del live[sid]
        poll += 1
    return feeds, pool, closed_audio, close_ms


def summarise(feeds, pool, audio_samples, close_ms):
    log = pool.step_log
    window = pool.sched.window
    full = [r for r in log if not r["first"] and r["rows"][0][2] == window]
    rows = sum(len(r["rows"]) for r in full)
    padded = sum(r["batch"] for r in full)
    wall = [f[0] for f in feeds]
    total_s = (sum(wall) + close_ms) / 1e3                   # feeds and closes: everything the streams cost
    return dict(feeds=len(feeds), mean_streams_per_feed=round(statistics.mean(f[1] for f in feeds), 2),
                ms_per_feed_median=round(statistics.median(wall), 3), ms_per_feed_mean=round(statistics.mean(wall), 3),
                ms_per_feed_p90=round(sorted(wall)[int(0.9 * (len(wall) - 1))], 3),
                steps=len(log), full_window_steps=len(full), steps_per_feed=round(len(log) / len(feeds), 3),
                mean_rows_per_full_step=round(rows / max(len(full), 1), 2),
                padding_row_share=round(1.0 - rows / max(padded, 1), 4),
                replayed_steps=sum(r["replayed"] for r in log), in_place_steps=sum(r["in_place"] for r in log),
                audio_sec_per_sec=round(audio_samples / 16000.0 / total_s, 1),
                gather_scatter_launches_per_step=3)


def eager_step_launches(model, wave, slots):
    """Kernel launches of one eager full-window step of `slots` rows, by the profiler; None where it reports no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        pool = StreamPool(model, slots, CHUNK, "ctc_prefix_beam_search", beam_size=BEAM, use_graph=False)
        sids = [pool.open() for _ in range(slots)]
        buf = wave[:, :slots * 4 + 3 * PACKET].unfold(1, 3 * PACKET, 4)[0, :slots].contiguous()
        pool.feed(sids, buf)                                    # first windows (and the second of every stream)
        nxt = wave[:, 5 * PACKET:5 * PACKET + slots * 4 + PACKET].unfold(1, PACKET, 4)[0, :slots].contiguous()
        before = len(pool.step_log)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            pool.feed(sids, nxt)
            torch.cuda.synchronize()
        steps = len(pool.step_log) - before
        kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if not kernels or steps < 1:
            return None
        return dict(steps=steps, kernel_events_in_the_feed=len(kernels), note="the whole feed: fbank pair, the steps, the decoder")
    except Exception as e:                                       # the profiler is an optional extra of this bench
        return dict(error=f"{type(e).__name__}: {e}"[:200])


def lockstep(model, wave, slots, feeds):
    st = AudioStreamer(model, slots, CHUNK, "ctc_prefix_beam_search", beam_size=BEAM)
    wall = []
    for k in range(feeds + 4):
        buf = wave[:, k * PACKET:k * PACKET + slots * 4 + PACKET].unfold(1, PACKET, 4)[0, :slots].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.feed(buf)
        torch.cuda.synchronize()
        if k >= 4:                                               # (the first feeds bind, allocate and warm up)
            wall.append((time.perf_counter() - t0) * 1e3)
    return dict(streams=slots, feeds=len(wall), ms_per_feed_median=round(statistics.median(wall), 3),
                ms_per_feed_mean=round(statistics.mean(wall), 3),
                audio_sec_per_sec=round(slots * PACKET / 16000.0 / (statistics.mean(wall) / 1e3), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--phases", type=int, nargs="*", default=[4, 1])
    ap.add_argument("--lockstep-feeds", type=int, default=40)
    ap.add_argument("--profile", action="store_true", help="also count the kernel events of one eager feed with torch.profiler")
    a = ap.parse_args()
    dev = torch.device("cuda")
    model = build_model(dev)
    wave = B.synthetic_waveform(120.0, 777).to(dev)
    lengths = stream_lengths(a.streams)
    out = dict(bench="stream_pool", slots=a.slots, streams=a.streams, chunk_frames=CHUNK, packet_samples=PACKET, beam=BEAM,
               vocab=B.VOCAB, stream_seconds=[round(min(lengths) / 16000, 1), round(max(lengths) / 16000, 1)], runs=[])
    with torch.no_grad():
        serve(model, wave, min(a.slots, 8), lengths[:8], 1, False)          # warm: binding, tables, plans
        for phases in a.phases:
            for use_graph in (False, True):
                feeds, pool, audio, close_ms = serve(model, wave, a.slots, lengths, phases, use_graph)
                res = summarise(feeds, pool, audio, close_ms)
                res.update(phases=phases, use_graph=use_graph)
                out["runs"].append(res)
        out["lockstep_audio_streamer"] = lockstep(model, wave, a.slots, a.lockstep_feeds)
        out["launches_per_step"] = eager_step_launches(model, wave, a.slots) if a.profile else "not measured"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
