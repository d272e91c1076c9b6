"""Streaming RNN-T greedy search (hip_ops.RnntGreedyStream: pafc_rnnt_greedy_stream_* + the lockstep step kernels) at the
shipped uni transducer's decoder shape (D = 512, LSTM 2 x 640, join 640, V = 5000).  Prints one JSON line.

    python tools/bench_rnnt_stream.py [--steps K] [--warmup W] [--seconds S] [--no-encoder]

Per configuration (1, 8 and 64 streams, 16 encoder frames = 0.64 s per chunk, fp32 and bf16): the decoder's ms per chunk
(median over the chunks of K timed passes over the stream), lockstep steps and host reads per chunk, whether the fixed part of
a feed replayed a captured graph, the emission rate, and the same frames through the offline rnnt_greedy_search (ms per
chunk's worth of audio).  The model is tools/bench_rnnt_greedy.make_model; the per-frame blank drive's lower bound is
calibrated once (offline decode, fp32) so the emission rate lands near a trained model's 0.1-0.5 tokens per frame.  Then
encoder + decoder per chunk for one stream at tools/bench_streaming.py's setup (12-layer uni encoder, causal conv, bf16,
forward_chunk_carry per window) and the real-time factor."""
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
from paper_accurate_fast_cheap_amd import hip_ops  # noqa: E402

CHUNK = 16
FRAME_SEC = 0.04


def calibrate(T=160, target=0.3):
    """The lower bound of the blank drive whose offline decode emits closest to `target` tokens per frame."""
    model = BG.to(BG.make_model(seed=0), "cuda", torch.float32)
    best = None
    for i in range(21):
        lo = -4.5 + 0.1 * i
        enc, lens = BG.make_batch(8, T, seed=0, lo=lo)
        with torch.no_grad():
            toks, _, _ = BG.kernel_call(model, enc.cuda(), lens.cuda())
        rate = sum(len(t) for t in toks) / float(lens.sum())
        if best is None or abs(rate - target) < abs(best[1] - target):
            best = (lo, rate)
    return best


def bench(B, dtype, lo, nchunks, steps, warmup):
    model = BG.to(BG.make_model(seed=0), "cuda", dtype)
    T = nchunks * CHUNK
    enc, _ = BG.make_batch(B, T, seed=1, lo=lo)
    enc = enc.to("cuda", dtype)
    st = hip_ops.RnntGreedyStream(model.predictor, model.joint, B, CHUNK)
    per, nsteps, reads, ntok = [], [], [], 0
    with torch.no_grad():
        for rep in range(warmup + steps):
            st.reset()
            for a in range(0, T, CHUNK):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks, frames = st.feed(enc[:, a:a + CHUNK])
                torch.cuda.synchronize()
                if rep >= warmup:
                    per.append((time.perf_counter() - t0) * 1e3)
                    nsteps.append(st.last_steps)
                    reads.append(2 + (st.last_steps - CHUNK) // hip_ops.RNNT_GREEDY_CHUNK)
                    ntok += sum(len(t) for t in toks)
        lens = torch.full((B,), T, device="cuda")
        off = []
        for _ in range(max(1, steps)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            BG.kernel_call(model, enc, lens)
            torch.cuda.synchronize()
            off.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(per)
    return dict(streams=B, dtype=str(dtype).replace("torch.", ""), decoder_ms_per_chunk=round(ms, 3),
                p90_ms_per_chunk=round(sorted(per)[int(0.9 * (len(per) - 1))], 3),
                steps_per_chunk=round(statistics.mean(nsteps), 1), max_steps_per_chunk=max(nsteps),
                host_reads_per_chunk=round(statistics.mean(reads), 2), graph=st.graphed,
                tokens_per_frame=round(ntok / float(B * T * steps), 3),
                offline_ms_same_frames=round(statistics.median(off), 2),
                offline_ms_per_chunk_of_audio=round(statistics.median(off) / nchunks, 3),
                x_real_time_decoder=round(CHUNK * FRAME_SEC * 1e3 / ms, 1))


def encoder_plus_decoder(lo, seconds, steps):
    """bench_streaming.py's model (12 x 512 uni encoder, causal conv k = 15, bf16), one stream, 16-frame chunks: the
    encoder's forward_chunk_carry per window, its output frames into the streamer."""
    import bench as Bn
    from paper_accurate_fast_cheap_amd.utils.graph_step import chunk_windows
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    torch.manual_seed(777)
    conf = Bn.encoder_conf()
    conf.update(selfattention_layer_type="rwkv_tmix60", rnn_att_direction="uni", causal=True, cnn_module_kernel=15)
    configs = dict(encoder="conformer", encoder_conf=conf, input_dim=80, output_dim=Bn.VOCAB, ctc="ctc",
                   ctc_conf={"ctc_blank_id": 0}, model_conf={}, dataset_conf={})

    class A:
        checkpoint = None

    asr, _ = init_model(A(), configs)
    enc = asr.encoder.eval().to(torch.bfloat16).cuda()
    feats, _ = Bn.front_end(Bn.synthetic_waveform(seconds, 777), torch.device("cuda"))
    feats = feats.to(torch.bfloat16)
    dec = BG.to(BG.make_model(seed=0, D=enc.output_size()), "cuda", torch.bfloat16)
    st = hip_ops.RnntGreedyStream(dec.predictor, dec.joint, 1, CHUNK)
    T = feats.shape[1]
    starts, window, _ = chunk_windows(enc.embed, CHUNK, T)
    res = []
    with torch.no_grad():
        for rep in range(1 + steps):
            st.reset()
            state, e_ms, d_ms = None, 0.0, 0.0
            torch.cuda.synchronize()
            for c in starts:
                t0 = time.perf_counter()
                y, state = enc.forward_chunk_carry(feats[:, c:min(c + window, T)], 0, state)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                st.feed(y)
                torch.cuda.synchronize()
                e_ms += (t1 - t0) * 1e3
                d_ms += (time.perf_counter() - t1) * 1e3
            if rep:
                res.append((e_ms / len(starts), d_ms / len(starts)))
    e, d = statistics.median(r[0] for r in res), statistics.median(r[1] for r in res)
    return dict(seconds=seconds, chunks=len(starts), encoder_ms_per_chunk=round(e, 3), decoder_ms_per_chunk=round(d, 3),
                total_ms_per_chunk=round(e + d, 3), x_real_time=round(CHUNK * FRAME_SEC * 1e3 / (e + d), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--no-encoder", action="store_true")
    a = ap.parse_args()
    lo, rate = calibrate()
    out = dict(bench="rnnt_greedy_stream", chunk_frames=CHUNK, drive_lo=round(lo, 2), calibrated_tokens_per_frame=round(rate, 3),
               results=[bench(B, dt, lo, a.chunks, a.steps, a.warmup) for dt in (torch.float32, torch.bfloat16) for B in (1, 8, 64)])
    if not a.no_encoder:
        out["encoder_plus_decoder"] = encoder_plus_decoder(lo, a.seconds, a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
