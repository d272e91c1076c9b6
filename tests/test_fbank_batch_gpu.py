"""Batched and streaming fbank on the MI355X (pafc_fbank_batch / pafc_fbank_stream, dataset.fbank.fbank_batch / FbankStreamer).
The arithmetic is that of the single-waveform kernel, frame by frame, so the yardstick is exact: bit for bit fbank() of each
utterance, zeros behind a row's frames, and for any cut of a stream into packets the frames of fbank_batch of the whole."""
import random

import pytest
import torch

from oracle import fbank_oracle as FO
from tests import synth
from tests.test_fbank_gpu import _wave

pytestmark = pytest.mark.gpu

# 0, 0, 1, 1, 2, exactly 64 (one full tile), 65 (a second tile of one frame) and 199 frames (a ragged fourth tile)
LENGTHS = [0, 399, 400, 559, 560, 400 + 160 * 63, 400 + 160 * 64, 32123]
PAD = 12345.0           # what lies behind an utterance in its row: must never be read into a frame


def _frames(S):
    return 0 if S < 400 else 1 + (S - 400) // 160


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def ragged(hip):
    """One ragged batch and, per row, fbank() of the utterance alone (computed once, never written to)."""
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank
    S = max(LENGTHS)
    w = torch.full((len(LENGTHS), S), PAD)
    for b, n in enumerate(LENGTHS):
        w[b, :n] = _wave(n, 20 + b)[0]
    w = w.cuda()
    single = [fbank(w[b:b + 1, :n], num_mel_bins=80) for b, n in enumerate(LENGTHS)]
    whole = [fbank(w[b:b + 1], num_mel_bins=80) for b in range(len(LENGTHS))]
    return w, single, whole


def check_ragged(feats, flens, single):
    T = _frames(max(LENGTHS))
    assert feats.shape == (len(LENGTHS), T, 80) and flens.dtype == torch.int32 and flens.is_cuda
    assert flens.tolist() == [_frames(n) for n in LENGTHS]
    for b, n in enumerate(LENGTHS):
        m = _frames(n)
        assert same_bits(feats[b, :m], single[b]), f"row {b} ({n} samples)"
        assert torch.equal(_bits(feats[b, m:]), torch.zeros_like(_bits(feats[b, m:]))), f"row {b}: padding is not +0.0"


@pytest.mark.parametrize("how", ["device tensor", "list", "strided view"])
def test_ragged_batch_is_bitwise_the_single_calls_and_zero_behind(ragged, how):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch
    w, single, _ = ragged
    if how == "device tensor":
        feats, flens = fbank_batch(w, torch.tensor(LENGTHS, dtype=torch.int64, device="cuda"))
    elif how == "list":
        feats, flens = fbank_batch(w, LENGTHS)
    else:
        wide = torch.full((w.size(0), w.size(1) + 37), -PAD, device="cuda")
        wide[:, 5:5 + w.size(1)] = w
        view = wide[:, 5:5 + w.size(1)]
        assert not view.is_contiguous()
        feats, flens = fbank_batch(view, LENGTHS)
    check_ragged(feats, flens, single)


def test_lengths_none_means_every_row_is_whole_and_lengths_are_clamped(ragged):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch
    w, _, whole = ragged
    T = _frames(w.size(1))
    feats, flens = fbank_batch(w)
    assert flens.tolist() == [T] * w.size(0)
    for b in range(w.size(0)):
        assert same_bits(feats[b], whole[b])
    over = [n + 10 ** 6 for n in LENGTHS[:4]] + [-5, -1, 0, 2 ** 40]          # clamped to [0, S_max] in the kernel
    feats2, flens2 = fbank_batch(w, over)
    assert flens2.tolist() == [T] * 4 + [0, 0, 0, T]
    assert same_bits(feats2[:4], feats[:4]) and same_bits(feats2[7], feats[7]) and not feats2[4:7].any()


def test_bf16_output_is_the_rounded_fp32_output(ragged):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch
    w, _, _ = ragged
    f32, l32 = fbank_batch(w, LENGTHS)
    b16, l16 = fbank_batch(w, LENGTHS, out_dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and same_bits(b16, f32.to(torch.bfloat16)) and torch.equal(l32, l16)


def test_batch_matches_the_oracle_at_the_single_call_bound(hip):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch
    lens = [16000 + 123, 560, 7000]
    w = torch.zeros(3, max(lens))
    for b, n in enumerate(lens):
        w[b, :n] = _wave(n, 40 + b)[0]
    feats, flens = fbank_batch(w.cuda(), lens)
    feats = feats.cpu()
    for b, n in enumerate(lens):
        ref = FO.fbank(w[b:b + 1, :n], num_mel_bins=80)
        got = feats[b, :_frames(n)]
        torch.testing.assert_close(got, ref, rtol=0, atol=2e-3)      # the bound of test_fbank_gpu: the arithmetic is the same
        assert float((got - ref).abs().mean()) < 1e-4


def test_dither_row_b_uses_its_own_noise_rows(hip):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank, fbank_batch
    lens = [400 + 160 * 70 + 3, 1000, 8000]
    S, T = max(lens), _frames(max(lens))
    w = torch.full((3, S), PAD)
    for b, n in enumerate(lens):
        w[b, :n] = _wave(n, 50 + b)[0]
    w, noise = w.cuda(), synth.randn((3, T, 400), 9).cuda()
    feats, _ = fbank_batch(w, lens, dither=1.0, noise=noise)
    plain, _ = fbank_batch(w, lens)
    for b, n in enumerate(lens):
        m = _frames(n)
        one = fbank(w[b:b + 1, :n], num_mel_bins=80, dither=1.0, noise=noise[b, :m].contiguous())
        assert same_bits(feats[b, :m], one) and not feats[b, m:].any()
        assert not torch.equal(feats[b, :m], plain[b, :m])              # (the noise was applied)


def test_23_bins_and_empty_batches(hip):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank, fbank_batch
    w = _wave(2000, 3).cuda()
    feats, flens = fbank_batch(w, num_mel_bins=23)
    assert same_bits(feats[0], fbank(w, num_mel_bins=23)) and flens.tolist() == [11]
    f0, l0 = fbank_batch(torch.zeros(0, 1000, device="cuda"))
    assert f0.shape == (0, 4, 80) and l0.shape == (0,)
    f1, l1 = fbank_batch(torch.zeros(2, 399, device="cuda"), out_dtype=torch.bfloat16)
    assert f1.shape == (2, 0, 80) and f1.dtype == torch.bfloat16 and l1.tolist() == [0, 0]


def test_refusals(hip):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.dataset.fbank import FbankStreamer, fbank_batch
    w = torch.zeros(2, 2000, device="cuda")
    with pytest.raises(PafcError):
        fbank_batch(w.cpu())
    with pytest.raises(PafcError):
        fbank_batch(torch.zeros(2, 4000, device="cuda")[:, ::2])                 # inner stride 2
    with pytest.raises(PafcError):
        fbank_batch(w, dither=1.0, noise=torch.zeros(2, 11, 399, device="cuda"))
    with pytest.raises(PafcError):
        fbank_batch(w, dither=1.0, noise=torch.zeros(11, 400, device="cuda"))
    with pytest.raises(PafcError):
        fbank_batch(w, torch.tensor([2000, 1000], dtype=torch.int32, device="cuda"))
    with pytest.raises(PafcError):
        fbank_batch(w, torch.tensor([2000, 1000], dtype=torch.int64))            # lengths on the host as a tensor
    with pytest.raises(PafcError):
        fbank_batch(w, [2000])
    with pytest.raises(PafcError):
        fbank_batch(w, out_dtype=torch.float16)
    with pytest.raises(PafcError):
        fbank_batch(w, frame_shift=20.0)
    with pytest.raises(PafcError):
        FbankStreamer(2, dither=1.0)
    st = FbankStreamer(2)
    with pytest.raises(PafcError):
        st.feed(torch.zeros(2, 500))
    with pytest.raises(PafcError):
        st.feed(torch.zeros(3, 500, device="cuda"))
    with pytest.raises(PafcError):
        st.feed_into(torch.zeros(2, 500, device="cuda"), torch.zeros(2, 1, 80, device="cuda"), 1)   # no room for the frame
    assert st.carry_len == 0 and st.frames_emitted == 0                          # a refused feed changed nothing


# ---- streaming --------------------------------------------------------------------------------------------------------
S_STREAM = 3 * 16000 + 77


@pytest.fixture(scope="module")
def stream_case(hip):
    from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch
    w = torch.cat([_wave(S_STREAM, 60 + b) for b in range(3)]).cuda()
    whole, _ = fbank_batch(w)
    return w, whole


def _cuts(name):
    rng = random.Random(11)
    if name == "one feed":
        return [S_STREAM]
    if name == "10240":
        sizes = [10240]
    elif name == "160":
        sizes = [160]
    elif name == "37 then irregular":
        out, pos = [], 0
        while pos < 1200:
            out.append(min(37, 1200 - pos))
            pos += out[-1]
        while pos < S_STREAM:
            out.append(min(rng.randint(1, 5000), S_STREAM - pos))
            pos += out[-1]
        return out
    else:                                                   # "empty feeds interleaved"
        out, pos = [], 0
        while pos < S_STREAM:
            out += [0, min(rng.randint(1, 3000), S_STREAM - pos)]
            pos += out[-1]
        return out + [0]
    n = sizes[0]
    return [n] * (S_STREAM // n) + ([S_STREAM % n] if S_STREAM % n else [])


def _run_stream(st, w, cuts):
    """Feed w by `cuts`; returns the concatenated frames, having checked every feed's frame count against the arithmetic."""
    out, pos, c = [], 0, 0
    for n in cuts:
        want = _frames(c + n)
        y = st.feed(w[:, pos:pos + n])
        assert y.shape == (w.size(0), want, 80), (pos, n, c)
        c = c + n - 160 * want
        assert st.carry_len == c < 560
        pos += n
        out.append(y)
    assert pos == w.size(1) and st.frames_emitted == sum(y.size(1) for y in out)
    return torch.cat(out, 1)


@pytest.mark.parametrize("cut", ["one feed", "10240", "160", "37 then irregular", "empty feeds interleaved"])
def test_stream_of_any_cut_is_bitwise_the_whole(stream_case, cut):
    from paper_accurate_fast_cheap_amd.dataset.fbank import FbankStreamer, stream_plan
    w, whole = stream_case
    cuts = _cuts(cut)
    assert sum(cuts) == S_STREAM
    if cut == "160":                                        # once filled: one frame per feed, n < c: the in-place shift
        assert stream_plan(240, 160) == (1, 240)
    st = FbankStreamer(3)
    got = _run_stream(st, w, cuts)
    assert same_bits(got, whole)
    st.reset()
    assert st.carry_len == 0 and st.frames_emitted == 0
    assert same_bits(_run_stream(st, w, cuts), whole)       # stale carry contents do not leak into the next stream


def test_stream_bf16_and_appending_into_a_strided_buffer(stream_case):
    from paper_accurate_fast_cheap_amd.dataset.fbank import FbankStreamer
    w, whole = stream_case
    T = whole.size(1)
    st = FbankStreamer(3, out_dtype=torch.bfloat16)
    buf = torch.full((3, T + 5, 80), 7.0, dtype=torch.bfloat16, device="cuda")
    rows = buf[:, 2:]                                       # rows strided, frames contiguous
    pos = got = 0
    for n in _cuts("37 then irregular"):
        got += st.feed_into(w[:, pos:pos + n], rows, got)
        pos += n
    assert got == T and same_bits(rows[:, :T], whole.to(torch.bfloat16))
    assert bool((buf[:, :2] == 7.0).all()) and bool((buf[:, T + 2:] == 7.0).all())      # nothing written around the frames


def test_steady_state_feed_replays_from_a_captured_graph(stream_case):
    """10 240 samples behind a carry of 320 are 64 frames and leave 320: the same launches every packet, so one captured feed
    replays over the packets that follow."""
    from paper_accurate_fast_cheap_amd.dataset.fbank import FbankStreamer, stream_plan
    from paper_accurate_fast_cheap_amd.utils import graph_step
    w, whole = stream_case
    n = 10240
    pk = [torch.cat([w, w], 1)[:, i * n:(i + 1) * n].contiguous() for i in range(6)]
    assert stream_plan(0, n) == (62, 320) and stream_plan(320, n) == (64, 320)
    eager = FbankStreamer(3)
    want = [eager.feed(p) for p in pk]
    st = FbankStreamer(3)
    got = [st.feed(pk[0])]
    static_in = pk[1].clone()
    got.append(graph_step.on_side_stream(w.device, lambda: st.feed(static_in)))       # warms the kernels up, c stays 320
    assert st.carry_len == 320
    graph, y_static = graph_step.capture(lambda: st.feed(static_in), w.device)
    assert graph is not None, "the runtime refused to capture the feed"
    for p in pk[2:]:
        static_in.copy_(p)
        graph.replay()
        got.append(y_static.clone())
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), f"packet {i}"
    assert same_bits(torch.cat(want, 1)[:, :whole.size(1)][:, :62 + 64 * 3], whole[:, :62 + 64 * 3])
