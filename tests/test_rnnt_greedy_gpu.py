"""RNN-T greedy search on the MI355X (csrc/rnnt_greedy.hip through hip_ops.rnnt_greedy_search): the reference's golden tokens,
every decision of the kernel's own path checked against an fp64 restatement at the paper's dimensions (fp32 and bf16 weights),
bitwise repeatability, agreement with the reference's per-utterance loop on the same GPU, two streams, and the host reads."""
import math
import os
import sys
import threading
import warnings

import pytest
import torch

from tests.conftest import load_golden
from tests.test_rnnt_greedy import golden_model

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bench_rnnt_greedy as BG  # noqa: E402

pytestmark = pytest.mark.gpu
FP32_MARGIN = 1e-4


def _bf16_margin(joint):
    """The fp64 restatement below rounds to bf16 where the kernels do, so what separates the two is fp32 against fp64
    accumulation before each rounding: a value next to a bf16 rounding boundary can round to the neighbouring bf16 number
    (2^-8 relative; |tanh| <= 1 and |h|, |c| of the LSTM stay O(1)).  Allow 64 such one-ulp flips of elements of the joint's
    input (directly or through P) and both logits of the top-2 pair: 2 * 64 * max|W_out| * 2^-8."""
    return 2 * 64 * joint.ffn_out.weight.detach().float().abs().max().item() * 2.0 ** -8


def _fp64_replay(model, enc_row, T_b, toks, frames, n_steps, bf16):
    """Follow the kernel's path (tokens + frames) through predictor and joint in fp64; return every decision as
    (taken, fp64 argmax, fp64 top-2 margin) and the fp64 path score."""
    rnd = (lambda x: x.to(torch.bfloat16).double()) if bf16 else (lambda x: x)
    P_, J_ = model.predictor, model.joint
    d = lambda t: None if t is None else t.detach().double()
    rnn = P_.rnn
    L, H = rnn.num_layers, rnn.hidden_size
    W = [(d(getattr(rnn, f"weight_ih_l{l}")), d(getattr(rnn, f"weight_hh_l{l}")), d(getattr(rnn, f"bias_ih_l{l}")),
          d(getattr(rnn, f"bias_hh_l{l}"))) for l in range(L)]
    emb = d(P_.embed.weight)
    E = rnd(enc_row.double() @ d(J_.enc_ffn.weight).T + d(J_.enc_ffn.bias))
    Wo, bo = d(J_.ffn_out.weight), d(J_.ffn_out.bias)

    def predictor(tok, state):
        x, new = emb[tok], []
        for l, (wi, wh, bi, bh) in enumerate(W):
            h, c = state[l]
            g = wi @ x + bi + wh @ h + bh
            i, f, gg, o = torch.sigmoid(g[:H]), torch.sigmoid(g[H:2 * H]), torch.tanh(g[2 * H:3 * H]), torch.sigmoid(g[3 * H:])
            c1 = f * c + i * gg
            h1 = rnd(o * torch.tanh(c1))
            new.append((h1, rnd(c1)))
            x = h1
        po = rnd(d(P_.projection.weight) @ x + d(P_.projection.bias))
        return new, rnd(d(J_.pred_ffn.weight) @ po + d(J_.pred_ffn.bias))

    zero = torch.zeros(H, dtype=torch.float64, device=E.device)
    state = [(zero, zero)] * L
    pend, P = predictor(model.blank, state)
    by_frame = {}
    for y, f in zip(toks, frames):
        by_frame.setdefault(f, []).append(y)
    decisions, score = [], 0.0

    def decide(t, taken):
        nonlocal score
        lp = torch.log_softmax(Wo @ rnd(torch.tanh(rnd(E[t] + P))) + bo, -1)
        top = lp.topk(2)
        decisions.append((taken, int(top.indices[0]), float(top.values[0] - top.values[1])))
        score += float(lp[taken])

    for t in range(T_b):
        ys = by_frame.get(t, [])
        assert len(ys) <= n_steps
        for y in ys:
            decide(t, y)
            state = pend
            pend, P = predictor(y, state)
        if len(ys) < n_steps:
            decide(t, model.blank)
    return decisions, score


@pytest.mark.parametrize("n_steps", [64, 2])
def test_kernels_reproduce_the_reference_golden(hip, n_steps):
    g = load_golden("rnnt_greedy_c5")
    model = golden_model(g, "cuda")
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import batch_greedy_search
    with torch.no_grad():
        res = batch_greedy_search(model, g["enc_out"].cuda(), g["enc_lens"].cuda(), n_steps)
        assert [r.tokens for r in res] == g["tokens"][n_steps]
        if n_steps == 64:
            speech = torch.zeros(3, 37, 80, device="cuda")
            assert model.greedy_search(speech, g["enc_lens"].cuda()) == g["tokens"][64]
            dec = model.decode(["rnnt_greedy_search"], speech, g["enc_lens"].cuda())["rnnt_greedy_search"]
            assert [r.tokens for r in dec] == g["tokens"][64]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_steps", [2, 64])
def test_full_dims_follow_the_fp64_path(hip, dtype, n_steps):
    model = BG.to(BG.make_model(seed=1), "cuda", dtype)
    enc, lens = BG.make_batch(8, 60, seed=1, zero_row=True)
    enc = enc.to("cuda", dtype)
    with torch.no_grad():
        toks, frames, scores = BG.kernel_call(model, enc, lens.cuda(), n_steps)
    bf16 = dtype == torch.bfloat16
    bound = _bf16_margin(model.joint) if bf16 else FP32_MARGIN
    caps = 0
    for b in range(8):
        T_b = int(lens[b])
        assert len(toks[b]) == len(frames[b])
        assert all(0 <= f < T_b for f in frames[b]) and frames[b] == sorted(frames[b])
        assert all(0 <= y < 5000 and y != model.blank for y in toks[b])
        caps += sum(1 for f in set(frames[b]) if frames[b].count(f) >= n_steps)
        if T_b == 0:
            assert toks[b] == [] and scores[b] == 0.0
            continue
        with torch.no_grad():
            decisions, score = _fp64_replay(model, enc[b, :T_b].float() if not bf16 else enc[b, :T_b], T_b, toks[b], frames[b],
                                            n_steps, bf16)
        for taken, best, margin in decisions:
            assert taken == best or margin < bound, (b, taken, best, margin, bound)
        if not bf16:
            assert scores[b] == pytest.approx(score, rel=1e-4)
    assert sum(len(t) for t in toks) > 0
    if n_steps == 2:
        assert caps > 0


def test_two_calls_are_bitwise_identical(hip):
    model = BG.to(BG.make_model(seed=2), "cuda", torch.float32)
    enc, lens = BG.make_batch(8, 60, seed=2)
    enc, lens = enc.cuda(), lens.cuda()
    with torch.no_grad():
        a = BG.kernel_call(model, enc, lens)
        b = BG.kernel_call(model, enc, lens)
    assert a[0] == b[0] and a[1] == b[1]
    assert [struct_bits(x) for x in a[2]] == [struct_bits(x) for x in b[2]]


def struct_bits(x):
    import struct
    return struct.pack("<d", x)


def test_matches_basic_greedy_search_on_the_same_gpu(hip):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import basic_greedy_search
    model = BG.to(BG.make_model(seed=0), "cuda", torch.float32)
    enc, lens = BG.make_batch(8, 100, seed=0)
    enc = enc.cuda()
    with torch.no_grad():
        toks, _, _ = BG.kernel_call(model, enc, lens.cuda())
        ref = [basic_greedy_search(model, enc[b:b + 1], int(lens[b]), 64)[0] for b in range(8)]
    assert sum(int(a == r) for a, r in zip(toks, ref)) >= 7


def test_two_streams_give_the_sequential_results(hip):
    model = BG.to(BG.make_model(seed=3), "cuda", torch.float32)
    batches = [BG.make_batch(8, 60, seed=s) for s in (3, 4)]
    batches = [(e.cuda(), l.cuda()) for e, l in batches]
    with torch.no_grad():
        seq = [BG.kernel_call(model, e, l) for e, l in batches]
        out = [None, None]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]

        def run(i):
            with torch.cuda.stream(streams[i]):
                e, l = batches[i]
                streams[i].wait_stream(torch.cuda.default_stream())
                out[i] = BG.kernel_call(model, e, l)

        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    torch.cuda.synchronize()
    assert out == seq


def test_host_reads_per_call_are_as_documented(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    model = BG.to(BG.make_model(seed=5), "cuda", torch.float32)
    enc, lens = BG.make_batch(8, 60, seed=5)
    enc, lens_d = enc.cuda(), lens.cuda()
    with torch.no_grad():
        BG.kernel_call(model, enc, lens_d)                   # warm: library binding, allocator
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                toks, frames, _ = BG.kernel_call(model, enc, lens_d)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    reads = [x for x in w if "synchroniz" in str(x.message).lower()]
    S = BG.count_steps(toks, frames, lens.tolist(), 64)
    expect = 2 + math.ceil(max(0, S - enc.shape[1]) / hip_ops.RNNT_GREEDY_CHUNK)
    assert len(reads) == expect, ([str(x.message)[:80] for x in reads], S)
