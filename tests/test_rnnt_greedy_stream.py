"""Streaming RNN-T greedy search (transducer/search/greedy_search.GreedyStreamer, hip_ops.RnntGreedyStream,
csrc/rnnt_greedy.hip: pafc_rnnt_greedy_stream_*): checks that need no GPU -- chunked decodes on CPU tensors against the
reference's golden tokens and the whole-utterance decode, reset in the middle of a stream, the reference's runtime step API,
the C boundary, the compiled kernels, and what the GPU path refuses."""
import ctypes
import os
import re

import pytest
import torch

from tests.conftest import load_golden
from tests.test_rnnt_greedy import ERR_ALIGN, ERR_DIMS, ERR_DTYPE, ERR_NULL, ERR_UNSUP, ERR_WS, _net, golden_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_API = ("pafc_rnnt_greedy_stream_workspace_bytes", "pafc_rnnt_greedy_stream_reset", "pafc_rnnt_greedy_stream_feed",
              "pafc_rnnt_greedy_stream_drain")


@pytest.fixture(scope="module")
def golden():
    return load_golden("rnnt_greedy_c5")


def _offline(model, enc, lens, n_steps):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import batch_greedy_search
    with torch.no_grad():
        return batch_greedy_search(model, enc, lens, n_steps)


def _cuts(T, how):
    """Chunk boundaries over T frames: 1 frame, 7 frames, or irregular sizes."""
    if how == "irregular":
        sizes, out, a = [3, 1, 9, 2, 5, 11, 4], [], 0
        i = 0
        while a < T:
            out.append((a, min(T, a + sizes[i % len(sizes)])))
            a, i = out[-1][1], i + 1
        return out
    step = {"one": 1, "seven": 7}[how]
    return [(a, min(T, a + step)) for a in range(0, T, step)]


def _stream(model, enc, lens, n_steps, cuts, Tmax=11):
    """Feed enc (B, T, D) in the given chunks; row b takes min(chunk, frames it has left) frames of each chunk (0 once its
    utterance has ended)."""
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import GreedyStreamer
    s = GreedyStreamer(model, enc.shape[0], Tmax, n_steps)
    with torch.no_grad():
        for a, b in cuts:
            nf = [max(0, min(b, int(L)) - a) for L in lens]
            s.feed(enc[:, a:b], nf)
    return s.results()


@pytest.mark.parametrize("how", ["one", "seven", "irregular"])
@pytest.mark.parametrize("n_steps", [64, 2])
def test_cpu_streamer_reproduces_golden_and_whole_utterance(golden, n_steps, how):
    model = golden_model(golden)
    enc, lens = golden["enc_out"], golden["enc_lens"]
    got = _stream(model, enc, lens.tolist(), n_steps, _cuts(enc.shape[1], how))
    assert [r.tokens for r in got] == golden["tokens"][n_steps]
    ref = _offline(model, enc, lens, n_steps)
    assert [r.times for r in got] == [r.times for r in ref]
    assert [r.score for r in got] == [r.score for r in ref]


def test_cpu_streamer_rows_sitting_chunks_out(golden):
    """Rows given 0 frames in some chunks (not only at their end) pick up where they stopped."""
    model = golden_model(golden)
    enc, lens = golden["enc_out"], golden["enc_lens"].tolist()
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import GreedyStreamer
    s = GreedyStreamer(model, 3, 8, 64)
    pos = [0, 0, 0]
    sched = [(1, 1, 1), (1, 0, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1)]
    i = 0
    with torch.no_grad():
        while any(p < L for p, L in zip(pos, lens)):
            on = sched[i % len(sched)]
            i += 1
            chunk = torch.zeros(3, 8, enc.shape[2])
            nf = []
            for b in range(3):
                n = min(8 if on[b] else 0, lens[b] - pos[b])
                chunk[b, :n] = enc[b, pos[b]:pos[b] + n]
                pos[b] += n
                nf.append(n)
            s.feed(chunk, nf)
    ref = _offline(model, enc, golden["enc_lens"], 64)
    res = s.results()
    assert [r.tokens for r in res] == golden["tokens"][64]
    assert [r.times for r in res] == [r.times for r in ref]
    assert [r.score for r in res] == [r.score for r in ref]


def test_cpu_reset_mid_stream_equals_a_fresh_decode(golden):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import GreedyStreamer
    model = golden_model(golden)
    enc = golden["enc_out"]
    s = GreedyStreamer(model, 3, 7, 64)
    with torch.no_grad():
        for a in range(0, 14, 7):
            s.feed(enc[:, a:a + 7])
        s.reset([1])
        fresh = GreedyStreamer(model, 1, 7, 64)
        for a in range(14, 28, 7):
            new = s.feed(enc[:, a:a + 7])
            assert fresh.feed(enc[1:2, a:a + 7]) == [new[1]]
            assert s.last_frames[1] == fresh.last_frames[0]          # absolute frames count from the reset
    r, f = s.results()[1], fresh.results()[0]
    assert r.tokens == f.tokens and r.score == f.score
    assert r.times == f.times
    ref = _offline(model, enc[1:2, 14:28], torch.tensor([14]), 64)[0]
    assert (r.tokens, r.times, r.score) == (ref.tokens, ref.times, ref.score)
    whole = _offline(model, enc[:, :28], torch.tensor([28, 28, 28]), 64)
    assert s.results()[0].tokens == whole[0].tokens and s.results()[2].tokens == whole[2].tokens


@pytest.mark.parametrize("n_steps", [64, 2])
def test_reference_step_api_loop_reproduces_golden(golden, n_steps):
    """A runtime's own loop (the reference's decoder runtime) from forward_predictor_init_state, forward_predictor_step and
    forward_joint_step only."""
    model = golden_model(golden)
    enc, lens = golden["enc_out"], golden["enc_lens"].tolist()
    out = []
    with torch.no_grad():
        for b in range(3):
            cache = model.forward_predictor_init_state()
            assert [tuple(c.shape) for c in cache] == [(2, 1, 64), (2, 1, 64)]
            tok = torch.tensor([[model.blank]])
            pred, new_cache = model.forward_predictor_step(tok, cache)
            hyp, t, k = [], 0, 0
            while t < lens[b]:
                y = int(model.forward_joint_step(enc[b:b + 1, t:t + 1], pred).log_softmax(-1).argmax(-1))
                if y != model.blank:
                    hyp.append(y)
                    k += 1
                    cache = new_cache
                    pred, new_cache = model.forward_predictor_step(torch.tensor([[y]]), cache)
                if y == model.blank or k >= n_steps:
                    t, k = t + 1, 0
            out.append(hyp)
    assert out == golden["tokens"][n_steps]


def test_stream_greedy_search_refuses_what_cannot_stream(golden):
    model = golden_model(golden)
    with pytest.raises(ValueError, match="decoding_chunk_size"):
        model.stream_greedy_search(torch.zeros(1, 100, 80), 0)
    with pytest.raises(ValueError, match="uni-directional"):   # the golden's encoder is no streaming encoder
        model.stream_greedy_search(torch.zeros(1, 100, 80), 16)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    so = build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT
    L = ctypes.CDLL(so)
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.pafc_rnnt_greedy_stream_workspace_bytes.restype = Z
    L.pafc_rnnt_greedy_stream_workspace_bytes.argtypes = [P, I, I, I]
    L.pafc_rnnt_greedy_workspace_bytes.restype = Z
    L.pafc_rnnt_greedy_workspace_bytes.argtypes = [P, I, I, I]
    L.pafc_rnnt_greedy_stream_reset.argtypes = [P, I, I, I, I, P, P, Z, P]
    L.pafc_rnnt_greedy_stream_feed.argtypes = [P, I, I, I, I, P, P, Z, P, P]
    L.pafc_rnnt_greedy_stream_drain.argtypes = [P, I, I, I, P, Z, I, P, P, P, P, P, P]
    return L


_ONE = 256


def test_stream_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "pafc_search.h")).read()
    for name in STREAM_API:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
    assert "pafc_rnnt_greedy_stream_feed" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_stream_workspace_size(lib):
    n = _net()
    ws = lambda B, T, k=64: lib.pafc_rnnt_greedy_stream_workspace_bytes(ctypes.byref(n), B, T, k)
    assert ws(8, 16) >= lib.pafc_rnnt_greedy_workspace_bytes(ctypes.byref(n), 8, 16, 64) + 8 * 8    # + the frame bases
    for B in (1, 2, 8, 64, 255):
        assert ws(B, 16) < ws(B + 1, 16)
    for T in (1, 2, 16, 100):
        assert ws(8, T) < ws(8, T + 1)
    assert ws(0, 16) == 0 and ws(257, 16) == 0 and ws(8, 0) == 0 and ws(8, 16, 0) == 0
    assert ws(8, 1 << 25, 64) == 0                                                 # Tmax * n_steps >= 2^31
    assert lib.pafc_rnnt_greedy_stream_workspace_bytes(None, 8, 16, 64) == 0


def test_stream_entry_points_validate_before_touching_the_device(lib):
    NULL, big = None, 1 << 40

    def reset(net=None, B=8, T=16, k=64, blank=0, mask=NULL, ws=_ONE, nbytes=big):
        net = net if net is not None else _net()
        return lib.pafc_rnnt_greedy_stream_reset(ctypes.byref(net), B, T, k, blank, mask, ws, nbytes, NULL)

    def feed(net=None, B=8, T=16, k=64, blank=0, nf=_ONE, ws=_ONE, nbytes=big):
        net = net if net is not None else _net()
        return lib.pafc_rnnt_greedy_stream_feed(ctypes.byref(net), B, T, k, blank, nf, ws, nbytes, NULL, NULL)

    def drain(B=8, T=16, k=64, ws=_ONE, nbytes=big, ld=10, tokens=_ONE, ntok=_ONE):
        n = _net()
        return lib.pafc_rnnt_greedy_stream_drain(ctypes.byref(n), B, T, k, ws, nbytes, ld, tokens, NULL, ntok, NULL, NULL, NULL)

    for fn in (reset, feed):
        assert fn(ws=NULL) == ERR_NULL
        assert fn(net=_net(out_w=None)) == ERR_NULL
        assert fn(B=0) == ERR_DIMS
        assert fn(B=257) == ERR_DIMS
        assert fn(T=0) == ERR_DIMS
        assert fn(k=0) == ERR_DIMS
        assert fn(blank=5000) == ERR_DIMS
        assert fn(net=_net(dtype=2)) == ERR_DTYPE
        assert fn(net=_net(hidden=642)) == ERR_UNSUP
        assert fn(T=1 << 25) == ERR_UNSUP
        assert fn(nbytes=1024) == ERR_WS
        assert fn(ws=_ONE + 16) == ERR_ALIGN
        assert fn(net=_net(out_w=_ONE + 8)) == ERR_ALIGN
    assert lib.pafc_rnnt_greedy_stream_reset(None, 8, 16, 64, 0, NULL, _ONE, big, NULL) == ERR_NULL
    assert lib.pafc_rnnt_greedy_stream_feed(None, 8, 16, 64, 0, _ONE, _ONE, big, NULL, NULL) == ERR_NULL
    assert feed(nf=NULL) == ERR_NULL
    n = _net()
    # a workspace big enough for the offline decode but without the frame bases is short
    short = lib.pafc_rnnt_greedy_workspace_bytes(ctypes.byref(n), 8, 16, 64)
    assert feed(nbytes=short) == ERR_WS
    assert drain(tokens=NULL) == ERR_NULL
    assert drain(ntok=NULL) == ERR_NULL
    assert drain(ws=NULL) == ERR_NULL
    assert lib.pafc_rnnt_greedy_stream_drain(None, 8, 16, 64, _ONE, big, 10, _ONE, NULL, _ONE, NULL, NULL, NULL) == ERR_NULL
    assert drain(ld=0) == ERR_DIMS
    assert drain(B=300) == ERR_DIMS
    assert drain(T=0) == ERR_DIMS
    assert drain(nbytes=8) == ERR_WS
    assert drain(ws=_ONE + 16) == ERR_ALIGN


@pytest.fixture(scope="module")
def asm():
    import subprocess
    from tests.test_rnnt_greedy import SRC
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    return subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.dirname(SRC), "-S", "--cuda-device-only", SRC, "-o", "-"],
                          stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.decode()


def test_stream_kernels_neither_spill_nor_use_scratch(asm):
    names = set(re.findall(r"\n(_ZN4pafc[^\n:]*greedy_stream_(\w+?)_kernel[^\n:]*):", asm))
    assert {k for _, k in names} == {"reset", "feed", "drain"}, names
    assert "scratch_" not in asm
    meta = asm[asm.index("amdhsa.kernels:"):]
    blocks = [b for b in re.split(r"\n  - \.", meta) if re.search(r"\.name:\s+_ZN4pafc\S*greedy_stream_", b)]
    assert len(blocks) == 3
    for b in blocks:                                                 # this PR's kernels: no VGPR / SGPR spill, no scratch
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert int(re.search(r"\.%s:\s+(\d+)" % key, b).group(1)) == 0, (key, b[:200])
    assert len(set(re.findall(r"\n(_ZN4pafc[^\n:]*greedy_lstm_kernel[^\n:]*):", asm))) == 4     # no new LSTM instantiations


# ---- what the GPU path refuses ------------------------------------------------------------------------------------------------------
def test_stream_unmet_names_each_unsupported_configuration(golden):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    un = lambda m, B=2, T=8, D=128, k=64: hip_ops.rnnt_greedy_stream_unmet(m.predictor, m.joint, B, T, D, "cpu", k)
    model = golden_model(golden)
    assert "Tmax" in un(model, T=0)
    assert "not on the GPU" in un(model)
    m = golden_model(golden)
    m.joint = TransducerJoint(50, 128, 64, 64, postjoin_linear=True).eval()
    assert "post-join" in un(m)
    m.joint = TransducerJoint(50, 128, 64, 64, activation="relu").eval()
    assert "tanh" in un(m)
    m = golden_model(golden)
    m.joint.hat_joint = True
    assert "hat_joint" in un(m)
    m = golden_model(golden)
    m.predictor.rnn = torch.nn.GRU(64, 64, 2, batch_first=True)
    assert "LSTM" in un(m)
    m = golden_model(golden)
    m.predictor.train()
    assert "dropout" in un(m)
    m = golden_model(golden)
    m.joint.ffn_out.to(torch.bfloat16)
    assert "all fp32 or all bf16" in un(m)


def test_gpu_stream_entry_raises_instead_of_falling_back(golden):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd._lib import PafcError
    model = golden_model(golden)
    model.joint.hat_joint = True
    with pytest.raises(PafcError, match="hat_joint"):
        hip_ops.RnntGreedyStream(model.predictor, model.joint, 3, 8)
    model = golden_model(golden)
    with pytest.raises(PafcError, match="not on the GPU"):
        hip_ops.RnntGreedyStream(model.predictor, model.joint, 3, 8)
    with pytest.raises(PafcError, match="Tmax"):
        hip_ops.RnntGreedyStream(model.predictor, model.joint, 3, 0)


def test_step_inner_products_round_alike_in_every_row_slot(asm):
    """The streamed decode equals the offline one only if a row's arithmetic does not depend on its position among the rows
    of a step (which differs between the two: chunk ends, idle rows, resets).  The LSTM, matvec and joint kernels unroll 8
    rows per pass; every row's 4-element product must be the same chain -- one multiply, three fmas (dot4) -- and not the
    mix of fused and unfused slots the compiler's own contraction produced (fp32 products are not exact, so that mix made an
    fp32 row's result depend on its slot).  Counted per kernel over the packed instructions the unrolled slots use."""
    src = open(os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc", "rnnt_greedy.hip")).read()
    assert not re.search(r"\+= w\[(g\]\[)?0\] \*", src)                 # every inner product goes through dot4
    seen = set()
    for m in re.finditer(r"\n(_ZN4pafc\S*greedy_(lstm|matvec|joint)_kernel\S*):[^\n]*\n(.*?)\.Lfunc_end", asm, re.S):
        body = m.group(3)
        mul, fma = len(re.findall(r"\bv_pk_mul_f32\b", body)), len(re.findall(r"\bv_pk_fma_f32\b", body))
        assert mul > 0 and fma == 3 * mul, (m.group(1), mul, fma)
        seen.add(m.group(1))
    assert len(seen) == 8                                               # lstm x 4, matvec x 2, joint x 2
