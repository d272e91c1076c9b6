"""CTC forced alignment without a GPU: the yardstick (tests/align_ref.py) and the package's host path against the reference's
recorded alignments (tests/golden/force_align.pt), the case the reference gets wrong, the time-stamp helpers, the cases the
reference does not define, the C ABI's argument checks, and ASRModel.align on a stubbed encoder."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests.align_ref import align_ref
from tests.conftest import load_golden

NINF = -float("inf")


@pytest.fixture(scope="module")
def golden():
    return load_golden("force_align")


def _host(lp, y, blank=0):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_forced_align
    res, align = ctc_forced_align(lp.unsqueeze(0), torch.tensor([lp.shape[0]]), torch.tensor([list(y)], dtype=torch.long).reshape(1, -1),
                                  torch.tensor([len(y)]), blank, return_alignment=True)
    return res[0], align[0].tolist()


def _bits(x):
    return np.float32(x).tobytes()


def _collapse(ali, blank):
    out, prev = [], None
    for tok in ali:
        if tok != prev and tok != blank:
            out.append(tok)
        prev = tok
    return out


def test_golden_holds_enough_cases(golden):
    assert len(golden["cases"]) >= 20
    kinds = " ".join(c["kind"] for c in golden["cases"])
    assert "inf" in kinds and "q" in kinds and "rand" in kinds
    assert any(any(a == b for a, b in zip(c["y"], c["y"][1:])) for c in golden["cases"])         # adjacent repeats
    assert any(c["blank"] != 0 for c in golden["cases"])


def test_align_ref_equals_every_golden(golden):
    for c in golden["cases"]:
        ali, first, last, score, ok = align_ref(c["lp"].numpy(), c["y"], c["blank"])
        assert ok == 1 and ali == c["align"], c["kind"]
        assert first == c["peaks"]


def test_host_path_equals_goldens_and_align_ref(golden):
    for c in golden["cases"]:
        r, ali = _host(c["lp"], c["y"], c["blank"])
        ref = align_ref(c["lp"].numpy(), c["y"], c["blank"])
        assert r.ok and ali == c["align"] == ref[0], c["kind"]
        assert r.tokens == c["y"] and r.nbest == [c["y"]]
        assert r.times == ref[1] == c["peaks"] and r.end_times == ref[2] and r.nbest_times == [r.times]
        assert _bits(r.score) == _bits(ref[3]) and r.nbest_scores == [r.score]


def test_the_case_the_reference_wraps(golden):
    """The reference reads log_alpha[t-1, -1] for state 0: on this case its path returns from the final blank to the first and
    its alignment does not collapse to the labels (kept as the record).  The correct recursion's does."""
    w = golden["wrap"]
    y, blank = w["y"], w["blank"]
    assert _collapse(w["align"], blank) != y
    ali, first, last, score, ok = align_ref(w["lp"].numpy(), y, blank)
    assert ok == 1 and _collapse(ali, blank) == y and len(ali) == w["lp"].shape[0]
    r, host_ali = _host(w["lp"], y, blank)
    assert r.ok and host_ali == ali and r.times == first and r.end_times == last and _bits(r.score) == _bits(score)
    # a valid path: the score is the sum of its own log-probabilities, frame by frame in fp32
    acc = np.float32(0)
    for t, tok in enumerate(ali):
        acc = np.float32(acc + w["lp"][t, tok].numpy()) if t else np.float32(w["lp"][0, tok].numpy())
    assert _bits(acc) == _bits(score)


def test_peak_times_and_stamps_equal_the_reference(golden):
    from paper_accurate_fast_cheap_amd.utils.ctc_utils import force_align, gen_ctc_peak_time, gen_timestamps_from_peak
    for c in golden["cases"]:
        T = c["lp"].shape[0]
        assert force_align(c["lp"], torch.tensor(c["y"]), c["blank"]) == c["align"]
        peaks = gen_ctc_peak_time(c["align"], c["blank"])
        assert peaks == c["peaks"] == align_ref(c["lp"].numpy(), c["y"], c["blank"])[1]
        for period in golden["periods"]:
            assert gen_timestamps_from_peak(peaks, T * period, period, 1.0) == c["stamps"][period]
    assert gen_ctc_peak_time([0, 3, 3, 0, 3, 4, 4], 0) == [1, 4, 5]
    assert gen_timestamps_from_peak([], 1.0) == []
    assert gen_timestamps_from_peak([10], 0.6) == [(0, 0.6)]            # defaults: 0.04 s frames, 1.0 s tokens


def _both(lp, y, blank=0):
    ref = align_ref(lp.numpy(), y, blank)
    r, ali = _host(lp, y, blank)
    assert bool(ref[4]) == r.ok
    assert ali == ref[0]
    if r.ok:
        assert r.times == ref[1] and r.end_times == ref[2] and _bits(r.score) == _bits(ref[3])
    else:
        assert r.times == [] and r.score == NINF and ref[1] == [-1] * len(y) and ref[3] == np.float32(NINF)
    return ref, r


def test_cases_the_reference_does_not_define():
    g = torch.Generator().manual_seed(3)
    lp = -(torch.randint(0, 8, (7, 5), generator=g).float() * 0.25)
    # L = 0: every frame blank, the score is the blank column summed in frame order
    ref, r = _both(lp, [], 0)
    acc = np.float32(lp[0, 0].numpy())
    for t in range(1, 7):
        acc = np.float32(acc + lp[t, 0].numpy())
    assert r.ok and ref[0] == [0] * 7 and _bits(r.score) == _bits(acc) and r.times == []
    # too many adjacent repeats for the frames: 4 labels + 3 repeats = 7 fits, + 1 more label does not
    assert _both(lp, [2, 2, 2, 2], 0)[1].ok
    ref, r = _both(lp, [2, 2, 2, 2, 3], 0)
    assert not r.ok and ref[0] == [-1] * 7
    assert not _both(lp, [1, 0, 2], 0)[1].ok                     # a label equals the blank
    assert not _both(lp, [1, 5], 0)[1].ok                        # a label >= V
    assert not _both(lp, [1, -1], 0)[1].ok
    assert not _both(torch.full((7, 5), NINF), [1, 2], 0)[1].ok  # all -inf: no path of finite score
    dead = lp.clone()
    dead[3, :] = NINF                                            # one frame that nothing survives
    assert not _both(dead, [1, 2], 0)[1].ok
    assert not _both(lp[:0], [1], 0)[1].ok                       # no frames
    assert _both(lp, [1, 2, 3], 4)[1].ok                         # blank = V - 1


def test_batch_with_padding_equals_the_rows_alone():
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_forced_align
    g = torch.Generator().manual_seed(5)
    lp = -(torch.randint(0, 8, (3, 12, 6), generator=g).float() * 0.25)
    hl, yl = [12, 7, 0], [3, 2, 1]
    ys = torch.tensor([[1, 2, 3], [4, 4, 5], [2, 1, 1]])
    for b in range(3):
        lp[b, hl[b]:] = float("nan")
    res, ali = ctc_forced_align(lp, torch.tensor(hl), ys, torch.tensor(yl), 0, return_alignment=True)
    for b in range(3):
        ref = align_ref(lp[b, :hl[b]].numpy(), ys[b, :yl[b]].tolist(), 0)
        assert ali[b].tolist() == ref[0] + [-1] * (12 - hl[b]) and res[b].ok == bool(ref[4])
        assert res[b].tokens == ys[b, :yl[b]].tolist()
    assert not res[2].ok and res[2].score == NINF and res[2].times == []


def test_a_length_outside_its_tensor_is_not_ok():
    """The kernel's rule, on the host: ctc_lens[b] outside [1, T] or ys_lens[b] outside [0, Lmax] is not alignable; the
    tokens reported are the labels with the count clamped."""
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_forced_align
    lp = torch.zeros(4, 6, 5)
    ys = torch.tensor([[1, 2, 3]] * 4)
    res, ali = ctc_forced_align(lp, torch.tensor([6, 6, 7, 6]), ys, torch.tensor([4, -1, 2, 3]), 0, return_alignment=True)
    assert [r.ok for r in res] == [False, False, False, True]
    assert [r.tokens for r in res] == [[1, 2, 3], [], [1, 2], [1, 2, 3]]
    assert all(r.score == NINF and r.times == [] and r.end_times == [] for r in res[:3])
    assert (ali[:3] == -1).all() and (ali[3] >= 0).all()


def test_c_abi_argument_checks_and_workspace_without_a_gpu():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    so = build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT
    L = ctypes.CDLL(so)
    P, I, G, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t
    L.pafc_ctc_align_workspace_bytes.restype = Z
    L.pafc_ctc_align_workspace_bytes.argtypes = [I, I, I]

    def formula(B, T, Lmax):            # two 64-bit planes per 64 states and frame + three clock stamps (32 bytes) per utterance
        return B * T * ((2 * Lmax + 1 + 63) // 64) * 16 + 32 * B
    assert L.pafc_ctc_align_workspace_bytes(8, 250, 40) == formula(8, 250, 40) == 8 * 250 * 2 * 16 + 256
    assert L.pafc_ctc_align_workspace_bytes(1, 45000, 5000) == formula(1, 45000, 5000) == 45000 * 157 * 16 + 32
    assert L.pafc_ctc_align_workspace_bytes(0, 250, 40) == 0
    assert L.pafc_ctc_align_workspace_bytes(3, 9, 0) == formula(3, 9, 0)
    f = L.pafc_ctc_align
    f.argtypes = [I, I, I, I, P, G, P, P, I, P, I, P, Z, P, P, P, I, P, P, P]
    NULL, one, big = P(0), P(16), 1 << 30

    def call(dtype=0, B=2, T=8, V=16, lp=one, ldl=16, hlens=one, ys=one, ldy=4, ylens=one, blank=0, ws=one, nws=big, align=one,
             first=one, last=one, ldt=4, score=one, ok=one):
        return f(dtype, B, T, V, lp, ldl, hlens, ys, ldy, ylens, blank, ws, nws, align, first, last, ldt, score, ok, NULL)
    for name in ("lp", "hlens", "ys", "ylens", "ws", "align", "first", "last", "score", "ok"):
        assert call(**{name: NULL}) == -1, name
    assert call(B=0) == -2 and call(T=0) == -2 and call(V=0) == -2 and call(B=-1) == -2
    assert call(ldl=15) == -2 and call(ldy=-1) == -2 and call(ldt=3) == -2
    assert call(blank=16) == -2 and call(blank=-1) == -2
    assert call(dtype=5) == -6
    assert call(ldy=8192, ldt=8192) == -7                       # S beyond 16 states per thread of a 1024-thread block
    assert call(nws=2 * 8 * 16 + 63) == -4                      # one byte short
    assert call(ws=P(24)) == -8                                 # workspace not 16-byte aligned


class _StubEncoder(torch.nn.Module):
    """Returns a fixed encoder output (the alignment is what is under test), with the subsampling rate align() asks for."""

    def __init__(self, enc_out):
        super().__init__()
        self.register_buffer("enc_out", enc_out)
        self.embed = types.SimpleNamespace(subsampling_rate=4)

    def forward(self, x, lens, *a, **k):
        mask = (torch.arange(self.enc_out.shape[1])[None, :] < lens[:, None]).unsqueeze(1)
        return self.enc_out[:x.shape[0]], mask


def test_asr_model_align_on_the_host():
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    torch.manual_seed(0)
    V, D, Tp = 12, 16, 30
    model = ASRModel(V, _StubEncoder(torch.randn(3, Tp, D)), CTC(V, D)).eval()
    lens = torch.tensor([30, 21, 4])
    text = torch.tensor([[3, 3, 5, 7, 2], [4, 9, 1, 0, 0], [1, 2, 3, 4, 5]])
    tlens = torch.tensor([5, 3, 5])
    res = model.align(torch.zeros(3, 120, 80), lens, text, tlens, tokens_info=True)
    plain = model.align(torch.zeros(3, 120, 80), lens, text, tlens)
    for b in range(2):
        r = res[b]
        assert r.ok and r.tokens == text[b, :tlens[b]].tolist() and plain[b].tokens_info is None and plain[b].times == r.times
        assert all(0 <= t < int(lens[b]) for t in r.times) and all(a < b_ for a, b_ in zip(r.times, r.times[1:]))
        assert all(f <= l for f, l in zip(r.times, r.end_times))
        assert len(r.tokens_info) == len(r.tokens)
        for i, (start, end) in enumerate(r.tokens_info):
            assert 0 <= start <= end <= Tp * 0.04 + 1e-9
            if i:
                assert start >= r.tokens_info[i - 1][1]          # intervals do not overlap
    assert not res[2].ok and res[2].times == [] and res[2].tokens_info == [] and res[2].score == NINF   # 5 labels, 4 frames
    pen = model.align(torch.zeros(3, 120, 80), lens, text, tlens, blank_penalty=2.0)
    assert pen[0].tokens == res[0].tokens and pen[0].score != res[0].score
