"""CTC forced alignment on the MI355X: every output of pafc_ctc_align EQUALS tests/align_ref.py -- the int32 tensors
element for element, the score bit for bit (every alpha is one fp32 add on identical operands: no tolerance)."""
import numpy as np
import pytest
import torch

from tests.align_ref import align_ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
NINF = -float("inf")


def _reference(lp, hlens, ys, ylens, blank):
    """align_ref row by row on the rows' own frames and labels -> padded (align, first, last, score bits, ok) arrays."""
    B, T, _ = lp.shape
    Lmax = ys.shape[1]
    align = np.full((B, T), -1, np.int32)
    first, last = np.full((B, Lmax), -1, np.int32), np.full((B, Lmax), -1, np.int32)
    score, ok = np.full(B, -np.inf, np.float32), np.zeros(B, np.int32)
    for b in range(B):
        n, m = int(hlens[b]), int(ylens[b])
        a, f, l, sc, good = align_ref(lp[b, :n].float().numpy(), ys[b, :m].tolist(), blank)
        ok[b], score[b] = good, sc
        if good:
            align[b, :n], first[b, :m], last[b, :m] = a, f, l
    return align, first, last, score, ok


def _check(out, ref):
    align, first, last, score, ok = [o.cpu().numpy() for o in out]
    assert (ok == ref[4]).all(), (ok, ref[4])
    assert (align == ref[0]).all()
    assert (first == ref[1]).all() and (last == ref[2]).all()
    assert score.dtype == np.float32 and score.tobytes() == ref[3].tobytes(), (score, ref[3])


HL1, YL1 = [37, 20, 37, 5, 12, 0], [9, 20, 1, 0, 7, 3]


def _ragged(blank):
    """Shape 1: B = 6, T = 37, V = 11, multiples of 0.25 with 15 % -inf, NaN beyond hlen, valid token ids beyond ylen."""
    g = torch.Generator().manual_seed(11 + blank)
    B, T, V = 6, 37, 11
    toks = [v for v in range(V) if v != blank]
    lp = -(torch.randint(0, 12, (B, T, V), generator=g).float() * 0.25)
    lp[torch.rand(B, T, V, generator=g) < 0.15] = NINF
    ys = torch.tensor(toks)[torch.randint(0, len(toks), (B, 20), generator=g)]
    ys[1] = torch.tensor((toks * 2)[:20])                         # 20 distinct-from-neighbour labels in 20 frames: one path
    lp[1, torch.arange(20), ys[1]] = -0.25                        # ... which must be alive
    ys[4, :7] = ys[4, 0]                                          # six adjacent repeats: 7 + 6 > 12 frames
    lp[3, :5, blank] = -0.5                                       # L = 0: the blank column is the path
    for b in (0, 2):                                              # a living blank column: these rows have a path
        lp[b, :, blank] = lp[b, :, blank].clamp(min=-3.0)
    for b in range(B):
        lp[b, HL1[b]:] = float("nan")
    return lp, torch.tensor(HL1), ys, torch.tensor(YL1)


@pytest.fixture(scope="module")
def ragged():
    out = {}
    for blank in (0, 10):
        lp, hl, ys, yl = _ragged(blank)
        out[blank] = (lp, hl, ys, yl, _reference(lp, hl, ys, yl, blank))
    return out


def test_ragged_batch_equals_align_ref(hip, ragged):
    from paper_accurate_fast_cheap_amd.hip_ops import ctc_align
    lp, hl, ys, yl, ref = ragged[0]
    assert list(ref[4]) == [1, 1, 1, 1, 0, 0]
    out = ctc_align(lp.cuda(), hl.cuda(), ys.cuda(), yl.cuda(), 0)
    _check(out, ref)
    # without the padding: every row alone, its own frames and labels only
    for b in range(6):
        n, m = HL1[b], YL1[b]
        if n == 0:
            continue
        one = ctc_align(lp[b:b + 1, :n].cuda(), hl[b:b + 1].cuda(), ys[b:b + 1, :m].cuda(), yl[b:b + 1].cuda(), 0)
        _check(one, (ref[0][b:b + 1, :n], ref[1][b:b + 1, :m], ref[2][b:b + 1, :m], ref[3][b:b + 1], ref[4][b:b + 1]))


def test_ragged_batch_other_blank_bf16_and_row_stride(hip, ragged):
    from paper_accurate_fast_cheap_amd.hip_ops import ctc_align
    lp, hl, ys, yl, ref = ragged[10]
    _check(ctc_align(lp.cuda(), hl.cuda(), ys.cuda(), yl.cuda(), 10), ref)            # blank = V - 1
    lp, hl, ys, yl, ref = ragged[0]
    _check(ctc_align(lp.cuda().bfloat16(), hl.cuda(), ys.cuda(), yl.cuda(), 0), ref)  # multiples of 0.25 are exact in bf16
    wide = torch.full((6, 37, 16), float("nan"), device="cuda")                       # ldl = 16 > V = 11
    wide[:, :, :11] = lp.cuda()
    view = wide[:, :, :11]
    assert not view.is_contiguous()
    _check(ctc_align(view, hl.cuda(), ys.cuda(), yl.cuda(), 0), ref)


def _long(L, seed, T=640):
    """Shape 2: one utterance, T = 640, V = 50, L labels with a few adjacent repeats: more states than the block has
    threads, the last 64-state word of the pointer planes partly filled."""
    g = torch.Generator().manual_seed(seed)
    V = 50
    lp = -(torch.randint(0, 12, (1, T, V), generator=g).float() * 0.25)
    ys = torch.randint(1, V, (1, L), generator=g)
    for i in range(1, L):                                         # no accidental repeats, then eight on purpose
        if ys[0, i] == ys[0, i - 1]:
            ys[0, i] = 1 + ys[0, i] % (V - 1)
    for i in range(40, L, L // 8):
        ys[0, i] = ys[0, i - 1]
    return lp, torch.tensor([T]), ys, torch.tensor([L])


# S = 2 L + 1 is odd, so it is never a multiple of 16 (or of the 64 states of a pointer word): the boundary cases are one state
# short of it (S = 1215) and one state beyond it (S = 1217 = 19 x 64 + 1); S = 1201 ends inside a word.  All three run two states per thread.
@pytest.mark.parametrize("L", [600, 607, 608])
def test_more_states_than_threads(hip, L):
    from paper_accurate_fast_cheap_amd.hip_ops import ctc_align
    lp, hl, ys, yl = _long(L, L)
    ref = _reference(lp, hl, ys, yl, 0)
    assert ref[4][0] == 1
    _check(ctc_align(lp.cuda(), hl.cuda(), ys.cuda(), yl.cuda(), 0), ref)


# The kernel is compiled for 1, 2, 4, 8 and 16 states per thread of a 1024-thread block; the cases above reach 1 and 2.  These
# reach 4 (S = 2201: 3 strides), 8 (S = 4201: 5 strides) and 16 (S = 8401: 9 strides, past 8192), each with a last wave that
# stops at an earlier stride than the first.  A double loop over 4264 x 8401 cells in Python would take minutes, so the
# yardstick here is the package's host path, which tests/test_ctc_align.py pins to align_ref score bits included; T is L + 64:
# room for the eight adjacent repeats and some slack, so that the path has choices to make.
@pytest.mark.parametrize("L", [1100, 2100, 4200])
def test_four_eight_and_sixteen_states_per_thread(hip, L):
    from paper_accurate_fast_cheap_amd.hip_ops import ctc_align
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_forced_align
    lp, hl, ys, yl = _long(L, L, T=L + 64)
    (host,), host_ali = ctc_forced_align(lp, hl, ys, yl, 0, return_alignment=True)
    assert host.ok and host.tokens == ys[0].tolist()
    align, first, last, score, ok = [o.cpu() for o in ctc_align(lp.cuda(), hl.cuda(), ys.cuda(), yl.cuda(), 0)]
    assert ok.tolist() == [1]
    assert torch.equal(align, host_ali)
    assert first[0].tolist() == host.times and last[0].tolist() == host.end_times
    assert score.numpy().tobytes() == np.float32(host.score).tobytes(), (score, host.score)


def test_label_count_outside_the_label_tensor_is_not_ok(hip, ragged):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_forced_align
    lp, hl, ys, yl, ref = ragged[0]
    yl = yl.clone()
    yl[0], yl[2] = 21, -1                                         # Lmax = 20
    host, host_ali = ctc_forced_align(lp, hl, ys, yl, 0, return_alignment=True)
    dev, dev_ali = ctc_forced_align(lp.cuda(), hl.cuda(), ys.cuda(), yl.cuda(), 0, return_alignment=True)
    assert torch.equal(dev_ali.cpu(), host_ali) and (host_ali[0] == -1).all() and (host_ali[2] == -1).all()
    assert [r.ok for r in host] == [r.ok for r in dev] == [False, True, False, True, False, False]
    for h, d in zip(host, dev):
        assert (d.tokens, d.times, d.end_times, d.score) == (h.tokens, h.times, h.end_times, h.score)
    assert host[0].tokens == ys[0].tolist() and host[2].tokens == [] and host[0].score == NINF and host[0].times == []


def test_kernel_equals_the_reference_goldens(hip):
    from paper_accurate_fast_cheap_amd.hip_ops import ctc_align
    from paper_accurate_fast_cheap_amd.utils.ctc_utils import force_align
    g = load_golden("force_align")
    for c in g["cases"]:
        T, y = c["lp"].shape[0], torch.tensor([c["y"]])
        align, first, last, score, ok = ctc_align(c["lp"].unsqueeze(0).cuda(), torch.tensor([T]).cuda(), y.cuda(),
                                                  torch.tensor([len(c["y"])]).cuda(), c["blank"])
        assert int(ok[0]) == 1 and align[0].tolist() == c["align"] and first[0].tolist() == c["peaks"], c["kind"]
        assert force_align(c["lp"].cuda(), y[0].cuda(), c["blank"]) == c["align"]
    w = g["wrap"]                                                 # where the reference wraps, the kernel is the yardstick
    ref = align_ref(w["lp"].numpy(), w["y"], w["blank"])
    assert force_align(w["lp"].cuda(), torch.tensor(w["y"]), w["blank"]) == ref[0] != w["align"]


def test_search_front_end_equals_the_host_path(hip, ragged):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_forced_align
    lp, hl, ys, yl, ref = ragged[0]
    host, host_ali = ctc_forced_align(lp, hl, ys, yl, 0, return_alignment=True)
    dev, dev_ali = ctc_forced_align(lp.cuda(), hl.cuda(), ys.cuda(), yl.cuda(), 0, return_alignment=True)
    fetch = ctc_forced_align(lp.cuda(), hl.cuda(), ys.cuda(), yl.cuda(), 0, return_alignment=True, defer=True)
    assert callable(fetch)
    later, later_ali = fetch()
    assert torch.equal(dev_ali.cpu(), host_ali) and torch.equal(later_ali.cpu(), host_ali)
    for h, d, l in zip(host, dev, later):
        for r in (d, l):
            assert (r.ok, r.tokens, r.times, r.end_times, r.nbest, r.nbest_times) == \
                (h.ok, h.tokens, h.times, h.end_times, h.nbest, h.nbest_times)
            assert np.float32(r.score).tobytes() == np.float32(h.score).tobytes() and r.nbest_scores == [r.score]
    assert [r.ok for r in dev] == [bool(v) for v in ref[4]] and dev[4].times == [] and dev[4].score == NINF


def test_captured_call_replays_on_refreshed_inputs(hip, ragged):
    from paper_accurate_fast_cheap_amd.hip_ops import ctc_align
    from paper_accurate_fast_cheap_amd.utils import graph_step
    a = ragged[0]
    dev = torch.device("cuda")
    lp, hl, ys, yl = [t.cuda().clone() for t in a[:4]]
    eager = {0: ctc_align(lp, hl, ys, yl, 0)}
    graph_step.on_side_stream(dev, lambda: ctc_align(lp, hl, ys, yl, 0))       # the eager step before a capture, off the default stream
    graph, out = graph_step.capture(lambda: ctc_align(lp, hl, ys, yl, 0), dev)
    assert graph is not None, "the runtime refused to capture pafc_ctc_align"
    # Four calls of other shapes, and tensors filled over whatever they freed, between the capture and its replays: the
    # graph's workspace is the graph's own, so none of this may reach it, and no replay may write into these.
    others = []
    for B, T, Lm in ((1, 37, 20), (6, 50, 20), (3, 37, 9), (6, 37, 33)):
        o = ctc_align(torch.zeros(B, T, 11, device=dev), torch.full((B,), T, device=dev),
                      torch.ones(B, Lm, dtype=torch.long, device=dev), torch.ones(B, device=dev, dtype=torch.long), 0)
        others.append([t.clone() for t in o])
        del o
    torch.cuda.synchronize()
    fill = [torch.full((1 << 16,), 0x5a, dtype=torch.uint8, device=dev) for _ in range(16)]
    # a second input set of the same shapes, then the first again: the graph reads whatever the fixed tensors hold
    g = torch.Generator().manual_seed(99)
    lp2 = -(torch.randint(0, 12, (6, 37, 11), generator=g).float() * 0.25)
    lp2[torch.rand(6, 37, 11, generator=g) < 0.15] = NINF
    hl2 = torch.tensor([30, 37, 9, 1, 37, 2])
    ys2 = torch.randint(1, 11, (6, 20), generator=g)
    yl2 = torch.tensor([4, 12, 9, 0, 20, 3])
    ref2 = _reference(lp2, hl2, ys2, yl2, 0)
    for data, ref in ((lp2, hl2, ys2, yl2), ref2), (a[:4], a[4]):
        for dst, src in zip((lp, hl, ys, yl), data):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        _check(out, ref)
    _check(eager[0], a[4])
    assert all(bool((f == 0x5a).all()) for f in fill)
    for o in others:                                              # one label, all log-probabilities 0: score 0, ok, label at frame T-1 or so
        assert o[4].tolist() == [1] * o[4].numel() and o[3].tolist() == [0.0] * o[3].numel()
