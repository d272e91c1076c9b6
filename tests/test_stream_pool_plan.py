"""The host side of the stream pool, without a GPU: utils.stream_pool.PoolScheduler on scripted arrivals (slots, packet cuts
against the ring, rounds, steps, buckets), the argument validation of the three entry points the pool adds
(pafc_fbank_stream_rows, pafc_rows_gather, pafc_rows_scatter), and the cases StreamPool refuses."""
import ctypes
import os
import random
from types import SimpleNamespace

import pytest

EMBED = SimpleNamespace(subsampling_rate=4, right_context=6)      # chunk 16: windows of 67 frames every 64
CHUNK, WINDOW, STRIDE, CTX = 16, 67, 64, 7


def _samples(frames):
    return 400 + 160 * (frames - 1)


def _sched(slots=3, **kw):
    from paper_accurate_fast_cheap_amd.utils.stream_pool import PoolScheduler
    return PoolScheduler(EMBED, slots, CHUNK, **kw)


def _feed(s, packets):
    """One feed of {sid: samples}: cut, run the rounds; -> (pieces per cut, rounds of steps)."""
    left = {sid: [0, n] for sid, n in packets.items()}
    cuts, rounds = [], []
    while any(ol[1] > 0 for ol in left.values()):
        pieces = s.cut(left)
        assert pieces, "a cut takes something"
        cuts.append(pieces)
        while s.pending():
            rounds.append(s.next_round())
    return cuts, rounds


def _drain(s):
    rounds = []
    while s.pending():
        rounds.append(s.next_round())
    return rounds


def test_slots_are_reused_and_a_full_pool_says_so():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    s = _sched(3)
    a, b, c = s.open(), s.open(), s.open()
    assert (a, b, c) == (0, 1, 2) and s.active == [0, 1, 2]
    assert [s.slot_of(x) for x in (a, b, c)] == [0, 1, 2]
    with pytest.raises(PafcError, match="pool full"):
        s.open()
    s.close([b])
    assert _drain(s) == []                      # no frames: no window
    s.release(b)
    assert s.active == [0, 2]
    d = s.open()
    assert d == 3 and s.slot_of(d) == 1         # a new sid in the freed slot
    with pytest.raises(PafcError, match="sid 1 was closed"):
        s.slot_of(b)
    with pytest.raises(PafcError, match="sid 17 is unknown"):
        s.slot_of(17)
    # the successor starts from nothing
    slot = s.slots[1]
    assert (slot.carry_len, slot.frames, slot.consumed, slot.plan.T, slot.plan.start) == (0, 0, 0, 0, 0)


def test_three_windows_of_one_stream_take_three_rounds_while_another_releases_none():
    s = _sched(3)
    a, b = s.open(), s.open()
    cuts, rounds = _feed(s, {a: _samples(3 * STRIDE + CTX), b: 399})
    assert len(cuts) == 1 and [p[:4] for p in cuts[0]] == [(a, 0, 0, _samples(3 * STRIDE + CTX)), (b, 1, 0, 399)]
    assert len(rounds) == 3                     # the windows of one stream are sequential
    for i, steps in enumerate(rounds):
        assert len(steps) == 1
        (step,) = steps
        assert [(r.sid, r.start, r.length, r.final) for r in step.rows] == [(a, 64 * i, WINDOW, False)]
        assert step.first == (i == 0)
    assert s.slots[1].carry_len == 399 and s.slots[1].frames == 0


def test_a_round_never_holds_two_windows_of_a_stream_and_first_windows_are_kept_apart():
    s = _sched(4)
    a, b, c = s.open(), s.open(), s.open()
    _feed(s, {a: _samples(STRIDE + CTX)})       # a's first window ran
    _, rounds = _feed(s, {a: 160 * 2 * STRIDE, b: _samples(2 * STRIDE + CTX), c: _samples(STRIDE + CTX)})
    for steps in rounds:
        sids = [r.sid for st in steps for r in st.rows]
        assert len(sids) == len(set(sids))
        for st in steps:
            assert len({r.start == 0 for r in st.rows}) == 1 and st.first == (st.rows[0].start == 0)
    # round 0: the first windows of b and c together, apart from a's second window
    r0 = rounds[0]
    assert [(st.first, [r.sid for r in st.rows], st.batch) for st in r0] == [(True, [b, c], 2), (False, [a], 1)]
    # round 1: a's third and b's second window share a step; c has nothing left
    assert [(st.first, [r.sid for r in st.rows], st.batch) for st in rounds[1]] == [(False, [a, b], 2)]


@pytest.mark.parametrize("slots,want", [(1, [1]), (3, [1, 2, 3]), (5, [1, 2, 4, 5]), (8, [1, 2, 4, 8]),
                                        (64, [1, 2, 4, 8, 16, 32, 64])])
def test_bucket_sizes(slots, want):
    s = _sched(slots)
    assert s.buckets == want
    for rows in range(1, slots + 1):
        assert s.bucket(rows) == min(b for b in want if b >= rows)


def test_steps_are_cut_at_max_step_rows_and_padded_to_buckets():
    s = _sched(5, max_step_rows=3)
    sids = [s.open() for _ in range(5)]
    _feed(s, {x: _samples(STRIDE + CTX) for x in sids})
    _, rounds = _feed(s, {x: 160 * STRIDE for x in sids})
    (steps,) = rounds
    assert [(len(st.rows), st.batch, st.first) for st in steps] == [(3, 4, False), (2, 2, False)]
    with pytest.raises(ValueError):
        _sched(3, max_step_rows=4)
    # a first window is not padded: it runs eagerly in its own shape
    t = _sched(5)
    ids = [t.open() for _ in range(3)]
    _, rounds = _feed(t, {x: _samples(STRIDE + CTX) for x in ids})
    assert [(len(st.rows), st.batch, st.first) for st in rounds[0]] == [(3, 3, True)]


def test_a_packet_larger_than_the_free_ring_is_split():
    ring = WINDOW + STRIDE
    s = _sched(2, ring_frames=ring)
    a, b = s.open(), s.open()
    total = _samples(5 * STRIDE + CTX)
    cuts, rounds = _feed(s, {a: total, b: 1000})
    assert len(cuts) > 1
    assert sum(n for pieces in cuts for sid, _, _, n, _, _ in pieces if sid == a) == total
    offs = [(off, n) for pieces in cuts for sid, _, off, n, _, _ in pieces if sid == a]
    assert all(o1 + n1 == o2 for (o1, n1), (o2, _) in zip(offs, offs[1:])) and offs[0][0] == 0
    # b's packet went whole with the first cut
    assert [(off, n) for pieces in cuts for sid, _, off, n, _, _ in pieces if sid == b] == [(0, 1000)]
    # no cut ever brings more frames than the ring had free, and a's windows are those of the whole
    t = _sched(1, ring_frames=ring)
    x = t.open()
    left = {x: [0, total]}
    while left[x][1] > 0:
        before = t.slots[0].frames
        free = t.free_frames(0)
        t.cut(left)
        assert t.slots[0].frames - before <= free
        assert t.slots[0].frames - t.slots[0].consumed <= ring
        _drain(t)
    assert [(r.start, r.length) for steps in rounds for st in steps for r in st.rows if r.sid == a] == \
        [(64 * i, WINDOW) for i in range(5)]
    with pytest.raises(ValueError, match="ring_frames"):
        _sched(2, ring_frames=ring - 1)


@pytest.mark.parametrize("ring", [None, WINDOW + STRIDE])
def test_every_stream_gets_the_windows_of_its_whole_length(ring):
    """Random ragged arrivals through three slots: per stream the released windows equal chunk_windows of its final frame
    count, final on the last -- what tests/test_audio_stream_plan.py checks for one stream."""
    from paper_accurate_fast_cheap_amd.utils.graph_step import chunk_windows
    rng = random.Random(7)
    s = _sched(3, ring_frames=ring, max_step_rows=2)
    lengths = [_samples(259), _samples(286) + 77, _samples(5) + 50, 0, _samples(131) + 3, _samples(67), 123456]
    todo = list(enumerate(lengths))
    live, seen, done = {}, {}, {}
    while todo or live:
        while todo and len(live) < 3 and rng.random() < 0.7:
            _, S = todo.pop(0)
            sid = s.open()
            live[sid], seen[sid], done[sid] = [0, S], [], S
        packets = {}
        for sid, (pos, S) in live.items():
            if rng.random() < 0.8:
                packets[sid] = min(rng.choice([0, 1, 159, 160, 1000, 10240, 30000]), S - pos)
        _, rounds = _feed(s, packets)
        for sid, n in packets.items():
            live[sid][0] += n
        for steps in rounds:
            for st in steps:
                assert 1 <= len(st.rows) <= 2 and st.batch in s.buckets + [len(st.rows)]
                for r in st.rows:
                    seen[r.sid].append((r.start, r.length, r.final))
        for sid in [x for x, (pos, S) in live.items() if pos == S and rng.random() < 0.5]:
            s.close([sid])
            for steps in _drain(s):
                for st in steps:
                    for r in st.rows:
                        seen[r.sid].append((r.start, r.length, r.final))
            s.release(sid)
            del live[sid]
    assert len(seen) == len(lengths)
    for sid, S in done.items():
        T = 0 if S < 400 else 1 + (S - 400) // 160
        starts, window, _ = chunk_windows(EMBED, CHUNK, T)
        want = [(c, min(c + window, T) - c, i == len(starts) - 1) for i, c in enumerate(starts)]
        assert seen[sid] == want, (sid, S)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    path = build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT
    lib = ctypes.CDLL(path)
    P, I, G, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    lib.pafc_fbank_stream_rows.argtypes = [P, I, P, P, I, P, G, G, P, P, P, P, P, I, F, F, P, I, I, P]
    lib.pafc_rows_gather.argtypes = [P, P, I, P, P, I, I, P]
    lib.pafc_rows_scatter.argtypes = [P, P, I, P, I, I, P]
    return lib


NULLP, ERR_NULL, ERR_DIMS, ERR_DTYPE, ERR_UNSUP, ERR_ALIGN = ctypes.c_void_p(0), -1, -2, -6, -7, -8
ONE = ctypes.c_void_p(16)          # a non-null address that is never dereferenced (validation fails first)


def test_fbank_stream_rows_validates_before_it_touches_the_device(L):
    def call(rows, R=None, S=5, carry=ONE, rows_dev=ONE, chunk=ONE, ld=2000, n_max=2000, tables=ONE, nmel=80, dither=0.0,
             out=ONE, dtype=0, ring=96):
        host = (ctypes.c_int * max(len(rows), 1))(*rows) if rows is not None else NULLP
        return L.pafc_fbank_stream_rows(carry, S, host, rows_dev, len(rows) // 4 if R is None else R, chunk, ld, n_max, tables,
                                        tables, tables, tables, tables, nmel, dither, 0.97, out, dtype, ring, NULLP)
    ok = [3, 0, 1000, 0, 1, 399, 160, 7]
    assert call(ok, carry=NULLP) == ERR_NULL
    assert call(None, R=2) == ERR_NULL
    assert call(ok, rows_dev=NULLP) == ERR_NULL
    assert call(ok, tables=NULLP) == ERR_NULL
    assert call(ok, chunk=NULLP) == ERR_NULL
    assert call(ok, out=NULLP) == ERR_NULL
    assert call(ok, S=0) == ERR_DIMS
    assert call(ok, R=0) == ERR_DIMS
    assert call(ok + ok + ok, S=2) == ERR_DIMS                     # more rows than slots
    assert call(ok, nmel=0) == ERR_DIMS and call(ok, nmel=129) == ERR_DIMS
    assert call(ok, ring=0) == ERR_DIMS
    assert call(ok, ld=1999) == ERR_DIMS
    assert call(ok, dither=1.0) == ERR_UNSUP
    assert call(ok, dtype=2) == ERR_DTYPE
    assert call([5, 0, 1000, 0]) == ERR_DIMS                       # slot >= S
    assert call([-1, 0, 1000, 0]) == ERR_DIMS
    assert call([0, 560, 10, 0]) == ERR_DIMS                       # c outside [0, 560)
    assert call([0, -1, 10, 0]) == ERR_DIMS
    assert call([0, 0, 2001, 0]) == ERR_DIMS                       # n > n_max
    assert call([0, 0, -1, 0]) == ERR_DIMS
    assert call([0, 0, 10, -1]) == ERR_DIMS                        # first_frame < 0
    assert call([2, 0, 100, 0, 2, 0, 100, 0]) == ERR_DIMS          # one slot twice
    assert call([0, 0, 400 + 160 * 96, 0], n_max=1 << 20, ld=1 << 20) == ERR_DIMS      # 97 frames into a ring of 96
    assert call([0, 0, 2000, 0x7fffffff]) == ERR_DIMS              # first_frame + frames overflows
    # nothing to do is not an error, and needs neither chunk nor out
    assert call([0, 17, 0, 3, 4, 0, 0, 0], chunk=NULLP, out=NULLP) == 0


def test_rows_gather_and_scatter_validate_before_they_touch_the_device(L):
    def table(*entries):
        flat = [v for e in entries for v in e]
        return (ctypes.c_long * len(flat))(*flat)
    ok = table((1 << 20, 2 << 20, 1024, 0), (3 << 20, 4 << 20, 12, 0))
    assert L.pafc_rows_gather(NULLP, ONE, 2, ONE, NULLP, 3, 5, NULLP) == ERR_NULL
    assert L.pafc_rows_gather(ok, NULLP, 2, ONE, NULLP, 3, 5, NULLP) == ERR_NULL
    assert L.pafc_rows_gather(ok, ONE, 2, NULLP, NULLP, 3, 5, NULLP) == ERR_NULL
    assert L.pafc_rows_scatter(ok, ONE, 2, NULLP, 3, 5, NULLP) == ERR_NULL
    for n, m, S in ((0, 3, 5), (2, 0, 5), (2, 3, 0), (2, -1, 5)):
        assert L.pafc_rows_gather(ok, ONE, n, ONE, NULLP, m, S, NULLP) == ERR_DIMS
        assert L.pafc_rows_scatter(ok, ONE, n, ONE, m, S, NULLP) == ERR_DIMS
    for bad, code in (((0, 2 << 20, 1024, 0), ERR_NULL), ((1 << 20, 0, 1024, 0), ERR_NULL),
                      ((1 << 20, 2 << 20, 0, 0), ERR_DIMS), ((1 << 20, 2 << 20, 1022, 0), ERR_DIMS),       # not a multiple of 4
                      ((1 << 20, 2 << 20, 1021, 0), ERR_DIMS), ((1 << 20, 2 << 20, -4, 0), ERR_DIMS),
                      (((1 << 20) + 2, 2 << 20, 1024, 0), ERR_ALIGN), ((1 << 20, (2 << 20) + 1, 1024, 0), ERR_ALIGN)):
        t = table((5 << 20, 6 << 20, 16, 0), bad)
        assert L.pafc_rows_gather(t, ONE, 2, ONE, NULLP, 3, 5, NULLP) == code, bad
        assert L.pafc_rows_scatter(t, ONE, 2, ONE, 3, 5, NULLP) == code, bad
    ring = table((1 << 20, 2 << 20, 67 * 320, 96 * 320))
    assert L.pafc_rows_gather(ring, ONE, 1, ONE, NULLP, 3, 5, NULLP) == ERR_NULL          # a ring needs offs
    assert L.pafc_rows_scatter(ring, ONE, 1, ONE, 3, 5, NULLP) == ERR_UNSUP               # rings are filled by the fbank
    assert L.pafc_rows_gather(table((1 << 20, 2 << 20, 97 * 320, 96 * 320)), ONE, 1, ONE, ONE, 3, 5, NULLP) == ERR_DIMS
    assert L.pafc_rows_gather(table((1 << 20, 2 << 20, 320, 322)), ONE, 1, ONE, ONE, 3, 5, NULLP) == ERR_DIMS


# ---- what the pool refuses ---------------------------------------------------------------------------------------------
def _cpu_model(**over):
    import torch
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = dict(output_size=64, attention_heads=1, linear_units=64, num_blocks=1, input_layer="conv2d", normalize_before=True,
                cnn_module_kernel=15, causal=True, use_cnn_module=True, cnn_module_norm="layer_norm", activation_type="swish",
                pos_enc_layer_type="rel_pos", selfattention_layer_type="rwkv_tmix60", rnn_att_version="rwkv",
                rnn_att_direction="uni", rwkv_ctx_len=2048, rwkv_do_bfloat16=False)
    conf.update(over)
    torch.manual_seed(1)
    return ASRModel(11, ConformerEncoder(80, **conf), CTC(11, 64)).eval()


def test_the_pool_refuses_what_it_cannot_batch():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.utils.stream_pool import StreamPool
    with pytest.raises(ValueError, match="rnnt_beam_search.*device exception"):
        StreamPool(_cpu_model(), 4, 16, mode="rnnt_beam_search")
    with pytest.raises(ValueError, match="mode must be one of"):
        StreamPool(_cpu_model(), 4, 16, mode="attention_rescoring")
    with pytest.raises(ValueError, match="look-ahead.*age of the stream"):
        StreamPool(_cpu_model(causal=False, cnn_module_kernel=31), 4, 16)
    with pytest.raises(ValueError, match="bidirectional encoder needs the whole utterance"):
        StreamPool(_cpu_model(selfattention_layer_type="rwkv_tmix60_bidirectional", rnn_att_direction="bi"), 4, 16)
    with pytest.raises(ValueError, match="pre-norm"):
        StreamPool(_cpu_model(normalize_before=False), 4, 16)
    with pytest.raises(ValueError, match="needs a Transducer"):
        StreamPool(_cpu_model(), 4, 16, mode="rnnt_greedy_search")
    with pytest.raises(ValueError, match="decoding_chunk_size"):
        StreamPool(_cpu_model(), 4, 0)
    with pytest.raises(PafcError, match="no CPU fallback"):       # a model the pool takes, on the host: there is no CPU pool
        StreamPool(_cpu_model(), 4, 16)
