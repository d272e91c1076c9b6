"""pafc_fbank_stream_rows (dataset.fbank.FbankSlotStreamer): ragged feeds of independent streams into the slots of a pool.
For any cut of a stream into feeds, interleaved with other streams in any slot order, its frames are bit for bit fbank_batch
of its whole audio; what a call does not name is not touched."""
import pytest
import torch

from tests.test_fbank_gpu import _wave

pytestmark = pytest.mark.gpu
S, RING = 5, 96
# (slot, stream, samples) per feed, slots never sorted; stream "B" ends after feed 4 and "D" takes its slot
FEEDS = [
    [(4, "A", 0), (1, "B", 100), (2, "C", 400)],                 # n = 0; n < 160 (no frame); C: 0 + 400 == 400, its first frame
    [(2, "C", 160 * 70), (1, "B", 300)],                         # 70 frames (two tiles) beside B's c + n == 400: one frame
    [(4, "A", 159), (1, "B", 50)],                               # no row completes a frame: the carry update alone
    [(1, "B", 5000), (4, "A", 12000), (2, "C", 3000)],
    [(2, "C", 160 * 40), (1, "B", 7)],                           # C's frames 89.. wrap inside this launch (ring of 96)
    "reset 1",
    [(1, "D", 1000), (4, "A", 77)],
    [(4, "A", 0), (2, "C", 0)],                                  # nothing new at all
    [(1, "D", 160 * 96 - 700), (2, "C", 1), (4, "A", 160 * 64)],  # D: 92 frames, nearly the whole ring at once
    [(2, "C", 481), (1, "D", 3333)],
]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ragged_feeds_into_slots_equal_fbank_batch_of_each_whole_stream(hip, dtype):
    from paper_accurate_fast_cheap_amd.dataset.fbank import FbankSlotStreamer, fbank_batch
    total = {}
    for step in FEEDS:
        if not isinstance(step, str):
            for _, name, n in step:
                total[name] = total.get(name, 0) + n
    audio = {name: _wave(n, 90 + i).cuda() for i, (name, n) in enumerate(sorted(total.items()))}
    st = FbankSlotStreamer(S, RING, 80, dtype)
    st.ring.fill_(float("nan"))
    pos = {name: 0 for name in total}
    got = {name: [] for name in total}
    saw = set()
    for step in FEEDS:
        if isinstance(step, str):
            st.reset(int(step.split()[1]))
            continue
        n_max = max(n for _, _, n in step) + 3                   # (a packet buffer wider than any row's samples)
        chunk = torch.zeros(len(step), n_max, device="cuda")
        for i, (_, name, n) in enumerate(step):
            chunk[i, :n] = audio[name][0, pos[name]:pos[name] + n]
        named = [slot for slot, _, _ in step]
        others = [s for s in range(S) if s not in named]
        carry0, ring0 = st._carry.clone(), st.ring.clone()
        first = [st.frames_emitted[slot] for slot in named]
        frames = st.feed_rows(named, chunk, [n for _, _, n in step])
        for (slot, name, n), f0, f in zip(step, first, frames):
            pos[name] += n
            assert st.frames_emitted[slot] == f0 + f
            rows = [(f0 + k) % RING for k in range(f)]
            if rows and rows != sorted(rows):
                saw.add("wrap")
            if f > 64:
                saw.add("two tiles")
            if n > 0 and f == 0:
                saw.add("carry only")
            got[name].append(st.ring[slot, rows].clone())
        # what the call did not name is bitwise as it was: carries and rings of the other slots
        assert torch.equal(_bits(st._carry[others]), _bits(carry0[others]))
        assert torch.equal(_bits(st.ring[others]), _bits(ring0[others]))
        for (slot, _, n), f in zip(step, frames):
            if n == 0:
                assert torch.equal(_bits(st._carry[slot]), _bits(carry0[slot])) and f == 0
    assert saw == {"wrap", "two tiles", "carry only"}
    for name, wave in audio.items():
        want, lens = fbank_batch(wave, out_dtype=dtype)
        have = torch.cat(got[name])
        assert have.shape == want[0].shape and int(lens[0]) == have.size(0) > 0, name
        assert torch.equal(_bits(have), _bits(want[0])), name


def test_feed_rows_refuses_what_the_ring_cannot_hold(hip):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.dataset.fbank import FbankSlotStreamer
    st = FbankSlotStreamer(3, 8, 80)
    with pytest.raises(PafcError, match="cut the packet"):
        st.feed_rows([1], torch.zeros(1, 400 + 160 * 8, device="cuda"))
    with pytest.raises(PafcError, match="distinct slots"):
        st.feed_rows([1, 1], torch.zeros(2, 100, device="cuda"))
    with pytest.raises(PafcError, match="distinct slots"):
        st.feed_rows([3], torch.zeros(1, 100, device="cuda"))
    assert st.feed_rows([2, 0], torch.zeros(2, 400 + 160 * 7, device="cuda"), [400 + 160 * 7, 399]) == [8, 0]
    assert st.carry_len == [399, 0, 240] and st.frames_emitted == [0, 0, 8]
