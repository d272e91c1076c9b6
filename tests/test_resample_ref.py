"""The resampler without a GPU: the float64 restatement (tests/resample_ref.py) is a resampler, the product's compact float32
tables are that restatement's dense table, and the stream plan (pafc_resample_stream_plan, host arithmetic) releases the
outputs of the whole for any cut."""
import os
import random

import numpy as np
import pytest

from tests import resample_ref as ref

RATES = sorted(ref.RATES)


@pytest.fixture(scope="module")
def built():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        build.build()
    from paper_accurate_fast_cheap_amd.dataset import resample
    return resample


@pytest.mark.parametrize("f_sig,f_in,measured", [(1000.0, 8000, 1.7e-4), (3000.0, 44100, 5.2e-4)])
def test_the_restatement_resamples_a_sine(f_sig, f_in, measured):
    """Within 2e-3 of the analytic 16 kHz signal in the interior (measured when the definition was restated: 1.7e-4 for the
    1 kHz sine from 8 kHz, 5.2e-4 for the 3 kHz sine from 44.1 kHz)."""
    orig, new = ref.ratio(f_in, 16000)
    S = f_in // 4
    x = np.sin(2 * np.pi * f_sig * np.arange(S) / f_in)
    y = ref.resample(x, orig, new)
    assert len(y) == ref.num_out(S, orig, new) == -(-16000 * S // f_in)
    want = np.sin(2 * np.pi * f_sig * np.arange(len(y)) / 16000.0)
    edge = 200                                                  # > (W + orig) new / orig outputs at every rate
    err = np.abs(y - want)[edge:-edge].max()
    print(f"{f_sig:.0f} Hz sine, {f_in} -> 16000 Hz: max interior error {err:.2e} (measured at the restatement: {measured:.1e})")
    assert err <= 2e-3


@pytest.mark.parametrize("rate", RATES)
def test_compact_tables_are_the_float32_dense_table(built, rate):
    orig, new, W, taps, span = ref.RATES[rate]
    plan = built.resample_plan(rate, 16000)
    assert (plan.orig, plan.new, plan.W, plan.taps, plan.span) == (orig, new, W, taps, span)
    assert (orig, new) == ref.ratio(rate, 16000) and W == ref.width(orig, new)
    dense32 = ref.dense_table(orig, new).astype(np.float32)
    assert dense32.shape == (new, taps)
    first, coef = plan.first.numpy(), plan.coef.numpy()
    assert first.dtype == np.int32 and coef.dtype == np.float32 and coef.shape == (new, span)
    assert first.min() >= 0 and (first + span).max() <= taps
    kept = np.zeros_like(dense32, dtype=bool)
    rebuilt = np.zeros_like(dense32)
    for i in range(new):
        kept[i, first[i]:first[i] + span] = True
        rebuilt[i, first[i]:first[i] + span] = coef[i]
    assert np.abs(rebuilt.astype(np.float64) - dense32.astype(np.float64)).max() <= 2.0 ** -23
    assert np.all(dense32[~kept] == 0.0)                         # every dropped tap is exactly 0.0f
    runs = [np.flatnonzero(row) for row in dense32]
    assert max(r[-1] - r[0] + 1 for r in runs) == span


@pytest.mark.parametrize("rate", RATES)
def test_stream_plan_releases_the_outputs_of_the_whole_for_any_cut(built, rate):
    orig, new, W, taps, _ = ref.RATES[rate]
    plan = built.resample_plan(rate, 16000)
    rng = random.Random(rate)
    lengths = [0, 1, W, W + orig - 1, W + orig, taps, 4001] + [rng.randint(1, 30000) for _ in range(12)]
    for S in lengths:
        N = ref.num_out(S, orig, new)
        assert plan.num_out(S) == N
        pos, c, out = 0, W, 0                                    # the carry starts as the left padding
        while pos < S:
            n = min(S - pos, rng.choice((0, 0, 1, 1, 2, orig, taps, rng.randint(1, 3 * taps + 50), rng.randint(1, 9000))))
            n_out, c_next = plan.stream_plan(c, n)
            frames = n_out // new
            assert n_out == frames * new
            assert pos + W - c == (out // new) * orig            # the carry begins where the next frame's window begins
            if frames:
                assert (frames - 1) * orig + taps <= c + n       # every released window lies inside carry + chunk
            assert (frames == 0) == (c + n < taps)               # ... and nothing that could be released is held back
            assert c_next == c + n - frames * orig and 0 <= c_next <= orig + 2 * W
            pos, c, out = pos + n, c_next, out + n_out
            assert out <= ref.num_out(pos, orig, new)            # only outputs the whole has
        left = N - out                                           # what flush computes, with zeros behind the last sample
        assert 0 <= left
        more, _ = plan.stream_plan(c, W + orig)                  # as many zeros complete every frame that holds a sample
        assert left <= more
        assert out + left == N


def test_stream_plan_refuses_what_is_not_a_carry(built):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    plan = built.resample_plan(44100, 16000)
    for c, n in ((-1, 10), (plan.taps + 1, 10), (0, -1)):
        with pytest.raises(PafcError):
            plan.stream_plan(c, n)


def test_unsupported_ratios_are_named_on_the_host(built):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    for f_in, f_out in ((15999, 16000), (16000, 15999), (400000, 16000), (0, 16000), (8000.5, 16000)):
        with pytest.raises(PafcError):
            built.resample_plan(f_in, f_out)
