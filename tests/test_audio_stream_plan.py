"""The host arithmetic of audio-driven streaming, without a GPU: the fbank carry plan (pafc_fbank_stream_plan: how many frames a
packet completes, how many samples are carried on) and the window release rule (utils.audio_stream.WindowRelease: which encoder
windows of forward_chunk_by_chunk the frames so far complete)."""
import os
import random
import shutil
import subprocess
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _num_frames(S):
    return 0 if S < 400 else 1 + (S - 400) // 160


@pytest.fixture(scope="module")
def plan():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        build.build()
    from paper_accurate_fast_cheap_amd.dataset.fbank import stream_plan
    return stream_plan


def test_carry_plan_every_carry_length(plan):
    for c in range(560):
        for n in (0, 1, 159, 160, 161, 399, 400, 10240):
            frames, c_next = plan(c, n)
            assert frames == _num_frames(c + n), (c, n)
            assert c_next == c + n - 160 * frames and 0 <= c_next < 560, (c, n, frames, c_next)
            if frames == 0:
                assert c_next == c + n < 400


def test_carry_plan_refuses_what_is_not_a_carry(plan):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    for c, n in ((-1, 10), (560, 10), (0, -1)):
        with pytest.raises(PafcError):
            plan(c, n)


def test_carry_plan_frames_add_up_over_random_cuts(plan):
    rng = random.Random(7)
    for S in range(3001):
        pos, c, total = 0, 0, 0
        while pos < S:
            n = min(S - pos, rng.choice((1, 37, 159, 160, 161, 400, rng.randint(1, 1200))))
            frames, c_next = plan(c, n)
            assert pos - c == 160 * total          # this packet's first frame starts where the last one's frames stopped
            pos, c, total = pos + n, c_next, total + frames
            assert c < 560
        assert total == _num_frames(S), S


@pytest.mark.parametrize("sub,right_context", [(4, 6), (6, 10), (8, 14)])
@pytest.mark.parametrize("chunk", [1, 4, 16])
def test_window_release_equals_the_offline_window_plan(chunk, sub, right_context):
    from paper_accurate_fast_cheap_amd.utils.audio_stream import WindowRelease
    from paper_accurate_fast_cheap_amd.utils.graph_step import chunk_windows
    embed = SimpleNamespace(subsampling_rate=sub, right_context=right_context)
    ctx = right_context + 1
    _, window, stride = chunk_windows(embed, chunk, 0)
    assert window == (chunk - 1) * sub + ctx and stride == sub * chunk
    rng = random.Random(chunk * 100 + sub)
    for T in range(3 * stride + window + 8 + 1):
        starts, _, _ = chunk_windows(embed, chunk, T)
        want = [(c, min(c + window, T) - c, i == len(starts) - 1) for i, c in enumerate(starts)]
        if T < ctx:
            assert want == []
        for steps in (("all",), ("ones",), ("random",), ("two windows at once",)):
            rel = WindowRelease(embed, chunk)
            got, t = [], 0
            while t < T:
                d = {"all": T, "ones": 1, "random": rng.randint(0, stride + 3), "two windows at once": 2 * stride}[steps[0]]
                d = min(d, T - t)
                new = rel.push(d)
                t += d
                # a released window is full, not the last one, and lies within the frames that exist
                assert all(ln == window and not fin and st + stride + ctx <= t for st, ln, fin in new)
                if steps[0] == "two windows at once" and d == 2 * stride and t >= 3 * stride + ctx:
                    assert len(new) == 2
                got += new
            last = rel.finish()
            assert len(last) <= 1
            assert got + last == want, (T, steps, got + last, want)


def test_window_release_refuses_use_after_finish_and_restarts_on_reset():
    from paper_accurate_fast_cheap_amd.utils.audio_stream import WindowRelease
    embed = SimpleNamespace(subsampling_rate=4, right_context=6)
    rel = WindowRelease(embed, 16)
    assert rel.push(198) == [(0, 67, False), (64, 67, False)]      # window 2 is full at 195 frames, released at 128 + 64 + 7
    assert rel.push(1) == [(128, 67, False)]
    assert rel.finish() == [(192, 7, True)]
    with pytest.raises(AssertionError):
        rel.push(1)
    rel.reset()
    assert rel.push(70) == [] and rel.finish() == [(0, 67, True)]
    with pytest.raises(ValueError):
        WindowRelease(embed, 0)


def test_host_pieces_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The pure host pieces of the fbank entry points (frame arithmetic, carry plan, argument validation) as a stand-alone
    program with its own main, built with -fsanitize=address,undefined for the host and run here, on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fbank_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fbank_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("sanitize" in built.stderr.lower() or "asan" in built.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "fbank host check ok" in run.stdout
