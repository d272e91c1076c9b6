"""bench.py --dump-outputs: what the timed path computed, as float32 / float64 .npy files of at most 64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT


class _Result:
    def __init__(self, tokens):
        self.tokens = tokens


def test_sample_outputs_keeps_the_valid_frames_of_a_small_output_whole():
    import bench
    logp = torch.randn(2, 10, 7).bfloat16()
    a = bench.sample_outputs(logp, [10, 6], [[_Result([1, 2, 3]), _Result([])], [_Result([4])]])
    assert set(a) == {"ctc_log_probs", "ctc_log_probs_lengths", "tokens", "token_counts"}
    assert np.array_equal(a["ctc_log_probs"], torch.cat([logp[0], logp[1, :6]]).float().numpy())   # no padded frame
    assert a["ctc_log_probs_lengths"].tolist() == [10, 6]
    assert a["tokens"].tolist() == [1, 2, 3, 4] and a["token_counts"].tolist() == [3, 0, 1]
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())


def test_sample_outputs_samples_a_large_output_the_same_way_every_time():
    import bench
    logp = torch.randn(1, 9000, 5000)          # 180 MB of float32
    a, b = bench.sample_outputs(logp, [9000], None), bench.sample_outputs(logp.clone(), [9000], None)
    assert set(a) == {"ctc_log_probs", "ctc_log_probs_rows", "ctc_log_probs_lengths"}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["ctc_log_probs_rows"].astype(np.int64)
    assert len(rows) > 1000 and np.all(np.diff(rows) > 0) and rows[-1] < 9000
    assert np.array_equal(a["ctc_log_probs"], logp[0, rows].numpy())
    assert sum(x.nbytes for x in a.values()) + 128 * len(a) <= bench.DUMP_BYTES


def test_write_outputs(tmp_path):
    import bench
    arrays = {"ctc_log_probs": np.ones((3, 4), np.float32), "tokens": np.arange(5, dtype=np.float32)}
    shapes = bench.write_outputs(str(tmp_path / "d"), arrays)
    assert shapes == {"ctc_log_probs": [3, 4], "tokens": [5]}
    for name, x in arrays.items():
        assert np.array_equal(np.load(tmp_path / "d" / (name + ".npy")), x)


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(hip, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-extra",
           "--no-cpu-baseline", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    files = sorted(os.listdir(out))
    assert files == ["ctc_log_probs.npy", "ctc_log_probs_lengths.npy", "ctc_log_probs_rows.npy"]
    assert np.load(out / "ctc_log_probs_lengths.npy").tolist() == [44998]       # the 30-minute file, one sequence
    assert sum(os.path.getsize(out / f) for f in files) <= 64_000_000
    logp = np.load(out / "ctc_log_probs.npy")
    assert logp.dtype == np.float32 and logp.shape[1] == 5000 and np.isfinite(logp).all()
    assert np.allclose(np.exp(logp.astype(np.float64)).sum(1), 1.0, atol=1e-3)    # rows of a log-softmax
    assert line["dump_outputs"]["arrays"]["ctc_log_probs"] == list(logp.shape)
