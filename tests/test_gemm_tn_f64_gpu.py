"""The weight- and bias-gradient GEMM of the training step (csrc/gemm_tn.hip: pafc_gemm_tn_bf16[_batched]) at small shapes,
against float64.

dW = dY^T X and dbias = the column sums of dY, over R rows: a ring of four LDS-DMA stages of 64 rows, two K groups per block,
the rows past the end of a block's range zeroed in LDS, column tails clamped, blocks renumbered over the XCDs, R split over S
blocks per tile and a second kernel that adds the S partials of dW and of dbias.  Calls go through the bound library with
the layout of tests/gemm_launch.py (launch_tn): dy and x as column slices of wider NaN-filled buffers, dw, dbias and the
workspace each in front of 64 sentinels.  The split count is forced with PAFC_GEMM_TN_S, which the library reads on every
call; S = workspace_bytes / (4 batch M (N + 1)) is the only part of the plan it reports, and every case asserts that it is
what the documented arithmetic (gemm_ref.tn_plan) gives for the forced value.

Two yardsticks, no tolerance of this file's own:
  * grid operands (integers in [-3, 3]): every sum is an fp32 number, so the fp32 AND the bf16 outputs equal the exact value
    rounded once, bit for bit, dw and dbias alike -- ring fills, splits, the column walk, block renumbering, the batch;
  * random operands at R = 65 and 300: err / gemm_ref.bound <= 1 with the rounding count of gemm_ref.tn_problem.
Every case: rc == 0, finite results, every sentinel behind dw, dbias and the workspace intact."""
from collections import namedtuple

import pytest
import torch

from tests import gemm_launch, gemm_ref, parity_log
from tests.gemm_launch import ERR_ALIGNMENT, ERR_BAD_DIMS, ERR_WORKSPACE, SENTINEL

pytestmark = pytest.mark.gpu

OUTS = {"f32": torch.float32, "bf16": torch.bfloat16}
# s: the forced PAFC_GEMM_TN_S; bias: ask for dbias; batch: 0 = pafc_gemm_tn_bf16, else the batched entry
Case = namedtuple("Case", "R M N s bias batch grid", defaults=(1, True, 0, True))


def _cdiv(a, b):
    return -(-a // b)


def expected_S(case):
    """The S the library must report: a forced count the plan accepts (1 .. ceil(R / 128), at most 256) goes through the
    documented arithmetic."""
    assert 1 <= case.s <= min(256, max(1, _cdiv(case.R, 128))), case
    return gemm_ref.tn_plan(case.R, case.s)


def blocks_of(case):
    return _cdiv(case.M, 128) * _cdiv(case.N, 128) * expected_S(case)[0] * max(case.batch, 1)


RING_R = [1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 449, 512, 577]
WALK = [8, 120, 128, 136, 264]


def cases_ring_fills():
    """1 to 10 K-steps of one block against the four-stage ring, the last step holding 1, 63 or 64 rows."""
    return [Case(R, 136, 136) for R in RING_R]


def cases_splits():
    """R = 577: S = 4 leaves blocks of 192, 192, 192 and 1 rows, S = 3 ends on 65 rows."""
    return [Case(577, 136, 136, s=s) for s in range(1, 6)]


def cases_column_walk():
    shapes = [(m, 136) for m in WALK] + [(136, n) for n in WALK if n != 136]
    return [Case(129, m, n, bias=bias) for m, n in shapes for bias in (True, False)]


def cases_renumbering():
    """Fewer blocks than XCDs (1, 4), exactly 8 (all renumbered) and 18 (16 renumbered, 2 not); S = 2 at R = 129 gives the
    second split a single row."""
    return [Case(129, 8, 8), Case(129, 136, 136), Case(129, 136, 136, s=2), Case(129, 264, 264, s=2)]


def cases_batched():
    return [Case(300, 136, 72, s=2, batch=3)]


def cases_random():
    return [Case(R, 136, 72, s=s, batch=Z, grid=False) for R, s in ((65, 1), (300, 2)) for Z in (0, 2)]


def all_cases():
    return cases_ring_fills() + cases_splits() + cases_column_walk() + cases_renumbering() + cases_batched() + cases_random()


def make(case, device="cuda"):
    return gemm_ref.make_tn_operands(case.R, case.M, case.N, seed=1000 * case.R + case.M + case.N, batch=case.batch, grid=case.grid,
                                     device=device)


def _judge(case, out, dy, x, rc, S, dw, db, clean):
    """-> (problem or None, worst err / bound over dw and dbias (0 for grid cases))"""
    want_S, rps = expected_S(case)
    if rc != 0:
        return "rc %d" % rc, float("inf")
    if S != want_S:
        return "S = %d, the plan arithmetic gives %d" % (S, want_S), float("inf")
    form, ops_w, ops_b = gemm_ref.tn_problem(dy, x, out, S, rps)
    results = [(ops_w, dw.double())] + ([(ops_b, db.double().unsqueeze(-1))] if db is not None else [])
    worst = 0.0
    for ops, got in results:
        if case.grid:
            problem = gemm_launch.judge_exact(form, ops, rc, got, clean)
        else:
            problem, ratio, _ = gemm_launch.judge(form, ops, rc, got, clean)
            worst = max(worst, ratio)
        if problem:
            return ("dw: " if ops is ops_w else "dbias: ") + problem, worst
    return None, worst


def _run(hip, monkeypatch, family, cases, outs=("f32", "bf16")):
    worst, bad, splits = 0.0, [], set()
    for case in cases:
        monkeypatch.setenv("PAFC_GEMM_TN_S", str(case.s))
        dy, x = make(case)
        for out in outs:
            rc, dw, db, clean, S, _ = gemm_launch.launch_tn(hip, dy, x, OUTS[out], want_bias=case.bias)
            problem, ratio = _judge(case, out, dy, x, rc, S, dw, db, clean)
            print(f"{case} {out}: S={S} blocks={blocks_of(case)} " + (problem or ("exact" if case.grid else "err/bound %.4g" % ratio)))
            worst = max(worst, ratio)
            splits.add(S)
            if problem:
                bad.append((case, out, problem))
    verdict = "exact" if all(c.grid for c in cases) else "worst err / bound %.4g" % worst
    parity_log.record(f"gemm tn/{family}", S=sorted(splits), verdict="FAILED" if bad else verdict)
    assert not bad, bad


def test_ring_fills(hip, monkeypatch):
    """S = 1, 136 x 136 (four tiles with column tails): R from one row to ten K-steps -- a ring shorter than its four stages,
    exactly full, wrapped once and twice, the ragged last step of 1, 63 and 64 rows."""
    _run(hip, monkeypatch, "ring fills", cases_ring_fills())


def test_splits(hip, monkeypatch):
    """R = 577 with S = 1 .. 5 forced: unequal last blocks, one of a single row (S = 4), and the reducing kernel's quarter
    sums with fewer partials than quarters, as many, and more."""
    got = [expected_S(c) for c in cases_splits()]
    assert got == [(1, 640), (2, 320), (3, 256), (4, 192), (5, 128)] and 577 - 3 * 192 == 1 and 577 - 2 * 256 == 65
    _run(hip, monkeypatch, "splits", cases_splits())


def test_column_walk(hip, monkeypatch):
    """M and N in {8, 120, 128, 136, 264} against 136, with and without dbias: clamped column tails of dY and of X, the bias
    gradient at an M tail, and N of two and three tiles, of which only the first tile's blocks write the bias."""
    _run(hip, monkeypatch, "column walk", cases_column_walk())


def test_block_renumbering(hip, monkeypatch):
    cases = cases_renumbering()
    assert [blocks_of(c) for c in cases] == [1, 4, 8, 18]
    _run(hip, monkeypatch, "block renumbering", cases)


def test_batched_entries_and_repeatability(hip, monkeypatch):
    """Z = 3 at (300, 136, 72), strided entries, dbias: each entry against its own product, bit for bit, and a second call
    gives the same bits."""
    (case,) = cases_batched()
    _run(hip, monkeypatch, "batch 3", [case])
    dy, x = make(case)
    for out in OUTS.values():
        first = gemm_launch.launch_tn(hip, dy, x, out)
        again = gemm_launch.launch_tn(hip, dy, x, out)
        assert first[0] == 0 and again[0] == 0
        assert torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])


def test_random_operands(hip, monkeypatch):
    """R = 65 (S = 1) and 300 (S = 2) at 136 x 72, single and batch 2, fp32 and bf16 outputs: err / bound <= 1 for dw and dbias."""
    _run(hip, monkeypatch, "random operands", cases_random())


REFUSALS = [
    ("M = 4", dict(M=4), ERR_BAD_DIMS),
    ("M % 8", dict(M=132), ERR_BAD_DIMS),
    ("lda % 8", dict(lda=164), ERR_BAD_DIMS),
    ("lda < M", dict(lda=128), ERR_BAD_DIMS),
    ("misaligned dy", "dy", ERR_ALIGNMENT),
    ("workspace one byte short", "workspace_bytes", ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_every_buffer_alone(hip, monkeypatch, what, change, code):
    """What the entry refuses returns its documented error and launches nothing: dw, dbias and the workspace keep their
    sentinels from end to end.  (Every refused call describes operands inside the buffers it is given: 136 x 72, rows of 160.)"""
    monkeypatch.setenv("PAFC_GEMM_TN_S", "1")
    case = Case(129, 136, 72)
    dy, x = make(case)
    shifted = None
    if isinstance(change, dict):
        overrides = change
    elif change == "workspace_bytes":
        overrides = dict(workspace_bytes=4 * 136 * 73 - 1)
    else:
        from paper_accurate_fast_cheap_amd import _lib
        shifted = torch.zeros(129 * 160 + 8, dtype=torch.bfloat16, device="cuda")
        overrides = dict(dy=_lib.ptr(shifted[4:]))                                            # 8 bytes past a 16-byte boundary
    rc, _, _, _, S, (dw, db, ws) = gemm_launch.launch_tn(hip, dy, x, torch.float32, overrides=overrides)
    torch.cuda.synchronize()
    assert S == 1 and rc == code, (what, rc)
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all()) and bool((ws == SENTINEL).all()), what
