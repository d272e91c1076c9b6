"""The three kernels of the fp32 GEMM (csrc/gemm_f32.hip: pafc_gemm_f32) at small shapes, against float64.

pafc_gemm_f32 computes act(alpha A W^T + bias + residual) -- the activation AFTER the residual -- with one of three kernels:
the staged 128 x 128 tile (K-steps of 32), the staged 64 x 64 tile (K-steps of 64) and the few-rows 32 x 32 kernel whose four
waves split K.  PAFC_GEMM_F32_KERNEL (1 / 2 / 3), which the library reads on every call, forces one; unset, the plan picks from
M, N, batch and the CU count.  Calls go through the bound library with the layout of tests/gemm_launch.py (launch_f32):
operand rows wider than K with NaN in the padding, the output inside a sentinel-filled buffer with 64 guard rows per batch
entry and ldo > N, the residual in a buffer of its own with another leading dimension or in place, batch entries further
apart than one entry.

Two yardsticks, no tolerance of this file's own:
  * grid operands (gemm_ref.make_grid_operands, fp32 form; act "none"): every sum is an fp32 number in any order, so the
    result equals gemm_ref.round_to(form, ideal) BIT FOR BIT -- the row and column walks, the K walks, the batch, the plan;
  * random operands (gemm_ref.make_operands, fp32 form) at K <= 384: err / gemm_ref.bound <= 1 with the accumulation constant
    of fp32 operands, (2 Kw + 8) u -- every activation with bias and residual, bias alone, neither.
Every case: rc == 0, a finite result, every sentinel intact.  Which kernel an unforced call takes is not observed:
`planned_kernel` restates the documented rule, and test_the_plan_reaches_all_three_kernels asserts that its cases reach all
three on the card at hand.  Per family the parity log gets the kernel and "exact" or the worst err / bound."""
import functools
from collections import namedtuple

import pytest
import torch

from tests import gemm_launch, gemm_ref, parity_log
from tests.gemm_ref import Form

pytestmark = pytest.mark.gpu

KERNELS = {1: "128x128 staged", 2: "64x64 staged", 3: "32x32 few rows"}
EDGE = {1: 128, 2: 64, 3: 32}                  # the tile edge B
KSTEP = {1: 32, 2: 64}                         # K-step of the staged kernels
PAD = 20                                       # floats of NaN behind every operand row (a multiple of 4, not of the K-steps)
ACTS = ["none", "silu", "tanh", "relu"]

# kernel: forced through the environment (None: the plan); res: None | "sep" | "inplace"; batch: 0 = one problem
Case = namedtuple("Case", "kernel M N K act bias res pad grid batch shared_bias", defaults=("none", True, None, 0, True, 0, False))


def _cdiv(a, b):
    return -(-a // b)


def planned_kernel(M, N, batch, cus, forced=None):
    """The documented rule of pafc_gemm_f32: 128 x 128 tiles once they give every CU a block; the few-rows kernel when the
    64 x 64 tiles would leave three quarters of the CUs idle; else 64 x 64."""
    Z = max(batch, 1)
    if forced == 1 or (not forced and _cdiv(M, 128) * _cdiv(N, 128) * Z >= cus):
        return 1
    if forced == 3 or (not forced and 4 * _cdiv(M, 64) * _cdiv(N, 64) * Z <= cus):
        return 3
    return 2


def form_of(case):
    return Form(False, "f32", case.act, "f32" if case.res else None)


def _alpha(case):
    return 0.5 if case.res else 1.0


# ---- the case lists -------------------------------------------------------------------------------------------------------
def cases_row_walk(kernel):
    """M in {1, B - 1, B, B + 1, 2 B + 7} at N = 2 B + 7 and N in {1, B - 1, B, B + 1} at M = 2 B + 7; each with and without
    padded rows, and with no residual, a separate residual (alpha 0.5) and a residual in place.  K = 100: not a multiple of
    either K-step."""
    B = EDGE[kernel]
    top = 2 * B + 7
    shapes = [(m, top) for m in (1, B - 1, B, B + 1, top)] + [(top, n) for n in (1, B - 1, B, B + 1)]
    return [Case(kernel, m, n, 100, res=res, pad=pad) for m, n in shapes for pad in (0, PAD) for res in (None, "sep", "inplace")]


def cases_k_walk(kernel):
    B = EDGE[kernel]
    if kernel in KSTEP:
        # 1 to 5 K-steps, the last holding KS, 4, KS / 2, KS / 2 + 4 and KS - 4 columns: both LDS stages, the step that
        # fetches nothing more, the lane-half border of the K permutation
        KS = KSTEP[kernel]
        ks = sorted({KS * (steps - 1) + last for steps in range(1, 6) for last in (KS, 4, KS // 2, KS // 2 + 4, KS - 4)})
    else:
        # K-steps of 64 over four waves and two register sets: a wave with no step, 1 to 5 steps per wave, every branch of
        # the two-set loop (last step of 4 columns), the full multiples, and the half-lane border at K % 64 = 28, 32, 36
        ks = [64 * steps - 60 for steps in (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17)] + [64 * steps for steps in (4, 8, 16)]
        ks += [64 * full + r for full in (1, 4) for r in (28, 32, 36)]
    return [Case(kernel, B + 1, B + 1, K, res="sep", pad=PAD) for K in ks]


def cases_batch(kernel):
    B = EDGE[kernel]
    return [Case(kernel, B + 1, B + 1, 100, res=res, pad=PAD, batch=3, shared_bias=sb)
            for sb in (False, True) for res in ("sep", "inplace")]


def cases_random(kernel, act):
    """M = N = 2 B + 7, K in {36, 384}: bias and residual (alpha 0.5), bias alone, neither; and batch 2 once."""
    top = 2 * EDGE[kernel] + 7
    cases = [Case(kernel, top, top, K, act=act, bias=bias, res=res, pad=PAD, grid=False)
             for K in (36, 384) for bias, res in ((True, "sep"), (True, None), (False, None))]
    return cases + [Case(kernel, top, top, 36, act=act, res="inplace", pad=PAD, grid=False, batch=2)]


def cases_plan(cus):
    """Single-tile shapes; the batch count decides: about `cus` entries give every CU a 128 x 128 block, cus / 4 + 1 are too
    many for the few-rows rule, one entry takes the few-rows kernel."""
    return [Case(None, 40, 40, 100, res="sep", pad=PAD, batch=Z) for Z in (cus, cus // 4 + 1, 0)]


def grid_problems(cus=256):
    """(M, N, K, batch, alpha) of every case judged bit for bit (tests/test_gemm_ref.py checks that fp32 holds them)."""
    for k in KERNELS:
        for c in cases_row_walk(k) + cases_k_walk(k) + cases_batch(k):
            yield c.M, c.N, c.K, c.batch, _alpha(c)
    for c in cases_plan(cus):
        yield c.M, c.N, c.K, c.batch, _alpha(c)


def random_problems():
    """(act, M, N, K, batch, bias, residual) of every case judged by the bound."""
    for k in KERNELS:
        for act in ACTS:
            for c in cases_random(k, act):
                yield c.act, c.M, c.N, c.K, c.batch, c.bias, c.res is not None


# ---- operands, shared among the cases that slice them -----------------------------------------------------------------
RES_FORM = Form(False, "f32", "none", "f32")


def make_ops(act, rows, N, K, grid, batch, shared_bias, device):
    """The problem with a residual, alpha 0.5; `variant` derives the others from it."""
    form = Form(False, "f32", act, "f32")
    seed = 1000 * K + N + 7 * batch
    if grid:
        ops = gemm_ref.make_grid_operands(form, rows, N, K, seed=seed, alpha=0.5, device=device, f32_operands=True, batch=batch,
                                          shared_bias=shared_bias)
    else:
        ops = gemm_ref.make_operands(form, rows, N, K, seed=seed, batch=batch, alpha=0.5, shared_bias=shared_bias, device=device,
                                     f32_operands=True)
    ops["act_after_residual"] = True
    gemm_ref.products(form, ops)
    return ops


def variant(ops, bias, res):
    """The same product without the residual (alpha 1) and without the bias."""
    out = dict(ops)
    if not res:
        out["residual"], out["alpha"] = None, 1.0
    if not bias:
        out["bias"] = None
    return out


@functools.lru_cache(maxsize=None)
def _operands(act, rows, N, K, grid, batch, shared_bias):
    return make_ops(act, rows, N, K, grid, batch, shared_bias, "cuda")


def _ops_of(case):
    cap = 2 * EDGE[case.kernel] + 7 if case.kernel else case.M
    if case.batch:
        ops = _operands(case.act, case.M, case.N, case.K, case.grid, case.batch, case.shared_bias)
    else:
        ops = gemm_ref.rows(_operands(case.act, cap, case.N, case.K, case.grid, 0, False), case.M)
    return variant(ops, case.bias, case.res)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(hip, monkeypatch, family, ident, cases):
    cus, kernels, worst, bad = _cus(), set(), 0.0, []
    for case in cases:
        if case.kernel is None:
            monkeypatch.delenv("PAFC_GEMM_F32_KERNEL", raising=False)
        else:
            monkeypatch.setenv("PAFC_GEMM_F32_KERNEL", str(case.kernel))
        form, ops = form_of(case), _ops_of(case)
        rc, got, clean, _ = gemm_launch.launch_f32(hip, form, ops, pad=case.pad, inplace=case.res == "inplace")
        if case.grid:
            problem, ratio = gemm_launch.judge_exact(form, ops, rc, got, clean), 0.0
        else:
            problem, ratio, _ = gemm_launch.judge(form, ops, rc, got, clean)
        kernel = KERNELS[planned_kernel(case.M, case.N, case.batch, cus, case.kernel)]
        print(f"{case}: {kernel} " + (problem or ("exact" if case.grid else "err/bound %.4g" % ratio)))
        kernels.add(kernel)
        worst = max(worst, ratio)
        if problem:
            bad.append((case, kernel, problem))
    verdict = "exact" if all(c.grid for c in cases) else "worst err / bound %.4g" % worst
    parity_log.record(f"gemm f32/{family}", **{ident: "; ".join(sorted(kernels)) + ": " + ("FAILED" if bad else verdict)})
    assert not bad, bad
    return kernels


# ---- the tests ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_row_and_column_walk(hip, monkeypatch, kernel):
    """Each forced kernel over M and N around its tile edge: one row, one column, a tile less one, a whole tile, one more,
    two tiles and a tail -- contiguous and NaN-padded operands, without a residual, with one of another leading dimension
    and with one in place.  Grid operands: bit for bit."""
    _run(hip, monkeypatch, "row and column walk", KERNELS[kernel], cases_row_walk(kernel))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_k_walk(hip, monkeypatch, kernel):
    """Staged kernels: 1 to 5 K-steps with a last step of KS, 4, KS / 2, KS / 2 + 4 and KS - 4 columns.  Few rows: the step
    counts that give a wave no step, 1 to 5 steps and every branch of the two-register-set loop, whole multiples of 64 and
    K % 64 around the lane-half border.  Grid operands: bit for bit."""
    _run(hip, monkeypatch, "K walk", KERNELS[kernel], cases_k_walk(kernel))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_batch_with_distinct_strides(hip, monkeypatch, kernel):
    """batch = 3 over grid.z: A, W and the residual with batch strides larger than one entry, the guarded output, the bias
    per entry and shared (strideBias = 0), the residual separate and in place."""
    _run(hip, monkeypatch, "batch 3", KERNELS[kernel], cases_batch(kernel))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_activations_on_random_operands(hip, monkeypatch, kernel, act):
    """Every activation behind bias and residual (alpha 0.5; the activation AFTER the residual), bias alone and neither, at
    K = 36 and 384 on M = N = 2 B + 7, and once with batch 2 over a residual in place: err / bound <= 1."""
    _run(hip, monkeypatch, "random operands", f"{KERNELS[kernel]}/{act}", cases_random(kernel, act))


def test_the_plan_reaches_all_three_kernels(hip, monkeypatch):
    """PAFC_GEMM_F32_KERNEL unset: single-tile problems whose batch count alone sends them to the 128 x 128 tile, the 64 x 64
    tile and the few-rows kernel by the documented rule on this card -- each exact."""
    cus = _cus()
    cases = cases_plan(cus)
    want = [planned_kernel(c.M, c.N, c.batch, cus) for c in cases]
    parity_log.record("gemm f32/plan coverage", cus=cus, kernels=[KERNELS[k] for k in want])
    assert sorted(want) == [1, 2, 3], (cus, want)
    assert _run(hip, monkeypatch, "plan", "unforced", cases) == set(KERNELS.values())
