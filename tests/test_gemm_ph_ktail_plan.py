"""The tail plan of the phase-pipelined GEMM (hip_ops._ph_ktail_plan, mirrored by csrc/gemm_bf16.hip:
pafc_gemm_ph_ktail_plan), CPU only: which split-operand problems run the row tiles of their last, short round of
one-tile-per-CU work once per half of K (pafc_gemm_ph_ktail) -- a pure function of (M, N, K, CU count)."""
import ctypes
import os

import pytest

from paper_accurate_fast_cheap_amd.hip_ops import DISPATCH, _ph_ktail_plan

MIN_K = 1024                 # the threshold the plan started from; the cases hold at it and at the measured one
CASES = [
    # (M, N, K, cus) -> plan
    ((44998, 512, 2048, 256), (32768, 2)),       # w_2 of the 30-minute sequence: 352 tiles, one full round + 96
    ((44998, 512, 9728, 256), (32768, 2)),       # Linear(9728, 512) after the subsampling convolutions
    ((44998, 2048, 512, 256), None),             # w_1: K too short
    ((44998, 512, 512, 256), None),              # pointwise_conv2: K too short
    ((16000, 512, 2048, 256), None),             # one round: full == 0
    ((65536, 512, 2048, 256), None),             # 512 tiles: tail == 0
    ((51000, 512, 2048, 256), None),             # 400 tiles: tail 144, 2 x tail > cus
    ((44998, 512, 2048 + 64, 256), None),        # K / 32 = 66: not a multiple of 4
    ((44998, 512, 2048 + 32, 256), None),        # K / 32 = 65
]


@pytest.mark.parametrize("shape,want", CASES, ids=["%dx%dx%d@%d" % c[0] for c in CASES])
def test_plan_at_fixed_cu_counts(shape, want):
    M, N, K, cus = shape
    assert _ph_ktail_plan(M, N, K, cus, min_k=MIN_K) == want
    assert _ph_ktail_plan(M, N, K, cus) == want                  # ... and at the threshold the table ships with


def test_threshold_comes_from_the_dispatch_table():
    assert _ph_ktail_plan(44998, 512, 2048, 256, min_k=4096) is None
    assert _ph_ktail_plan(44998, 512, 2048, 256, min_k=2048) == (32768, 2)
    assert _ph_ktail_plan(44998, 512, 2048, 256) == _ph_ktail_plan(44998, 512, 2048, 256, min_k=DISPATCH["ktail_min_k"])
    assert _ph_ktail_plan(44998, 512, 2048, 256, batch=2, min_k=MIN_K) is None


def _invariants(M, N, K, cus, plan):
    if plan is None:
        return
    split_row, kslices = plan
    ntiles = (N + 255) // 256
    tiles = ((M + 255) // 256) * ntiles
    assert kslices == 2
    assert split_row % 256 == 0 and 0 < split_row <= M
    assert (split_row // 256) * ntiles % cus == 0                       # whole rounds in front of the split
    tail = tiles - (split_row // 256) * ntiles
    assert 0 < tail and 2 * tail <= cus                                 # the slices of the tail fit one round
    assert (K // 32) % 4 == 0 and K >= MIN_K


@pytest.mark.parametrize("cus", [64, 304, 256, 1])
def test_other_cu_counts(cus):
    hits = 0
    for M in list(range(1, 3000, 37)) + [16000, 44998, 65536, 100000, 77825]:
        for N in (8, 264, 512, 1000, 2048):
            for K in (1024, 2048, 9728):
                plan = _ph_ktail_plan(M, N, K, cus, min_k=MIN_K)
                _invariants(M, N, K, cus, plan)
                hits += plan is not None
    assert hits > 0 or cus == 1                                          # (one CU: every round is full)


@pytest.fixture(scope="module")
def so_path():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    return build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT


def test_the_library_plans_as_python_does(so_path):
    """pafc_gemm_ph_ktail_plan with the CU count given is host arithmetic: no GPU call."""
    from paper_accurate_fast_cheap_amd import _lib
    L = _lib._bind(ctypes.CDLL(so_path))
    row = ctypes.c_long(-1)
    shapes = [c[0] for c in CASES] + [(M, N, K, cus) for M in (257, 582, 20000, 44998, 77825, 100000) for N in (264, 512, 1000)
                                      for K in (512, 1024, 2048 + 64, 9728) for cus in (64, 256, 304)]
    for M, N, K, cus in shapes:
        for min_k in (MIN_K, 4096):
            ks = L.pafc_gemm_ph_ktail_plan(M, N, K, 1, cus, min_k, ctypes.byref(row))
            want = _ph_ktail_plan(M, N, K, cus, min_k=min_k)
            assert ((row.value, ks) if ks else None) == want, (M, N, K, cus, min_k)
            assert ks or row.value == 0
    assert L.pafc_gemm_ph_ktail_plan(44998, 512, 2048, 2, 256, MIN_K, ctypes.byref(row)) == 0        # batch > 1: no plan
