"""CPU-only checks of the training-step CTC loss (csrc/ctc_loss.hip) and the first subsampling convolution's weight gradient
(csrc/conv_sub.hip): the compiled gfx950 code, the C boundary's limits, and that the module never routes to a call the boundary
refuses.  The numerics are checked on the GPU in test_train_loss_kernels_gpu.py."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc")
ERR_DIMS, ERR_WORKSPACE, ERR_DTYPE, ERR_UNSUP = -2, -4, -6, -7


def _asm(tmp_path_factory, name):
    src = os.path.join(CSRC, name)
    out = tmp_path_factory.mktemp("asm") / (name + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I",
                           os.path.join(ROOT, "include"), "-I", CSRC, "-S", "--cuda-device-only", src, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


@pytest.fixture(scope="module")
def ctc_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "ctc_loss.hip")


@pytest.fixture(scope="module")
def conv_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "conv_sub.hip")


def test_ctc_loss_has_no_float_atomics(ctc_asm):
    """The CTC input gradient adds occupancies in a fixed order: bitwise reproducible, like every other reduction here."""
    assert "ctc_grad_kernel" in ctc_asm and "ctc_lattice_kernel" in ctc_asm
    atomics = re.findall(r"^\s+((?:ds|global|flat|buffer)_(?:atomic_)?(?:add|pk_add|min|max)\w*_f(?:32|64)\w*)", ctc_asm, flags=re.M)
    atomics += re.findall(r"^\s+((?:ds|global|flat|buffer)_atomic_pk_add\w*)", ctc_asm, flags=re.M)
    assert not atomics, sorted(set(atomics))


@pytest.mark.parametrize("which", ["ctc_asm", "conv_asm"])
def test_train_loss_kernels_have_no_register_spills(which, request):
    asm = request.getfixturevalue(which)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)
    assert spills and all(int(v) == 0 for v in spills)
    assert "scratch_" not in asm


@pytest.fixture(scope="module")
def lib():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    P, I, G, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t
    L.pafc_ctc_loss_workspace_bytes.restype = Z
    L.pafc_ctc_loss_workspace_bytes.argtypes = [I, I, I]
    L.pafc_ctc_loss_forward.argtypes = [I, I, I, I, P, G, P, P, I, P, I, I, P, P, Z, P]
    L.pafc_ctc_loss_backward.argtypes = [I, I, I, I, P, G, P, P, I, P, I, I, P, P, F, P, G, P, Z, P]
    L.pafc_conv3x3s2_c1_wgrad_workspace_bytes.restype = Z
    L.pafc_conv3x3s2_c1_wgrad_workspace_bytes.argtypes = [I, I, I]
    L.pafc_conv3x3s2_c1_wgrad_bf16.argtypes = [I, I, I, I, P, P, P, P, P, Z, P]
    return L


ONE = ctypes.c_void_p(16)     # non-null, never dereferenced: every call below is refused before anything is launched


def _fwd(L, *, dtype=1, B=2, T=8, V=16, ldl=None, ldy=None, Lmax=4, ws=0):
    return L.pafc_ctc_loss_forward(dtype, B, T, V, ONE, V if ldl is None else ldl, ONE, ONE, Lmax if ldy is None else ldy, ONE,
                                   Lmax, 0, ONE, ONE, ws, None)


def _bwd(L, *, dtype=1, B=2, T=8, V=16, ldg=None, Lmax=4, ws=0):
    return L.pafc_ctc_loss_backward(dtype, B, T, V, ONE, V, ONE, ONE, Lmax, ONE, Lmax, 0, ONE, ONE, 1.0, ONE,
                                    V if ldg is None else ldg, ONE, ws, None)


def test_ctc_loss_forward_limits(lib):
    # the lattice keeps two fp64 time steps of 2 L + 3 entries in LDS, at most 120 KB: L <= 3838
    assert 2 * (2 * 3838 + 3) * 8 <= 120 * 1024 < 2 * (2 * 3839 + 3) * 8
    assert _fwd(lib, Lmax=3839) == ERR_UNSUP
    assert _fwd(lib, Lmax=3838) == ERR_WORKSPACE                   # accepted: next comes the (here too small) workspace
    assert _fwd(lib, dtype=5) == ERR_DTYPE
    assert _fwd(lib, B=65536) == ERR_DIMS
    assert _fwd(lib, B=65535) == ERR_WORKSPACE
    assert _fwd(lib, Lmax=4, ldy=3) == ERR_DIMS                    # ldy < max_target_len
    assert _fwd(lib, V=16, ldl=15) == ERR_DIMS


def test_ctc_loss_backward_limits(lib):
    assert _bwd(lib, V=38401, ldg=38464) == ERR_UNSUP              # one fp32 row of occupancies in LDS, at most 150 KB
    assert _bwd(lib, V=38400, ldg=38400) == ERR_WORKSPACE
    assert _bwd(lib, V=40, ldg=39) == ERR_DIMS                     # ldg < V
    assert _bwd(lib, dtype=5) == ERR_DTYPE
    assert _bwd(lib, B=65536) == ERR_DIMS


def test_ctc_loss_workspace_is_one_fp64_lattice_plus_row_statistics(lib):
    B, T, Lmax = 32, 499, 160
    Smax = 2 * Lmax + 1
    assert lib.pafc_ctc_loss_workspace_bytes(B, T, Lmax) == B * T * Smax * 8 + (B * T + B) * 4
    assert lib.pafc_ctc_loss_workspace_bytes(B, T, -1) == 0


def test_conv1_wgrad_limits(lib):
    def call(B=2, T=9, F=80, C=64, ws=None):
        n = lib.pafc_conv3x3s2_c1_wgrad_workspace_bytes(B, T, C) if ws is None else ws
        return lib.pafc_conv3x3s2_c1_wgrad_bf16(B, T, F, C, ONE, ONE, ONE, ONE, ONE, n, None)
    assert call(C=12) == ERR_DIMS                                  # C % 8
    assert call(C=24) == ERR_DIMS                                  # 256 % (C / 8)
    assert call(C=4096) == ERR_DIMS                                # C > 2048
    assert call(T=2) == ERR_DIMS
    assert call(F=2) == ERR_DIMS
    assert call(ws=lib.pafc_conv3x3s2_c1_wgrad_workspace_bytes(2, 9, 64) - 1) == ERR_WORKSPACE
    # one (10, C) fp32 partial per block of 32 output rows
    assert lib.pafc_conv3x3s2_c1_wgrad_workspace_bytes(31, 2000, 512) == (31 * 999 + 31) // 32 * 10 * 512 * 4


def _eligible(B, V, Lmax):
    from paper_accurate_fast_cheap_amd import hip_ops
    x = SimpleNamespace(is_cuda=True, shape=(B, 7, 64), dtype=torch.bfloat16, dim=lambda: 3)
    w = SimpleNamespace(shape=(V, 64), dtype=torch.bfloat16)
    ys = SimpleNamespace(shape=(B, Lmax), dim=lambda: 2)
    with torch.enable_grad():
        return hip_ops.ctc_head_loss_eligible(x, w, ys)


def test_ctc_head_loss_eligibility_lies_inside_the_boundary(lib, monkeypatch):
    """ctc_head_loss_eligible's edges, and one step past each: what the module routes to the kernels the C ABI accepts."""
    monkeypatch.delenv("PAFC_TRAIN_KERNELS", raising=False)
    monkeypatch.delenv("PAFC_TRAIN_CTC", raising=False)
    assert _eligible(32, 5000, 160)
    assert _eligible(65535, 38400, 3000)
    assert not _eligible(32, 38408, 160)
    assert not _eligible(32, 5000, 3001)
    assert not _eligible(65536, 5000, 160)
    # the largest eligible call passes every limit of both entry points (it stops only at the zero-byte workspace)
    assert _fwd(lib, B=65535, V=38400, Lmax=3000) == ERR_WORKSPACE
    assert _bwd(lib, B=65535, V=38400, Lmax=3000) == ERR_WORKSPACE
