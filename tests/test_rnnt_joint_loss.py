"""The fused RNN-T joint + loss (csrc/rnnt_loss.hip, hip_ops.rnnt_joint_loss, Transducer(transducer_type="fused_joint")):
checks that need no GPU -- the boundary's symbols and argument validation, the compiled kernels' instructions, and the model
layer's refusal to run the fused path where it cannot (and its default path left as it was)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc", "rnnt_loss.hip")
ERR_NULL, ERR_DIMS, ERR_UNSUP = -1, -2, -7


@pytest.fixture(scope="module")
def lib():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    so = build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT
    L = ctypes.CDLL(so)
    P, I, G, Z, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t, ctypes.c_float
    L.pafc_rnnt_joint_loss_workspace_bytes.restype = Z
    L.pafc_rnnt_joint_loss_workspace_bytes.argtypes = [I, I, I, G, G, P, I]
    L.pafc_rnnt_joint_loss_forward.argtypes = [I, I, I, I, I, P, G, G, P, G, G, P, P, P, P, P, I, I, G, P, P, Z, P]
    L.pafc_rnnt_joint_loss_backward.argtypes = [I, I, I, I, I, P, G, G, P, G, G, P, P, P, P, P, I, I, G, P, G, P, F, I, P, P, P, P,
                                                P, Z, P, Z, P]
    return L


def test_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "pafc_encoder_ops.h")).read()
    for name in ("pafc_rnnt_joint_loss_workspace_bytes", "pafc_rnnt_joint_loss_forward", "pafc_rnnt_joint_loss_backward"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name


def test_workspace_sizes_and_slab_plan(lib):
    B, J, V = 3, 640, 5000
    rows = [7 * 3, 5 * 1, 9 * 5]
    off = (ctypes.c_int64 * (B + 1))(0, rows[0], rows[0] + rows[1], sum(rows))
    R = sum(rows)
    fwd = lib.pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, 0, None, 0)
    assert fwd >= R * J * 2 + R * 40 * 8          # H + the per-tile row statistics
    assert lib.pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, max(rows), off, 1) > 0
    # one utterance with more rows than a slab may hold: no plan
    assert lib.pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, max(rows) - 1, off, 1) == 0
    assert lib.pafc_rnnt_joint_loss_workspace_bytes(0, J, V, R, 0, None, 0) == 0


def test_entry_points_validate_before_touching_the_device(lib):
    NULL = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)          # aligned, never dereferenced: validation fails first
    B, T, Up1, J, V, R = 2, 5, 4, 64, 40, 20

    def fwd(B=B, T=T, Up1=Up1, J=J, V=V, E=one, blank=0, R=R, nll=one, ws=one):
        return lib.pafc_rnnt_joint_loss_forward(B, T, Up1, J, V, E, J, T * J, one, J, Up1 * J, one, NULL, one, one, one, 3, blank, R,
                                                nll, ws, 1 << 40, NULL)

    assert fwd(E=NULL) == ERR_NULL
    assert fwd(nll=NULL) == ERR_NULL
    assert fwd(ws=NULL) == ERR_NULL
    assert fwd(B=0) == ERR_DIMS
    assert fwd(R=0) == ERR_DIMS
    assert fwd(blank=V) == ERR_DIMS
    assert fwd(J=96) == ERR_UNSUP                        # J % 64
    assert fwd(V=42) == ERR_UNSUP                        # V % 8
    assert fwd(Up1=4000) == ERR_UNSUP                    # the lattice's LDS

    off = (ctypes.c_int64 * 3)(0, 12, 20)

    def bwd(J=J, V=V, dE=one, grad=one, B=B, off=off):
        return lib.pafc_rnnt_joint_loss_backward(B, T, Up1, J, V, one, J, T * J, one, J, Up1 * J, one, NULL, one, one, one, 3, 0, R, off,
                                                 64, grad, 1.0, 1, dE, one, one, NULL, one, 1 << 40, one, 1 << 40, NULL)

    assert bwd(dE=NULL) == ERR_NULL
    assert bwd(grad=NULL) == ERR_NULL
    assert bwd(off=None) == ERR_NULL
    assert bwd(B=-1) == ERR_DIMS
    assert bwd(off=(ctypes.c_int64 * 3)(0, 12, 19)) == ERR_DIMS   # row_off[B] != R
    assert bwd(J=32) == ERR_UNSUP
    assert bwd(V=44) == ERR_UNSUP


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("asm") / "rnnt_loss.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.dirname(SRC), "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def _kernels(asm):
    parts = re.split(r"\n(?=_ZN4pafc[^\n]*:\s)", asm)
    return {p.split(":")[0]: p.split("s_endpgm")[0] for p in parts[1:]}


def test_gemm_kernels_run_on_the_matrix_cores_and_nothing_spills(asm):
    ks = _kernels(asm)
    gemms = {n: b for n, b in ks.items() if "rnnt_gemm_kernel" in n}
    assert len(gemms) == 2, sorted(ks)                  # row statistics and dz
    for name, body in gemms.items():
        assert re.search(r"v_mfma_f32_(16x16x32|32x32x16)_bf16", body), name
    assert any("rnnt_lattice_kernel" in n for n in ks)
    assert "scratch_" not in asm
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)
    assert spills and all(int(v) == 0 for v in spills)


def test_no_float_atomics_in_the_source():
    src = open(SRC).read()
    assert "atomicAdd" not in src and "atomic" not in re.sub(r"//[^\n]*", "", src)


class _TinyEncoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Linear(8, 16)

    def output_size(self):
        return 16

    def forward(self, x, lens, *a, **k):
        mask = (torch.arange(x.shape[1])[None, :] < lens[:, None]).unsqueeze(1)
        return self.proj(x), mask


def _model(**kw):
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    torch.manual_seed(0)
    V = 16
    joint_kw = kw.pop("joint_kw", {})
    return Transducer(V, 0, _TinyEncoder(), RNNPredictor(V, 8, 12, 0.0, 12, 1, dropout=0.0),
                      TransducerJoint(V, 16, 12, 64, **joint_kw), ctc=CTC(V, 16), ctc_weight=0.3, transducer_weight=0.7, **kw)


def _batch():
    return {"feats": torch.randn(2, 7, 8, generator=torch.Generator().manual_seed(3)), "feats_lengths": torch.tensor([7, 5]),
            "target": torch.tensor([[3, 4, 2], [5, -1, -1]]), "target_lengths": torch.tensor([3, 1])}


def test_fused_joint_on_cpu_tensors_raises():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    model = _model(transducer_type="fused_joint")
    with pytest.raises(PafcError, match="fused_joint.*GPU"):
        model(_batch(), torch.device("cpu"))


def test_fused_joint_refuses_a_joint_it_does_not_implement():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    model = _model(transducer_type="fused_joint", joint_kw=dict(postjoin_linear=True))
    with pytest.raises(PafcError, match="post-join"):
        model(_batch(), torch.device("cpu"))
    model = _model(transducer_type="fused_joint", joint_kw=dict(activation="relu"))
    with pytest.raises(PafcError, match="tanh"):
        model(_batch(), torch.device("cpu"))


@pytest.mark.parametrize("kw", [{}, {"transducer_type": "optimized_transducer"}, {"transducer_type": "warp-rnnt"}])
def test_other_transducer_types_keep_the_restated_path_bitwise(kw):
    want = _model()(_batch(), torch.device("cpu"))["loss_rnnt"]
    got = _model(**kw)(_batch(), torch.device("cpu"))["loss_rnnt"]
    assert torch.equal(got, want)
    assert not _model(**kw).fused_joint
