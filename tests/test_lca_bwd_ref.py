"""The analytic backward of limited-context attention (tests/lca_bwd_ref.py) on the CPU, in float64: against autograd through
tests/lca_ref.band_attention on every case of the GPU test's list, with four planted faults that it must notice; the module
restatement's float64 autograd against gradients captured from the reference's own module
(tests/golden/make_goldens_lca_train.py); and the switch that lets the Conformer baseline's slot train.

"Relative" is max |a - b| over max |b| of the gradient compared, with a floor of 1e-3 under max |b|: with w = 0 a query sees
itself alone, P = 1 and dS = 0, so dq, dk, dp, du and dvb are zero in exact arithmetic and rounding noise in float64."""
import pytest
import torch

from tests import lca_bwd_ref, lca_ref, synth
from tests.conftest import load_golden

NAMES = ("dq", "dk", "dv", "dp", "du", "dvb")


def _autograd(q, k, v, p, u, vb, dout, w, t_pad):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, p, u, vb)]
    out = lca_ref.band_attention(*leaves, w, t_pad)
    return torch.autograd.grad(out, leaves, dout)


def _rel_errors(fault=None):
    """{(case, gradient name): relative error of the analytic backward against float64 autograd}"""
    errs = {}
    for n, (B, T, w, t_pad) in enumerate(lca_bwd_ref.CASES):
        t_pad = lca_bwd_ref.t_pad_of(T, w, t_pad)
        ins = lca_bwd_ref.case_inputs(B, T, 40 + n)
        want = _autograd(*ins, w, t_pad)
        got = lca_bwd_ref.band_attention_bwd(*ins, w, t_pad, fault=fault)
        for name, a, b in zip(NAMES, got, want):
            errs[(B, T, w, t_pad), name] = ((a - b).abs().max() / b.abs().max().clamp_min(1e-3)).item()
    return errs


def test_analytic_backward_equals_float64_autograd():
    for key, e in _rel_errors().items():
        assert e <= 1e-10, (key, e)


def test_lse_of_the_analytic_backward_is_the_log_denominator():
    """lse includes the padding keys' term: exp(lse) = sum_j exp(s_ij) + n0_i, checked through sum_j P_ij = 1 - n0_i e^-lse_i
    with P taken from the forward's output on a value of ones."""
    B, T, w, t_pad = 2, 67, 16, 96
    q, k, v, p, u, vb, dout = lca_bwd_ref.case_inputs(B, T, 3)
    lse = lca_bwd_ref.band_attention_bwd(q, k, v, p, u, vb, dout, w, t_pad)[-1]
    psum = lca_ref.band_attention(q, k, torch.ones_like(v), p, u, vb, w, t_pad)[..., 0]              # (B, T, H)
    n0 = (torch.clamp(torch.arange(T) + w, max=t_pad - 1) - T + 1).clamp(min=0).double().view(1, T, 1)
    assert n0.max() > 0
    assert (psum - (1 - n0 * torch.exp(-lse))).abs().max().item() <= 1e-12


@pytest.mark.parametrize("fault", lca_bwd_ref.FAULTS)
def test_planted_faults_are_noticed(fault):
    errs = _rel_errors(fault)
    assert any(not e <= 1e-10 for e in errs.values()), fault          # (a NaN counts as noticed)


def test_module_restatement_autograd_against_the_reference_gradients():
    """tests/lca_ref.lca_attention under float64 autograd against the gradients of the reference's module for x, pos_bias_u,
    pos_bias_v and linear_pos.weight, to 1e-9 relative."""
    g = load_golden("lca_attention_grad")
    att = load_golden("lca_attention")
    assert g["weight_seed"] == att["weight_seed"] and len(g["cases"]) == 2
    assert {(c["w"], c["B"], c["T"]) for c in g["cases"]} == {(16, 2, 67), (16, 2, 32)}
    for c in g["cases"]:
        w, B, T = c["w"], c["B"], c["T"]
        sd = {k: v.double().requires_grad_(True) for k, v in synth.synth_state_dict(att["spec"], att["weight_seed"]).items()}
        x = synth.randn((B, T, g["d"]), c["seed"]).double().requires_grad_(True)
        dy = synth.randn((B, T, g["d"]), c["seed"] + g["grad_seed_offset"]).double()
        y, _ = lca_ref.lca_attention(x, att["pos_rows"][:, :T].double(), sd, g["heads"], w)
        keys = ("pos_bias_u", "pos_bias_v", "linear_pos.weight")
        grads = torch.autograd.grad((y * dy).sum(), [x] + [sd[k] for k in keys])
        for name, got in zip(("dx",) + keys, grads):
            want = c[name]
            assert want.dtype == torch.float64 and want.abs().max() > 0
            e = ((got - want).abs().max() / want.abs().max()).item()
            assert e <= 1e-9, (w, B, T, name, e)


def test_encoder_built_slots_are_trainable_and_a_bare_module_is_not():
    from paper_accurate_fast_cheap_amd.transformer.attention import LimitedRelPositionMultiHeadedAttention
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = dict(load_golden("encoder_lca")["conf"])
    enc = ConformerEncoder(80, **conf)
    assert len(enc.encoders) > 0
    for layer in enc.encoders:
        assert isinstance(layer.self_attn, LimitedRelPositionMultiHeadedAttention) and layer.self_attn.trainable is True
    bare = LimitedRelPositionMultiHeadedAttention(2, 128, 0.0, True, [4, 4])
    assert bare.trainable is False and LimitedRelPositionMultiHeadedAttention.trainable is False
    x = torch.zeros(1, 7, 128)
    with pytest.raises(NotImplementedError, match="inference only"):
        bare(x, x, x, torch.ones(1, 1, 7, dtype=torch.bool), torch.zeros(1, 7, 128))


def test_training_entry_points_validate_before_they_launch():
    """pafc_mha_band_lse / pafc_mha_band_bwd answer bad arguments with a PAFC_ERR_* before any launch (the addresses are never
    dereferenced, so this runs without a GPU: the library builds here with hipcc; skipped only where neither hipcc nor a built
    library exists).  A library that is stale or lacks one of the symbols fails the test."""
    import ctypes
    import os
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)          # (a private handle)
    for name in ("pafc_mha_band_lse", "pafc_mha_band_bwd_workspace_bytes", "pafc_mha_band_bwd"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    check_band_bad_arguments(L)


def check_band_bad_arguments(L):
    import ctypes
    one, NULL, odd = ctypes.c_void_p(16), ctypes.c_void_p(0), ctypes.c_void_p(8)

    def lse(dtype=0, B=1, T=5, H=2, dk=64, w=2, t_pad=8, q=one, ld=128, stats=one):
        return L.pafc_mha_band_lse(dtype, B, T, H, dk, w, t_pad, q, ld, one, one, ld, one, ld, one, one, one, ld, stats, NULL)

    assert lse(q=NULL) == -1 and lse(stats=NULL) == -1 and lse(dtype=3) == -6 and lse(B=0) == -2 and lse(t_pad=4) == -2
    assert lse(dk=32) == -7 and lse(ld=120) == -2 and lse(ld=130) == -2 and lse(q=odd) == -8

    need = L.pafc_mha_band_bwd_workspace_bytes(1, 5, 2)
    assert need == 4 * (5 * 2 * 64 + 1 * 2 * 128) + 8 * 5 * 2
    assert L.pafc_mha_band_bwd_workspace_bytes(3, 131, 2) == 4 * (3 * 131 * 128 + 3 * 9 * 2 * 128) + 8 * 3 * 131 * 2
    assert L.pafc_mha_band_bwd_workspace_bytes(0, 5, 2) == 0 and L.pafc_mha_band_bwd_workspace_bytes(1, 0, 2) == 0
    assert L.pafc_mha_band_bwd_workspace_bytes(1, 5, 0) == 0

    def bwd(dtype=0, B=1, T=5, H=2, dk=64, w=2, t_pad=8, q=one, ld=128, lddo=128, lddkv=128, lddp=128, stats=one, dq=one, du=one,
            ws=one, nbytes=need):
        return L.pafc_mha_band_bwd(dtype, B, T, H, dk, w, t_pad, q, ld, one, one, ld, one, ld, one, one, one, ld, one, lddo, stats,
                                   dq, ld, one, one, lddkv, one, lddp, du, one, ws, nbytes, NULL)

    assert bwd(q=NULL) == -1 and bwd(stats=NULL) == -1 and bwd(dq=NULL) == -1 and bwd(du=NULL) == -1 and bwd(ws=NULL) == -1
    assert bwd(dtype=2) == -6 and bwd(B=0) == -2 and bwd(H=0) == -2 and bwd(T=0, t_pad=0) == -2 and bwd(w=-1) == -2
    assert bwd(t_pad=4) == -2                                                            # t_pad < T
    big = 65535 * 64                                                                     # the reduce launch's grid would not fit
    assert bwd(T=1 << 30, t_pad=1 << 30, H=65535, ld=big, lddo=big, lddkv=big, lddp=big) == -2
    assert bwd(dk=32) == -7 and bwd(H=1, dk=128) == -7                                   # PAFC_ERR_UNSUPPORTED: heads of 64 only
    assert bwd(ld=120) == -2 and bwd(lddo=130) == -2 and bwd(dtype=1, lddkv=132) == -2 and bwd(lddp=126) == -2
    assert bwd(q=odd) == -8 and bwd(dq=odd) == -8 and bwd(ws=odd) == -8
    assert bwd(nbytes=need - 1) == -4                                                    # PAFC_ERR_WORKSPACE
