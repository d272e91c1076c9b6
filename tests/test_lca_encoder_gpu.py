"""The Conformer baseline's slot on the GPU: LimitedRelPositionMultiHeadedAttention against the fixtures captured from the
reference (tests/golden/make_goldens_lca.py), and a ConformerEncoder built with `limited_rel_selfattn` against the reference
encoder's forward and forward_chunk -- on the module path, without a library GEMM, and through the hipGraph cache.

Bounds.  The module in fp32: 8 x the error of the float32 CPU restatement (tests/lca_ref.py) of the same case against the
float64 golden, the bound tests/test_attn_rescore_gpu.py uses for a kernels backend.  The encoder: `_assert_close`'s fp32
bound of tests/test_encoder_gpu.py, restated below."""
import pytest
import torch

from tests import lca_ref, parity_log, synth
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def _assert_close_fp32(got, ref, what):
    """tests/test_encoder_gpu.py:_assert_close, fp32 path: 1e-3 relative with an absolute floor for values near zero."""
    got, ref = got.float().cpu(), ref.float().cpu()
    d = (got - ref).abs()
    parity_log.record(f"golden/{what}", max_abs_err=float(d.max()), mean_abs_err=float(d.mean()),
                      ref_abs_max=float(ref.abs().max()), mode="fp32")
    tol = 1e-3 * ref.abs().clamp_min(5e-2)
    assert bool((d <= tol).all()), f"{what}: max {float(d.max()):.4g} mean {float(d.mean()):.4g}"


def _module(g, w):
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    m = WENET_ATTENTION_CLASSES["limited_rel_selfattn"](g["heads"], g["d"], 0.1, True, [w, w], 0, 1, False, 0)   # (dropout: a no-op in eval)
    m.load_state_dict(synth.synth_state_dict(g["spec"], g["weight_seed"]), strict=True)
    return m.cuda().eval()


def test_module_against_every_attention_golden(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    g = load_golden("lca_attention")
    sd32 = synth.synth_state_dict(g["spec"], g["weight_seed"])
    empty = torch.zeros((0, 0, 0, 0), device="cuda")
    for c in g["cases"]:
        w, B, T = c["w"], c["B"], c["T"]
        m = _module(g, w)
        x = synth.randn((B, T, g["d"]), c["seed"])
        pos = g["pos_rows"][:, :T]
        mask = (torch.arange(T)[None, :] < torch.tensor(c["lens"])[:, None]).unsqueeze(1)
        cpu, _ = lca_ref.lca_attention(x, pos, sd32, g["heads"], w)                       # the float32 restatement
        yard = (cpu.double() - c["out"]).abs().max().item()
        with torch.no_grad():
            y, cache = m(x.cuda(), x.cuda(), x.cuda(), mask.cuda(), pos.cuda(), empty)
            w_qkv, b_qkv = m._stacked_qkv()
            qkv = hip_ops.linear_fused(x.cuda().reshape(B * T, -1), w_qkv, b_qkv, "none", split_ok=False)
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and tuple(y.shape) == (B, T, g["d"]) and tuple(cache.shape) == c["cache_shape"]
        err = (y.double().cpu() - c["out"]).abs().max().item()
        print(f"lca module w={w} B={B} T={T}: max|err| {err:.3e}, float32 CPU restatement {yard:.3e}")
        parity_log.record(f"lca_module_w{w}_B{B}_T{T}", max_abs_err=err, cpu_float32_err=yard)
        assert yard > 0 and err <= 8 * yard, (w, B, T, err, yard)
        # the returned cache is cat(k, v) of the module's own projections, bit for bit, in the reference's layout
        D = g["d"]
        k = qkv[:, D:2 * D].view(B, T, g["heads"], -1).transpose(1, 2)
        v = qkv[:, 2 * D:].view(B, T, g["heads"], -1).transpose(1, 2)
        assert torch.equal(cache, torch.cat((k, v), dim=-1))
        assert (cache[:, :, c["cache_frames"]].double().cpu() - c["cache_at"]).abs().max().item() <= 1e-4


def test_bf16_module_runs_and_is_recorded(hip):
    """A whole-model-bf16 module through the bf16 GEMMs and the bf16 attention kernel: finite, of the right dtype and shape.  No
    bound for a bf16 stack against the float64 golden of the fp32 weights is derived here (the kernel's own bf16 bound is in
    tests/test_mha_band_gpu.py), so the difference is recorded, not asserted."""
    g = load_golden("lca_attention")
    c = next(c for c in g["cases"] if (c["w"], c["T"]) == (16, 67) and c["B"] == 2)
    m = _module(g, 16).to(torch.bfloat16)
    x = synth.randn((2, 67, g["d"]), c["seed"]).cuda().to(torch.bfloat16)
    with torch.no_grad():
        y, cache = m(x, x, x, torch.ones(2, 1, 67, dtype=torch.bool, device="cuda"), g["pos_rows"].cuda().to(torch.bfloat16))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 67, g["d"]) and tuple(cache.shape) == c["cache_shape"]
    assert torch.isfinite(y.float()).all()
    parity_log.record("lca_module_bf16_w16_B2_T67", max_abs_diff=(y.double().cpu() - c["out"]).abs().max().item())


def test_module_is_inference_only_and_takes_no_cache(hip):
    g = load_golden("lca_attention")
    m = _module(g, 5)
    x, pos = torch.zeros(1, 7, g["d"], device="cuda"), torch.zeros(1, 7, g["d"], device="cuda")
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x, x, x, torch.ones(1, 1, 7, dtype=torch.bool, device="cuda"), pos)
    with torch.no_grad():
        with pytest.raises(ValueError, match="cache"):
            m(x, x, x, torch.ones(1, 1, 7, dtype=torch.bool, device="cuda"), pos, torch.zeros(1, 2, 3, 128, device="cuda"))
        with pytest.raises(ValueError, match="pos_emb"):
            m(x, x, x, torch.ones(1, 1, 7, dtype=torch.bool, device="cuda"), pos[:, :6])
        y, _ = m(x, x, x, torch.ones(1, 1, 7, dtype=torch.bool, device="cuda"), pos)
    assert torch.isfinite(y).all()


def test_rows_are_independent_and_padded_frames_are_keys(hip):
    """Row b of a batched call equals that row run alone with the same T, bit for bit.  The reference applies no length mask:
    changing the values of the frames beyond a row's length changes that row's valid frames within w of the boundary and no
    others -- asserted so that nobody "fixes" it."""
    g = load_golden("lca_attention")
    w, B, T, n = 5, 3, 40, 23                                              # row 1 has n valid frames
    m = _module(g, w)
    x = synth.randn((B, T, g["d"]), 77).cuda()
    pos = lca_ref.position_rows(3, T, g["d"], torch.float32).cuda()
    mask = torch.ones(B, 1, T, dtype=torch.bool, device="cuda")
    mask[1, :, n:] = False
    with torch.no_grad():
        y, cache = m(x, x, x, mask, pos)
        for b in range(B):
            yb, cb = m(x[b:b + 1], x[b:b + 1], x[b:b + 1], mask[b:b + 1], pos)
            assert torch.equal(yb[0], y[b]) and torch.equal(cb[0], cache[b]), b
        x2 = x.clone()
        x2[1, n:] = synth.randn((T - n, g["d"]), 78).cuda() * 3
        y2, _ = m(x2, x2, x2, mask, pos)
    changed = (y2 != y).any(dim=-1).cpu()                                   # (B, T)
    assert not changed[0].any() and not changed[2].any()
    assert changed[1, n - w:n].all() and not changed[1, :n - w].any()


@pytest.fixture(scope="module")
def lca_encoder():
    from paper_accurate_fast_cheap_amd.transformer.cmvn import GlobalCMVN
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_lca")
    sd = synth.synth_state_dict(g["spec"], g["seed"])
    assert abs(synth.checksum(sd) - g["checksum"]) <= 1e-6 * g["checksum"]
    enc = ConformerEncoder(80, global_cmvn=GlobalCMVN(torch.zeros(80), torch.ones(80)), **g["conf"])
    enc.load_state_dict(sd)                # strict: every reference key present, nothing extra
    xs = synth.randn((3, 135, 80), g["xs_seed"], 2.0).cuda()
    xc = synth.randn((1, 63, 80), g["chunk_seed"], 2.0).cuda()
    return g, enc.cuda().eval(), xs, xc


def test_encoder_forward_and_chunk_against_the_reference(hip, lca_encoder):
    g, enc, xs, xc = lca_encoder
    with torch.no_grad():
        assert enc._fused(xs) is None                                       # no fused schedule for this slot: the module path
        out, masks = enc(xs, g["lens"].cuda())
        assert torch.equal(masks.cpu(), g["masks"]) and out.dtype == torch.float32
        _assert_close_fp32(out, g["out"], "encoder_lca/out")
        yc, att, cnn = enc.forward_chunk(xc, g["chunk_offset"], -1)
        _assert_close_fp32(yc, g["chunk_y"], "encoder_lca/chunk")
        assert att.shape == g["chunk_att_cache"].shape and tuple(cnn.shape) == g["cnn_cache_shape"]
        _assert_close_fp32(att, g["chunk_att_cache"], "encoder_lca/chunk_att_cache")
        yc4, att4, _ = enc.forward_chunk(xc, g["chunk_offset"], 4)            # required_cache_size 4: the last 4 frames
        assert torch.equal(yc4, yc) and att4.shape == g["chunk_att_cache_r4"].shape and torch.equal(att4, att[:, :, -4:])
        assert enc.forward_chunk(xc, g["chunk_offset"], 0)[1].size(2) == 0
        with pytest.raises(ValueError, match="cache"):                      # a non-empty attention cache is refused
            enc.forward_chunk(xc, g["chunk_offset"] + 15, -1, att_cache=att)


def test_encoder_graph_replay_equals_eager_bit_for_bit(hip, lca_encoder):
    g, enc, xs, _ = lca_encoder
    lens = g["lens"].cuda()
    with torch.no_grad():
        eager, emask = enc(xs, lens)
        enc.graph_cache_size = 2
        try:
            for _ in range(3):                                              # seen, captured (and replayed), replayed
                got, gmask = enc(xs, lens)
            assert any(isinstance(v, tuple) for v in enc._graphs.values()), "the shape was not captured"
        finally:
            enc.graph_cache_size = 0
            enc._graphs.clear()
    torch.cuda.synchronize()
    assert torch.equal(got, eager) and torch.equal(gmask, emask)


def test_encoder_pass_calls_no_library_gemm(hip, lca_encoder, monkeypatch):
    """Under torch.profiler the pass lists no library GEMM kernel (rocBLAS / hipBLASLt "Cijk_", at::native gemm / gemv), and
    F.linear / torch.matmul / torch.bmm are not called at all: the attention runs in mha_band_kernel."""
    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile
    g, enc, xs, _ = lca_encoder
    lens = g["lens"].cuda()
    with torch.no_grad():
        want, _ = enc(xs, lens)                                             # (warm: stacked weights, library load)

        def refuse(*a, **k):
            raise AssertionError("a library GEMM was called in the encoder pass")
        monkeypatch.setattr(F, "linear", refuse)
        monkeypatch.setattr(torch, "bmm", refuse)
        monkeypatch.setattr(torch, "matmul", refuse)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            got, _ = enc(xs, lens)
            torch.cuda.synchronize()
    assert torch.equal(got, want)
    names = [e.key for e in prof.key_averages()]
    assert any("mha_band_kernel" in n for n in names), names
    bad = [n for n in names if "Cijk_" in n or ("gemm" in n.lower() and "at::native" in n)
           or n in ("aten::mm", "aten::addmm", "aten::bmm")]
    assert not bad, bad


def test_init_model_decodes_with_the_shipped_encoder_conf(hip):
    """init_model builds the shipped conf/conformer YAML's encoder_conf (global_tokens: 0) unchanged and
    decode(["ctc_greedy_search"]) runs on it."""
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    from tests.test_lca_attention import SHIPPED_ENCODER_CONF
    torch.manual_seed(5)
    configs = dict(input_dim=80, output_dim=50, encoder="conformer", encoder_conf=dict(SHIPPED_ENCODER_CONF), ctc="ctc",
                   ctc_conf=dict(ctc_blank_id=0), model="asr_model", model_conf=dict(ctc_weight=1.0))

    class Args:
        checkpoint = None
    model, _ = init_model(Args(), configs)
    model = model.cuda().eval()
    speech = synth.randn((2, 2100, 80), 6).cuda()                           # T' = 524 > 2 w: a band that does not cover everything
    with torch.no_grad():
        res = model.decode(["ctc_greedy_search"], speech, torch.tensor([2100, 1500]).cuda())
    assert len(res["ctc_greedy_search"]) == 2
