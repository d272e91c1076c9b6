"""Pin the CPU oracle: C recurrence vs independent closed forms, and the Python
restatement vs goldens captured from the reference's own modules
(tests/golden/make_goldens.py).  CPU only."""
import pytest
import torch

from oracle import encoder_oracle as EO
from oracle import wkv6_oracle as WO
from tests import synth
from tests.conftest import load_golden


torch.set_num_threads(4)  # the goldens were captured with 4 threads; with 4 the restatement is bit-identical here


def _close(a, b, bf16_path):
    """fp32 paths: 1e-3 relative (north_star's bar), in practice ~1e-6.  Paths that round to bf16 inside are
    chaotic at the bf16-ulp level under a mere change of GEMM summation order (thread count, CPU model):
    one flipped rounding is 2^-8 relative and is carried through the following layers, so they are held to
    a max / mean absolute bound measured across thread counts instead (values are O(1), max |x| ~ 4)."""
    a, b = a.float(), b.float()
    if torch.equal(a, b):
        return True
    d = (a - b).abs()
    if bf16_path:
        return bool(d.max() <= 0.1 and d.mean() <= 6e-3)
    return bool((d <= 1e-3 * b.abs().clamp_min(1e-2)).all())


def _bf16_model_gemms(monkeypatch):
    """The whole-model-bf16 goldens were captured on oneDNN's AMX bf16 GEMMs (bit-identical here with 4 threads).  Without
    AMX oneDNN takes other bf16 kernels that round differently (AVX512-BF16 on a Zen 5 EPYC: mean |diff| 6.3e-3 / 6.8e-3 on
    the two bf16-model cases, over _close's bound); ATen's own bf16 GEMM gives the same numbers on both CPUs (mean 5.3e-3 /
    3.7e-3), so the bf16 model runs on it there."""
    if not torch.cpu._is_amx_tile_supported():
        monkeypatch.setattr(torch.backends.mkldnn, "enabled", False)


def _sd(g, spec_key="spec", seed_key="seed", cs_key="checksum"):
    sd = synth.synth_state_dict(g[spec_key], g[seed_key])
    assert abs(synth.checksum(sd) - g[cs_key]) <= 1e-6 * g[cs_key], "synthetic weights drifted from capture time"
    return sd


# ---------------------------------------------------------------- WKV recurrence (C) vs closed forms
def _rand_rkvwu(B, T, C, H, seed):
    r, k, v = (synth.randn((B, T, C), seed + i, 0.5) for i in range(3))
    w = synth.randn((B, T, C), seed + 3) - 3.0
    u = synth.randn((H, C // H), seed + 4, 0.3)
    return r, k, v, w, u


@pytest.mark.parametrize("B,T,C,H", [(1, 1, 64, 1), (2, 37, 128, 2), (1, 65, 192, 3)])
def test_c_forward_matches_f64_closed_form(B, T, C, H):
    a = _rand_rkvwu(B, T, C, H, 100)
    y = WO.forward(*a)
    y64 = WO.forward_closed_form_f64(*a)
    assert (y.double() - y64).abs().max() <= 2e-6 * max(1.0, y64.abs().max())


def _torch_wkv_f64(r, k, v, w, u):
    B, T, C = r.shape
    H = u.shape[0]
    N = C // H
    r_, k_, v_ = (t.view(B, T, H, N) for t in (r, k, v))
    d = torch.exp(-torch.exp(w)).view(B, T, H, N)
    S = torch.zeros(B, H, N, N, dtype=r.dtype)
    ys = []
    for t in range(T):
        kv = k_[:, t, :, :, None] * v_[:, t, :, None, :]
        ys.append(torch.einsum("bhj,bhji->bhi", r_[:, t], u[None, :, :, None] * kv + S))
        S = S * d[:, t, :, :, None] + kv
    return torch.stack(ys, 1).reshape(B, T, C)


@pytest.mark.parametrize("B,T,C,H", [(2, 2, 64, 1), (2, 3, 64, 1), (2, 19, 128, 2)])
def test_c_backward_matches_autograd_f64(B, T, C, H):
    a = _rand_rkvwu(B, T, C, H, 200)
    gy = synth.randn((B, T, C), 209)
    leaves = [t.double().requires_grad_() for t in a]
    _torch_wkv_f64(*leaves).backward(gy.double())
    got = WO.backward(*a, gy)
    for name, g, leaf in zip("rkvwu", got, leaves):
        ref = leaf.grad
        if name == "w":
            # kernel_backward_201 defines gw[0] = gw[T-1] = 0 (wkv6_cuda.cu:236,262): w_0 only ever decays the
            # zero initial state and w_{T-1} decays a state nobody reads, so autograd agrees (both are 0)
            assert g[:, 0].abs().max() == 0 and g[:, -1].abs().max() == 0
        assert (g.double() - ref).abs().max() <= 3e-5 * max(1.0, ref.abs().max()), name


def test_c_bf16_is_f32_arithmetic_with_bf16_io():
    a = [t.bfloat16() for t in _rand_rkvwu(2, 31, 128, 2, 300)]
    y = WO.forward(*a)
    yf = WO.forward(*[t.float() for t in a])
    assert y.dtype == torch.bfloat16 and torch.equal(y, yf.bfloat16())


def test_c_state_carry_and_reverse():
    r, k, v, w, u = _rand_rkvwu(2, 40, 128, 2, 400)
    y = WO.forward(r, k, v, w, u)
    cut = lambda t, a, b: t[:, a:b].contiguous()
    y1, s1 = WO.forward(*(cut(t, 0, 17) for t in (r, k, v, w)), u, want_state=True)
    y2, s2 = WO.forward(*(cut(t, 17, 40) for t in (r, k, v, w)), u, s_in=s1, want_state=True)
    assert torch.equal(torch.cat([y1, y2], 1), y)
    _, s_full = WO.forward(r, k, v, w, u, want_state=True)
    assert torch.equal(s2, s_full)
    yr = WO.forward(r, k, v, w, u, reverse=True)
    yf = WO.forward(*(t.flip(1).contiguous() for t in (r, k, v, w)), u).flip(1)
    assert torch.equal(yr, yf)


# ---------------------------------------------------------------- Python restatement vs reference goldens
@pytest.mark.parametrize("tag", ["reduced_f32", "reduced_bf16", "full_f32", "full_bf16"])
def test_uni_wrapper_golden(tag):
    g = load_golden("uni_wrapper_" + tag)
    sd = _sd(g)
    y, cache = EO.rwkv_wrapper(g["x"], sd, "", g["head_size"], g["do_bfloat16"])
    assert _close(y, g["y"], g["do_bfloat16"]) and tuple(cache.shape) == g["cache_shape"]
    xin = g["x"].bfloat16() if g["do_bfloat16"] else g["x"]
    assert _close(EO.tmix_x060c(xin, sd, "tmix_block.", g["head_size"]), g["block_y"], g["do_bfloat16"])


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_bi_wrapper_golden(tag):
    g = load_golden("bi_wrapper_" + tag)
    y, cache = EO.rwkv_wrapper_bidirectional(g["x"], _sd(g), "", g["head_size"], g["do_bfloat16"])
    assert y.dtype == torch.float32 and _close(y, g["y"], g["do_bfloat16"]) and tuple(cache.shape) == g["cache_shape"]


def test_dir_dropout_eval_golden():
    g = load_golden("dir_dropout_eval")
    sd = _sd(g)
    assert len(g["cases"]) == 24
    for c in g["cases"]:
        y, _ = EO.self_attn(g["x"], sd, "", c["kind"], g["head_size"], True, c["layer_id"], env=c["env"])
        assert _close(y, c["y"], True), (c["kind"], c["env"], c["layer_id"])


@pytest.mark.parametrize("variant", ["bf16slot", "f32", "uni_bf16slot", "uni_bf16model"])
def test_encoder_reduced_golden(variant, monkeypatch):
    g = load_golden("encoder_reduced_" + variant)
    sd = _sd(g)
    csd = synth.synth_state_dict(g["ctc_spec"], g["ctc_seed"])
    if variant == "uni_bf16model":
        _bf16_model_gemms(monkeypatch)
        sd = {k: v.bfloat16() for k, v in sd.items()}
        csd = {k: v.bfloat16() for k, v in csd.items()}
    out, masks, layers = EO.encoder_forward(g["xs"], g["lens"], sd, g["conf"], env={}, return_layers=True)
    assert torch.equal(masks, g["masks"])
    bf = variant != "f32"
    assert _close(layers[0], g["layer0"], bf) and _close(layers[1], g["layer1"], bf)
    assert _close(out, g["out"], bf)
    yc, att, cnn = EO.encoder_forward_chunk(g["chunk_x"], sd, g["conf"], env={})
    assert _close(yc, g["chunk_y"], bf)
    assert tuple(att.shape) == g["att_cache_shape"] and tuple(cnn.shape) == g["cnn_cache_shape"]
    logp = EO.ctc_log_softmax(out, {"ctc." + k: v for k, v in csd.items()})
    assert _close(logp[:, ::7, :], g["logp_sample"], bf)
    enc_lens = masks.squeeze(1).sum(1)
    assert torch.equal(enc_lens, g["enc_lens"])
    # token ids are the bit-exact bar: decode the golden's own encoder output so that a bf16 rounding flip
    # upstream cannot masquerade as a search bug, then also require our end-to-end tokens to agree
    assert EO.ctc_greedy_search(g["logp_full"].float(), enc_lens, 0) == g["greedy"]
    if torch.equal(out, g["out"]):  # same machine / thread count as the capture: end to end is exact too
        assert EO.ctc_greedy_search(logp.float(), enc_lens, 0) == g["greedy"]


@pytest.mark.parametrize("variant", ["bf16slot", "f32", "uni_bf16slot"])
def test_forward_chunk_by_chunk_golden(variant):
    """BaseEncoder.forward_chunk_by_chunk (encoder.py:341-402) captured from the reference (make_goldens_r2.py)."""
    g = load_golden("encoder_chunk_by_chunk")
    c = g["cases"][variant]
    sd = _sd(c)
    for chunk, want in c["outs"].items():
        ys, masks = EO.encoder_forward_chunk_by_chunk(g["xs"], chunk, sd, c["conf"], env={})
        assert torch.equal(masks, want["masks"]) and ys.shape == want["ys"].shape == (1, 50, 128)
        assert _close(ys, want["ys"], variant != "f32"), (variant, chunk)
    # windows are independent full-context passes: a chunked pass differs from the whole-utterance pass
    full, _ = EO.encoder_forward(g["xs"], torch.tensor([g["xs"].size(1)]), sd, c["conf"], env={})
    assert full.shape == (1, 50, 128)
    assert not torch.allclose(full.float(), c["outs"][16]["ys"].float(), atol=1e-2)


def test_dir_dropout_train_golden():
    """Train-time branch of the direction-dropout wrappers (…direction_dropout.py:59-69, …_both.py:55-71): same host
    RNG draws as the reference under torch.manual_seed, same branch arithmetic; every branch occurs in the fixture."""
    g = load_golden("dir_dropout_train")
    sd = _sd(g)
    seen = set()
    for c in g["cases"]:
        torch.manual_seed(c["manual_seed"])
        keep, left_only = EO.draw_direction_dropout(c["both"])
        branch = "bi" if keep else ("left" if (not c["both"] or left_only) else "right")
        assert branch == c["branch"], c["manual_seed"]
        y, _ = EO.rwkv_wrapper_dir_dropout_train(g["x"], sd, "", g["head_size"], True, c["both"], keep, left_only)
        assert _close(y, c["y"], True), (c["kind"], c["manual_seed"])
        seen.add((c["both"], branch))
    assert seen == {(False, "bi"), (False, "left"), (True, "bi"), (True, "left"), (True, "right")}


def test_whole_model_bf16_bidirectional_mode_is_defined_by_one_flag():
    """The headline precision (whole-model bf16, bidirectional slot) cannot run in the reference: its wrapper returns
    .float() (rwkv_wrapper_bidirectional.py:55-56) into a bf16 LayerNorm.  The oracle's `oracle_slot_out_as_query` is the
    one change that defines it; for an fp32 query it changes nothing."""
    g = load_golden("encoder_reduced_bf16slot")
    sd = _sd(g)
    a, _ = EO.encoder_forward(g["xs"], g["lens"], sd, g["conf"], env={})
    b, _ = EO.encoder_forward(g["xs"], g["lens"], sd, dict(g["conf"], oracle_slot_out_as_query=True), env={})
    assert torch.equal(a, b)
    sdb = {k: v.bfloat16() for k, v in sd.items()}
    with pytest.raises(RuntimeError):
        EO.encoder_forward(g["xs"].bfloat16(), g["lens"], sdb, g["conf"], env={})
    out, _ = EO.encoder_forward(g["xs"].bfloat16(), g["lens"], sdb, dict(g["conf"], oracle_slot_out_as_query=True), env={})
    assert out.dtype == torch.bfloat16 and bool(torch.isfinite(out.float()).all())
    d = (out.float() - g["out"]).abs()
    assert float(d.max()) <= 0.4 and float(d.mean()) <= 2e-2      # the bf16 model is the fp32 + bf16-slot model, rounded


def test_padding_dependence_is_reproduced():
    """The reference flips the whole padded tensor (rwkv_wrapper_bidirectional.py:44), so a short utterance's
    right-to-left state is warmed by its padding: valid-frame outputs depend on the batch it sits in."""
    g = load_golden("encoder_reduced_bf16slot")
    sd = _sd(g)
    out_b, _ = EO.encoder_forward(g["xs"], g["lens"], sd, g["conf"], env={})
    n = int(g["lens"][2])
    out_1, _ = EO.encoder_forward(g["xs"][2:3, :n].contiguous(), g["lens"][2:3], sd, g["conf"], env={})
    t1 = out_1.shape[1]
    assert not torch.allclose(out_b[2:3, :t1], out_1, atol=1e-3)


def test_fbank_oracle_agrees_with_an_independent_kaldi_compatible_extractor():
    """torchaudio (the reference's fbank, dataset/processor.py:363-369) is absent from the image, so the fbank oracle is
    restated from the Kaldi definition.  Cross-check against an INDEPENDENT implementation of the same definition that
    is installed here: transformers' SeamlessM4TFeatureExtractor (its `_extract_fbank_features` is documented and
    tested upstream as torchaudio.compliance.kaldi.fbank-compatible: povey window, pre-emphasis 0.97, DC removal, 512-
    point power spectrum, 80 Kaldi mel bins from 20 Hz, log with the float-epsilon floor, 2^15 input scaling)."""
    np = pytest.importorskip("numpy")
    tr = pytest.importorskip("transformers")
    from oracle import fbank_oracle as FO
    fe = tr.SeamlessM4TFeatureExtractor(feature_size=80, sampling_rate=16000, num_mel_bins=80)
    rng = np.random.default_rng(0)
    for seconds, amp in ((3.0, 0.1), (0.5, 0.5), (1.234, 0.01)):
        w = (rng.standard_normal(int(16000 * seconds)) * amp).astype(np.float32)
        want = torch.from_numpy(fe._extract_fbank_features(w))
        got = FO.fbank(torch.from_numpy(w * 2 ** 15).unsqueeze(0), num_mel_bins=80, frame_length=25.0, frame_shift=10.0,
                       dither=0.0, energy_floor=0.0, sample_frequency=16000.0)
        assert got.shape == want.shape == (1 + (len(w) - 400) // 160, 80)
        assert float((got - want).abs().max()) < 2e-3, float((got - want).abs().max())   # log-mel values are 5..26
        assert float((got - want).abs().mean()) < 5e-5


def test_mamba2_oracle_agrees_with_an_independent_port_of_the_published_block():
    """`mamba_ssm` (the reference's Mamba-2, mamba_att_wrapper.py:24-35, mamba2_bidirectional.py:40-62) is absent from
    the image, so the Mamba-2 oracle restates the published block.  Cross-check against an INDEPENDENT implementation
    that is installed here: transformers' Mamba2Mixer (the upstream port of mamba_ssm's Mamba2 with the same parameter
    names and layout -- in_proj / conv1d / dt_bias / A_log / D / norm / out_proj -- whose CPU path is a chunked SSD,
    not a sequential recurrence), on the paper's configuration (headdim 64, d_state 128, d_conv 4, expand 2, 1 group,
    gate before the RMSNorm, eps 1e-5) with the same weights, at lengths below, at and across its chunk size."""
    tr = pytest.importorskip("transformers")
    try:
        from transformers.models.mamba2.modeling_mamba2 import Mamba2Mixer
    except ImportError:
        pytest.skip("this transformers has no Mamba2Mixer")
    from oracle import mamba2_oracle as MO
    torch.manual_seed(0)
    d_model, H = 128, 4
    cfg = tr.Mamba2Config(hidden_size=d_model, state_size=128, conv_kernel=4, expand=2, head_dim=64, num_heads=H,
                          n_groups=1, use_bias=False, use_conv_bias=True, rms_norm=True, chunk_size=64,
                          num_hidden_layers=1, layer_norm_epsilon=1e-5, time_step_limit=(0.0, float("inf")))
    mixer = Mamba2Mixer(cfg, 0).eval()
    with torch.no_grad():
        for n, p in mixer.named_parameters():
            if n in ("in_proj.weight", "out_proj.weight"):
                p.copy_(torch.randn_like(p) * 0.08)
            elif n.startswith("conv1d."):
                p.copy_(torch.randn_like(p) * 0.3)
            elif n == "norm.weight":
                p.copy_(1 + 0.2 * torch.randn_like(p))
        mixer.D.copy_(torch.randn(H))
        mixer.A_log.copy_(torch.log(torch.empty(H).uniform_(1, 16)))
    sd = {"m." + k: v.detach() for k, v in mixer.state_dict().items()}
    assert {k[2:] for k in sd} == {"in_proj.weight", "conv1d.weight", "conv1d.bias", "dt_bias", "A_log", "D",
                                   "norm.weight", "out_proj.weight"}
    for L in (1, 7, 64, 150):
        u = torch.randn(2, L, d_model)
        with torch.no_grad():
            want = mixer(u)
        got = MO.mamba2_forward(u, sd, "m.")
        assert got.shape == want.shape
        assert float((got - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max())), (L, float((got - want).abs().max()))


def test_state_recurrence_f64_agrees_with_the_pinned_c_restatement():
    """The differentiable float64 recurrence used to check the state-carrying backward (oracle/wkv6_oracle.py) computes
    what the golden-pinned C restatement of wkv6state_cuda.cu:6-65 computes: outputs and final state, with a state."""
    from oracle import wkv6_oracle as WO
    from tests import synth
    B, T, C, H = 2, 23, 128, 2
    r, k, v = (synth.randn((B, T, C), 70 + i, 0.5) for i in range(3))
    w = synth.randn((B, T, C), 73, 0.5) - 1.0
    u = synth.randn((H, 64), 74, 0.3)
    s = synth.randn((B, H, 64, 64), 75, 0.5)
    y_c, s_c = WO.forward(r, k, v, w, u, s_in=s, want_state=True)
    y_p, s_p = WO.state_recurrence_f64(r, k, v, w, u, s)
    torch.testing.assert_close(y_p.float(), y_c, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(s_p.float(), s_c, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("case", ["postnorm_f32", "postnorm_bf16slot", "abspos_f32", "abspos_bf16slot"])
def test_postnorm_and_abspos_goldens(case):
    """Post-norm layers (encoder_layer.py:207-256) and abs_pos windows with their running offset (embedding.py:58-77,
    encoder.py:377-399), captured from the reference (make_goldens_r3.py)."""
    g = load_golden("encoder_postnorm_abspos")
    c = g["cases"][case]
    sd = _sd(c)
    bf = case.endswith("bf16slot")
    out, masks = EO.encoder_forward(g["xs"], g["lens"], sd, c["conf"], env={})
    assert torch.equal(masks, c["masks"]) and _close(out, c["out"], bf), case
    for chunk, want in c.get("chunks", {}).items():
        ys, m = EO.encoder_forward_chunk_by_chunk(g["long"], chunk, sd, c["conf"], env={})
        assert torch.equal(m, want["masks"]) and _close(ys, want["ys"], bf), (case, chunk)
        # the offset matters: the same windows embedded at offset 0 give something else
        ys0 = torch.cat([EO.encoder_forward_chunk(g["long"][:, cur:min(cur + (chunk - 1) * 4 + 7, g["long"].size(1))], sd,
                                                  c["conf"], env={})[0]
                         for cur in range(0, g["long"].size(1) - 6, 4 * chunk)], 1)
        assert not torch.allclose(ys0.float(), want["ys"].float(), atol=1e-2)


# ---------------------------------------------------------------- round 4: the causal conv module + cnn_cache (streaming leg)
@pytest.mark.parametrize("case", ["k15_f32", "k15_bf16", "k31_f32", "k31_bf16"])
def test_conv_module_causal_golden(case):
    """ConvolutionModule(causal=True) (convolution.py:49-60,113-126) captured from the reference (make_goldens_r4.py):
    a ragged masked batch without cache, and one stream cut in three with the cache handed on -- outputs and caches."""
    c = load_golden("conv_module_causal")["cases"][case]
    sd = _sd(c)
    bf = case.endswith("bf16")
    if bf:
        sd = {k: v.bfloat16() for k, v in sd.items()}
    k = c["kernel"]
    mask = (torch.arange(c["xb"].size(1))[None, :] < c["lens"][:, None]).unsqueeze(1)
    yb, cb = EO.conv_module(c["xb"], mask, sd, "", k, causal=True)
    assert yb.dtype == c["yb"].dtype and _close(yb, c["yb"], bf) and cb.shape == c["cb"].shape == (3, 128, k - 1)
    assert torch.equal(cb, c["cb"])                  # the cache is the (masked) input itself: exact
    empty = torch.ones((0, 0, 0), dtype=torch.bool)
    cache = None
    for (a, b), want in zip(zip(c["cuts"][:-1], c["cuts"][1:]), c["pieces"]):
        y, cache = EO.conv_module(c["xs"][:, a:b], empty, sd, "", k, causal=True, cache=cache)
        assert _close(y, want["y"], bf) and torch.equal(cache, want["new_cache"]), (case, a, b)
    whole, cw = EO.conv_module(c["xs"], empty, sd, "", k, causal=True)
    assert _close(whole, c["whole"], bf) and torch.equal(cw, c["whole_cache"])
    # causality: frame t of the output does not see inputs after t
    x2 = c["xs"].clone()
    x2[:, 50:] = 0
    y2, _ = EO.conv_module(x2, empty, sd, "", k, causal=True)
    assert torch.equal(y2[:, :50], whole[:, :50])


@pytest.mark.parametrize("prec", ["f32", "bf16slot", "bf16model"])
def test_encoder_causal_uni_golden(prec, monkeypatch):
    """Reduced ConformerEncoder, rwkv_tmix60 + causal: true, captured from the reference (make_goldens_r4.py): forward of
    a ragged batch, of one long utterance, forward_chunk with the cnn_cache handed on (encoder.py:311-337), and
    forward_chunk_by_chunk -- which in the reference carries the conv cache but restarts the recurrence per window."""
    g = load_golden("encoder_causal_uni")
    c = g["cases"][prec]
    sd = _sd(c)
    csd = synth.synth_state_dict(c["ctc_spec"], c["ctc_seed"])
    xs, long = g["xs"], g["long"]
    if prec == "bf16model":
        _bf16_model_gemms(monkeypatch)
        sd = {k: v.bfloat16() for k, v in sd.items()}
        csd = {k: v.bfloat16() for k, v in csd.items()}
        xs, long = xs.bfloat16(), long.bfloat16()
    bf = prec != "f32"
    assert c["conf"]["causal"] is True and c["conf"]["selfattention_layer_type"] == "rwkv_tmix60"
    out, masks, layers = EO.encoder_forward(xs, g["lens"], sd, c["conf"], env={}, return_layers=True)
    assert torch.equal(masks, c["masks"]) and out.dtype == c["out"].dtype
    assert _close(layers[0], c["layer0"], bf) and _close(layers[1], c["layer1"], bf) and _close(out, c["out"], bf)
    enc_lens = masks.squeeze(1).sum(1)
    assert EO.ctc_greedy_search(c["logp_full"].float(), enc_lens, 0) == c["greedy"]
    logp = EO.ctc_log_softmax(out, {"ctc." + k: v for k, v in csd.items()})
    if torch.equal(out, c["out"]):
        assert EO.ctc_greedy_search(logp.float(), enc_lens, 0) == c["greedy"]
    whole, _ = EO.encoder_forward(long, torch.tensor([long.size(1)]), sd, c["conf"], env={})
    assert _close(whole, c["whole"], bf)
    y0, a0, c0 = EO.encoder_forward_chunk(long[:, 0:35], sd, c["conf"], env={}, offset=0)
    y1, a1, c1 = EO.encoder_forward_chunk(long[:, 32:67], sd, c["conf"], env={}, offset=8, cnn_cache=c0)
    for (y, a, cc), want in (((y0, a0, c0), c["chunk0"]), ((y1, a1, c1), c["chunk1"])):
        assert tuple(a.shape) == want["att_shape"] == (0, 0, 0, 0)
        assert cc.shape == want["cnn"].shape == (2, 1, 128, 14)
        assert _close(y, want["y"], bf) and _close(cc, want["cnn"], bf)
    for chunk, want in c["chunks"].items():
        ys, m = EO.encoder_forward_chunk_by_chunk(long, chunk, sd, c["conf"], env={})
        assert torch.equal(m, want["masks"]) and _close(ys, want["ys"], bf), (prec, chunk)
    # the first window has no history in either form: it equals the head of the whole-sequence pass (causal conv, uni slot)
    assert _close(y0, c["whole"][:, :8], bf)
    # ... the later ones do not: the reference restarts the recurrence per window (rwkv_wrapper.py:81)
    assert not torch.allclose(c["chunks"][8]["ys"].float(), c["whole"].float(), atol=1e-2)
