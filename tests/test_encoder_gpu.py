"""The MI355X encoder path (HIP kernels through the C ABI) vs goldens captured from the reference and vs the
CPU oracle on the same seeded inputs.  GPU only."""
import pytest
import torch

from oracle import encoder_oracle as EO
from tests import parity_log, synth
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def _stats(a, b):
    d = (a.float() - b.float()).abs()
    return float(d.max()), float(d.mean())


def _assert_close(got, ref, bf16_path, what="", whole_model_bf16=False):
    """fp32 path: north_star's 1e-3 relative (with an absolute floor for values near zero).
    bf16-inside paths: max |err| <= 0.1 and mean |err| <= 6e-3 on O(1) activations -- the spread the reference
    shows against ITSELF when only its GEMM summation order changes (tests/test_oracle_goldens.py:_close)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    mx, mean = _stats(got, ref)
    if what:
        parity_log.record(f"golden/{what}", max_abs_err=mx, mean_abs_err=mean, ref_abs_max=float(ref.abs().max()),
                          mode="whole-bf16" if whole_model_bf16 else "bf16-inside" if bf16_path else "fp32")
    if whole_model_bf16:
        # every op of every layer rounds to bf16 (ulp 0.03 at |x| = 4) and CPU / GPU differ in each op's internal
        # order, not only in the GEMMs.  Bounds = 2 x the largest values recorded in profiles/parity_r03.json
        # (round 3: max 0.078, mean 0.0077 over the whole-bf16 goldens)
        assert mx <= 0.16 and mean <= 1.6e-2, f"{what}: max {mx:.4g} mean {mean:.4g}"
    elif bf16_path:
        assert mx <= 0.1 and mean <= 6e-3, f"{what}: max {mx:.4g} mean {mean:.4g}"
    else:
        tol = 1e-3 * ref.abs().clamp_min(5e-2)
        assert bool(((got - ref).abs() <= tol).all()), f"{what}: max {mx:.4g} mean {mean:.4g}"


def _sd(g):
    sd = synth.synth_state_dict(g["spec"], g["seed"])
    assert abs(synth.checksum(sd) - g["checksum"]) <= 1e-6 * g["checksum"]
    return sd


@pytest.mark.parametrize("tag", ["reduced_f32", "reduced_bf16", "full_f32", "full_bf16"])
def test_uni_wrapper(hip, tag):
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    g = load_golden("uni_wrapper_" + tag)
    C = g["x"].shape[-1]
    m = WENET_ATTENTION_CLASSES["rwkv_tmix60"](g["head_size"], C, 12 if "full" in tag else 2, "rwkv", "uni", 2048,
                                               g["do_bfloat16"], 1)
    m.load_state_dict(_sd(g))
    m = m.cuda().eval()
    x = g["x"].cuda()
    with torch.no_grad():
        y, cache = m(x, x, x, torch.ones((0, 0, 0), dtype=torch.bool), torch.empty(0), torch.zeros((0, 0, 0, 0)))
    assert y.dtype == g["y"].dtype and tuple(cache.shape) == g["cache_shape"]
    _assert_close(y, g["y"], g["do_bfloat16"], f"uni_wrapper/{tag}")


@pytest.mark.parametrize("key", ["rwkv_tmix60_bidirectional", "rwkv_tmix60_bidirectional2"])
@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_bi_wrapper(hip, key, tag):
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    g = load_golden("bi_wrapper_" + tag)
    m = WENET_ATTENTION_CLASSES[key](64, 128, 2, "rwkv", "bi", 2048, g["do_bfloat16"], 1)
    m.load_state_dict(_sd(g))
    m = m.cuda().eval()
    x = g["x"].cuda()
    with torch.no_grad():
        y, cache = m(x, x, x)
        y_none, _ = m(x, None, None, None, None, None)  # bidirectional2 calls its inner wrappers with None
    assert y.dtype == torch.float32 and tuple(cache.shape) == g["cache_shape"]
    assert torch.equal(y, y_none)
    _assert_close(y, g["y"], g["do_bfloat16"], f"{key}/{tag}")


def test_dir_dropout_eval(hip, monkeypatch):
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    g = load_golden("dir_dropout_eval")
    sd = _sd(g)
    x = g["x"].cuda()
    for c in g["cases"]:
        for k in ("RWKV_BIDIRECTIONAL_LAYERS", "RWKV_ALT_DECODING"):
            monkeypatch.delenv(k, raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
        m = WENET_ATTENTION_CLASSES[c["kind"]](64, 128, 4, "rwkv", "bi", 2048, True, c["layer_id"])
        m.load_state_dict(sd)
        m = m.cuda().eval()
        with torch.no_grad():
            y, _ = m(x, x, x)
        _assert_close(y, c["y"], True, f"{c['kind']} {c['env']} layer {c['layer_id']}")


@pytest.mark.parametrize("kind", ["rwkv_tmix60_dir_layer_drop", "rwkv_tmix60_dir_layer_drop_both"])
@pytest.mark.parametrize("env,want", [
    ({}, [(2, False)] * 4),                                                         # no variable set: every layer bidirectional
    ({"RWKV_BIDIRECTIONAL_LAYERS": "-1"}, [(1, False)] * 4),                         # "alt-only" as the sweep script RAN it: l2r only
    ({"RWKV_BIDIRECTIONAL_LAYERS": "-1", "RWKV_ALT_DECODING": "1"}, [(1, False), (1, True), (1, False), (1, True)]),
    ({"RWKV_BIDIRECTIONAL_LAYERS": "3", "RWKV_ALT_DECODING": "1"}, [(1, False), (1, True), (1, False), (2, False)]),
    ({"RWKV_BIDIRECTIONAL_LAYERS": "0,1"}, [(2, False), (2, False), (1, False), (1, False)])])
def test_dir_dropout_eval_variants_on_the_fused_executor(hip, monkeypatch, kind, env, want):
    """The eval-time variants of the direction-dropout models the paper's RTF sweep runs (go-run-encoder-rtf.single-gpu-3x3-g5.sh:
    83-103: RWKV_BIDIRECTIONAL_LAYERS = -1 / 11 / 9,10,11 / 0 / 6..11, RWKV_ALT_DECODING) through the fused executor: each layer
    runs both directions, left-to-right only or right-to-left only as the wrapper's eval branches say
    (rwkv_wrapper_bidirectional_direction_dropout_both.py:72-92), and the result equals the module path, whose wrappers are
    pinned by the reference's golden (test_dir_dropout_eval).  fp32 model + bf16 slot and whole-model bf16, ragged batch."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_f32")
    for k in ("RWKV_BIDIRECTIONAL_LAYERS", "RWKV_ALT_DECODING"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    conf = dict(g["conf"], selfattention_layer_type=kind, rnn_att_direction="bi", num_blocks=4, rwkv_do_bfloat16=True)
    torch.manual_seed(21)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.05)
    xs = synth.randn((3, 211, 80), 77, 2.0)
    lens = torch.tensor([211, 150, 64])
    for whole_bf16 in (False, True):
        m = (enc.to(torch.bfloat16) if whole_bf16 else enc).cuda()
        x = xs.cuda().to(torch.bfloat16 if whole_bf16 else torch.float32)
        with torch.no_grad():
            m.fused_inference = True
            got, masks = m(x, lens.cuda())
            plan = m._fused_plan
            assert plan and [(lp.ndir, lp.reverse0) for lp in plan.layers] == want
            m.fused_inference = False
            ref, masks2 = m(x, lens.cuda())
            m.fused_inference = True
        assert torch.equal(masks, masks2)
        valid = masks.squeeze(1)
        if whole_bf16:
            # two schedules of a whole-bf16 model differ by bf16 rounding at every op (ulp 0.03 at |x| = 4), single elements by
            # more where a LayerNorm row has little variance: the bounds of test_full_size_encoder_properties (a wrong direction or
            # a wrong block would move the MEAN to O(0.5))
            d = (got[valid].float() - ref[valid].float()).abs()
            parity_log.record(f"fused dir-drop {kind} {env} bf16", max_abs_err=float(d.max()), mean_abs_err=float(d.mean()))
            assert float(d.mean()) < 2e-2 and float(d.max()) < 0.6, (float(d.mean()), float(d.max()))
        else:
            # both sides round to bf16 inside the slot, at different points (the executor keeps fp32 accumulators across fused
            # steps): recorded max 0.075-0.19, mean 0.005-0.007 on this 4-layer model with LoRA weights of 0.05 -- a wrong direction
            # or block moves the mean to O(0.3)
            d = (got[valid].float() - ref[valid].float()).abs()
            parity_log.record(f"fused dir-drop {kind} {env} bf16slot", max_abs_err=float(d.max()), mean_abs_err=float(d.mean()))
            assert float(d.mean()) <= 1.2e-2 and float(d.max()) <= 0.3, (float(d.mean()), float(d.max()))


@pytest.mark.parametrize("variant", ["bf16slot", "f32", "uni_bf16slot", "uni_bf16model"])
def test_encoder_reduced(hip, variant):
    from paper_accurate_fast_cheap_amd.transformer.cmvn import GlobalCMVN
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_greedy_search
    g = load_golden("encoder_reduced_" + variant)
    sd = _sd(g)
    enc = ConformerEncoder(80, global_cmvn=GlobalCMVN(torch.zeros(80), torch.ones(80)), **g["conf"])
    enc.load_state_dict(sd)  # strict: every reference key present, nothing extra
    ctc = CTC(50, 128)
    csd = synth.synth_state_dict(g["ctc_spec"], g["ctc_seed"])
    ctc.load_state_dict(csd)
    if variant == "uni_bf16model":
        enc, ctc = enc.to(torch.bfloat16), ctc.to(torch.bfloat16)
    enc, ctc = enc.cuda().eval(), ctc.cuda().eval()
    bf = variant != "f32"
    wm = variant == "uni_bf16model"

    def _assert_close(a, b, bfp, what):  # noqa: F811 -- same check, whole-model flag bound per variant
        globals()["_assert_close"](a, b, bfp, f"encoder_reduced_{variant}/{what}", whole_model_bf16=wm)
    with torch.no_grad():
        out, masks, layers = enc.forward_return_layers(g["xs"].cuda(), g["lens"].cuda(), want_layers=True)
        assert torch.equal(masks.cpu(), g["masks"])
        _assert_close(layers[0], g["layer0"], bf, "layer0")
        _assert_close(layers[1], g["layer1"], bf, "layer1")
        _assert_close(out, g["out"], bf, "out")
        assert out.dtype == g["out"].dtype
        yc, att, cnn = enc.forward_chunk(g["chunk_x"].cuda(), 0, -1)
        _assert_close(yc, g["chunk_y"], bf, "chunk")
        assert tuple(att.shape) == g["att_cache_shape"] and tuple(cnn.shape) == g["cnn_cache_shape"]
        logp = ctc.log_softmax(out)
        _assert_close(logp[:, ::7, :], g["logp_sample"], bf, "logp")
        enc_lens = masks.squeeze(1).sum(1)
        assert torch.equal(enc_lens.cpu(), g["enc_lens"])
        # bit-exact bar: token ids.  (1) our search on the golden's encoder output, (2) end to end
        # (1): the reference's own log-probs in -> the reference's tokens out, bit for bit
        glogp = g["logp_full"].cuda()
        top = glogp.float().max(-1).values
        ties = bool(((glogp.float() == top[..., None]).sum(-1) > 1).any())   # bf16 log-probs can tie exactly
        if not ties:
            assert [r.tokens for r in ctc_greedy_search(glogp.float(), enc_lens, 0)] == g["greedy"]
        else:  # which of several exact maximisers topk(1) returns is implementation-defined: ours must be one
            pick = glogp.float().argmax(-1)
            assert torch.equal(glogp.float().gather(-1, pick[..., None])[..., 0], top)
        ours = [r.tokens for r in ctc_greedy_search(logp.float(), enc_lens, 0)]
        if not bf:
            assert ours == g["greedy"]
        else:
            flips = _token_parity(logp, glogp, masks.squeeze(1), 0.07, f"encoder_reduced_{variant}")   # recorded: 0.028-0.034
            if flips == 0:
                assert ours == g["greedy"]


def _token_parity(logp, ref_logp, valid, logp_tol, what):
    """Token ids are the bit-exact bar.  A path that rounds to bf16 inside cannot promise the reference's argmax on a
    frame whose two best tokens the REFERENCE itself separates by less than the bf16 noise: with e = the measured
    max |log-prob difference| of this comparison (itself held to `logp_tol`, the spread the reference shows against
    itself across summation orders), an argmax can only move where the reference's top-2 margin is <= 2e.  So: every
    frame whose reference margin exceeds 2e must carry the reference's token, and the flipped frames are counted and
    reported.  Returns the number of flipped valid frames."""
    logp, ref_logp = logp.float().cpu(), ref_logp.float().cpu()
    valid = valid.cpu()
    e = float(((logp - ref_logp).abs() * valid[..., None]).max())
    assert e <= logp_tol, f"{what}: max |dlogp| {e:.4g} > {logp_tol}"
    top2 = ref_logp.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    same = logp.argmax(-1) == ref_logp.argmax(-1)
    decided = (margin > 2 * e) & valid
    assert bool((same | ~decided).all()), f"{what}: token differs on a frame the reference decides by more than 2e = {2 * e:.4g}"
    flips = int((~same & valid).sum())
    parity_log.record(f"tokens/{what}", max_abs_dlogp=e, flipped_frames=flips, valid_frames=int(valid.sum()),
                      largest_margin_among_flipped=float(margin[~same & valid].max()) if flips else 0.0,
                      undecided_frames_margin_le_2e=int(((margin <= 2 * e) & valid).sum()))
    print(f"[token parity] {what}: {flips} of {int(valid.sum())} valid frames flipped, all with reference top-2 margin "
          f"<= {2 * e:.4g} (max |dlogp| {e:.4g}); largest margin among flipped frames "
          f"{float(margin[~same & valid].max()) if flips else 0.0:.4g}")
    return flips


def test_encoder_matches_oracle_on_fresh_inputs(hip):
    """Same seeded inputs through the CPU restatement and the HIP path (not a golden: different lengths, batch 4,
    T not a multiple of anything)."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_f32")
    sd = _sd(g)
    sd = {k: v for k, v in sd.items() if not k.startswith("global_cmvn")}
    enc = ConformerEncoder(80, **g["conf"])
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    xs = synth.randn((4, 331, 80), 901, 2.0)
    lens = torch.tensor([331, 330, 97, 12])
    ref, ref_masks = EO.encoder_forward(xs, lens, sd, g["conf"], env={})
    with torch.no_grad():
        out, masks = enc(xs.cuda(), lens.cuda())
    assert torch.equal(masks.cpu(), ref_masks)
    _assert_close(out, ref, False, "fresh")


def test_config_c1_full_size_fp32_vs_oracle(hip, monkeypatch):
    """BASELINE configs[0] on the GPU: 10 utterances with the config's own length filter (100..2000 frames, conf yaml
    :113; the longest is exactly 2000), the FULL 12-layer 512-d bidirectional encoder in fp32 + CTC head: HIP path vs
    the CPU restatement ELEMENT-wise: |err| <= 1e-3 * |ref| + 2.5e-4 (outputs are LayerNorm rows of unit RMS: the
    absolute term, a quarter of 1e-3 of that RMS, covers the elements near zero, where a relative error means nothing), masks
    exact, CTC greedy token ids identical on every frame the oracle decides by more than the numerical noise."""
    import bench
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_greedy_search
    conf = dict(bench.encoder_conf(), rwkv_do_bfloat16=False)
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    ctc = CTC(200, 512).eval()
    g = torch.Generator().manual_seed(31)
    lens = torch.randint(100, 2001, (10,), generator=g)
    lens[0] = 2000
    xs = synth.randn((10, 2000, 80), 902, 2.0)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    ref, ref_masks = EO.encoder_forward(xs, lens, sd, conf, env={})
    ref_logp = EO.ctc_log_softmax(ref, {"ctc." + k: v for k, v in ctc.state_dict().items()})
    ref_lens = ref_masks.squeeze(1).sum(1)
    enc, ctc = enc.cuda(), ctc.cuda()
    # a pure-fp32 model takes exact fp32 products everywhere -- also outside the layers, at 4 990 rows (>= split_gemm_min_rows):
    # the encoder tells its front end, init_model tells the CTC head (set by hand here: the head is built stand-alone)
    from paper_accurate_fast_cheap_amd import hip_ops
    assert enc.fp32_split_operands is False and enc.embed.fp32_split_operands is False
    ctc.fp32_split_operands = enc.fp32_split_operands
    split_calls = []
    real_ex = hip_ops.gemm_ph_ex
    monkeypatch.setattr(hip_ops, "gemm_ph_ex", lambda *a, **k: (split_calls.append(k.get("a_split", False)), real_ex(*a, **k))[1])
    with torch.no_grad():
        out, masks = enc(xs.cuda(), lens.cuda())
        logp = ctc.log_softmax(out)
        toks = [r.tokens for r in ctc_greedy_search(logp, masks.squeeze(1).sum(1), 0)]
    assert not any(split_calls), "a pure-fp32 model launched a split-operand GEMM"
    assert out.shape == (10, 499, 512) and torch.equal(masks.cpu(), ref_masks)
    valid = ref_masks.squeeze(1)
    got = out.cpu()[valid]
    want = ref[valid]
    torch.testing.assert_close(got, want, rtol=1e-3, atol=2.5e-4)
    d = (got - want).abs()
    parity_log.record("c1 fp32 full size", max_abs_err=float(d.max()), mean_abs_err=float(d.mean()),
                      max_rel_err_where_ref_ge_0p05=float((d / want.abs().clamp_min(5e-2)).max()))
    flips = _token_parity(logp, ref_logp, valid, 1e-3 * float(ref_logp.abs().max()), "c1 fp32")
    assert flips == 0                                   # fp32: token ids are bit-exact, no margin rule
    assert toks == EO.ctc_greedy_search(ref_logp, ref_lens, 0)


def _bf16_headline(xs, lens, enc, ctc, conf, what):
    """HIP fused path in the bench's precision (whole-model bf16, bidirectional slot) vs (1) the oracle in MATCHED precision
    (every op rounds to bf16, the slot returns the query dtype: oracle_slot_out_as_query) and (2) the exact model: the
    same bf16-valued parameters and inputs in fp32 arithmetic with an fp32 slot.  The HIP path keeps fp32 accumulators
    across fused steps, so it must sit at least as close to the exact model as the reference's own rounding does."""
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_greedy_search
    sd_b = {k: v.detach().cpu().to(torch.bfloat16) for k, v in enc.state_dict().items()}
    csd_b = {"ctc." + k: v.detach().cpu().to(torch.bfloat16) for k, v in ctc.state_dict().items()}
    xb = xs.to(torch.bfloat16)
    ref, ref_masks = EO.encoder_forward(xb, lens, sd_b, dict(conf, oracle_slot_out_as_query=True), env={})
    assert ref.dtype == torch.bfloat16
    ref_logp = EO.ctc_log_softmax(ref, csd_b)
    sd_f = {k: v.float() for k, v in sd_b.items()}
    exact, _ = EO.encoder_forward(xb.float(), lens, sd_f, dict(conf, rwkv_do_bfloat16=False), env={})
    exact_logp = EO.ctc_log_softmax(exact, {k: v.float() for k, v in csd_b.items()})
    encb, ctcb = enc.to(torch.bfloat16).cuda().eval(), ctc.to(torch.bfloat16).cuda().eval()
    with torch.no_grad():
        encb.fused_inference = True
        out, masks = encb(xb.cuda(), lens.cuda())
        assert encb._fused(out) is not None                       # the fused executor (what bench.py times) really ran
        logp = ctcb.log_softmax(out)
        toks = [r.tokens for r in ctc_greedy_search(logp, masks.squeeze(1).sum(1), 0)]
    assert out.dtype == torch.bfloat16 and torch.equal(masks.cpu(), ref_masks)
    valid = ref_masks.squeeze(1)
    o, r, x = out.float().cpu()[valid], ref.float()[valid], exact[valid]
    d_ref = (o - r).abs()
    e_hip, e_ref = (o - x).abs(), (r - x).abs()
    parity_log.record(f"headline bf16/{what}", vs_matched_oracle_max=float(d_ref.max()), vs_matched_oracle_mean=float(d_ref.mean()),
                      hip_vs_exact_max=float(e_hip.max()), hip_vs_exact_mean=float(e_hip.mean()),
                      oracle_bf16_vs_exact_max=float(e_ref.max()), oracle_bf16_vs_exact_mean=float(e_ref.mean()))
    print(f"[headline bf16] {what}: vs matched-precision oracle max {float(d_ref.max()):.4g} mean {float(d_ref.mean()):.4g}; "
          f"vs exact model: HIP max {float(e_hip.max()):.4g} mean {float(e_hip.mean()):.4g}, oracle-bf16 max "
          f"{float(e_ref.max()):.4g} mean {float(e_ref.mean()):.4g}")
    # matched precision: two bf16 roundings of the same O(1) graph (ulp 0.03 at |x| = 4), 12 layers deep.  Bounds = 2 x the
    # values recorded in profiles/parity_r03.json (12 layers: max 0.196 / mean 0.0177; 2 layers: 0.086 / 0.0068)
    deep = conf["num_blocks"] > 2
    assert float(d_ref.mean()) <= (3.6e-2 if deep else 1.4e-2) and float(d_ref.max()) <= (0.4 if deep else 0.18)
    # against the exact model the HIP path is no further away than the reference's own bf16 arithmetic
    assert float(e_hip.mean()) <= 1.1 * float(e_ref.mean()) + 1e-3
    assert float(e_hip.max()) <= 1.5 * float(e_ref.max()) + 1e-2
    # tokens: flips only where the oracle itself is undecided at the measured noise
    flips = _token_parity(logp, ref_logp, valid, 0.25 if deep else 0.2, f"{what} vs matched-precision oracle")   # recorded 0.125 / 0.094
    # bf16 log-probs can tie EXACTLY; which maximiser a search returns is then implementation-defined (the reference's topk(1)
    # included), so whole token lists are compared only when neither side has a tie on a valid frame
    def _tied(lp):
        lp = lp.float().cpu()
        return bool((((lp == lp.max(-1, keepdim=True).values).sum(-1) > 1) & valid).any())
    if flips == 0 and not _tied(logp) and not _tied(ref_logp):
        assert toks == EO.ctc_greedy_search(ref_logp.float(), ref_masks.squeeze(1).sum(1), 0)
    # and the frame error rate against the exact model's tokens is not worse than the oracle's own
    ex_top = exact_logp.argmax(-1)
    fer_hip = float(((logp.float().cpu().argmax(-1) != ex_top) & valid).sum()) / float(valid.sum())
    fer_ref = float(((ref_logp.float().argmax(-1) != ex_top) & valid).sum()) / float(valid.sum())
    parity_log.record(f"headline bf16/{what}", frame_error_vs_exact_hip=fer_hip, frame_error_vs_exact_oracle_bf16=fer_ref)
    print(f"[headline bf16] {what}: frames whose token differs from the exact model's: HIP {fer_hip:.4f}, oracle-bf16 {fer_ref:.4f}")
    assert fer_hip <= fer_ref + 0.02
    if deep:
        _decisive_head_token_checks(out, ref, exact, valid, what)


def _decisive_head_token_checks(out, ref, exact, valid, what):
    """Tokens through a head that DECIDES.  A random-init 200-way head has near-uniform posteriors: two thirds of its frames
    have a top-2 margin below the bf16 noise, so token comparisons through it constrain little (the numbers above stay as
    the second data point).  Here the CTC head reads the leading principal direction(s) of the exact model's output -- the
    directions in which frames differ most: token = sign pattern of the top n components (blank = all-zero row, never
    the maximum), V = 1 + 2^n padded to 16 -- through the product's CTC module on the GPU (bf16) for the HIP output, the
    oracle's bf16 head for the matched-precision oracle and fp32 for the exact model.  Asserted (the criterion with teeth):
    frames whose HIP token differs from the exact model's <= frames whose ORACLE-bf16 token differs + 0.5 % of the frames.
    Recorded: both error rates, and how many frames are 'undecided' -- exact top-2 margin <= 2 e -- with e the max |dlogp|
    over the whole utterance (the round-3 rule) and per frame.  With the global max the share cannot drop below ~12-30 %
    for ANY linear head on these features (profiles/parity_r04.json 'decisive head' entries: the error distribution is
    heavy-tailed, max ~ 8 x median, and frames are Gaussian along every direction); per frame it is < 5 % for n = 1."""
    import itertools
    from oracle import encoder_oracle as EO
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    X = exact[valid]                                             # (frames, C) fp32, CPU
    mu = X.mean(0)
    _, _, V = torch.pca_lowrank(X - mu, q=8, center=False, niter=4)
    C = X.shape[1]
    for npc in (1, 3):
        P = V[:, :npc]
        rows = [torch.zeros(C)] + [(P * torch.tensor(pat)).sum(1) for pat in itertools.product([1.0, -1.0], repeat=npc)]
        W = torch.zeros(16, C)
        W[:len(rows)] = torch.stack(rows)
        W = W.to(torch.bfloat16)
        b = -(W.float() @ mu)
        b[len(rows):] = -60.0                                    # padding rows: never the maximum
        b = b.to(torch.bfloat16)
        head = CTC(16, C).to(torch.bfloat16)
        head.load_state_dict({"ctc_lo.weight": W, "ctc_lo.bias": b})
        with torch.no_grad():
            lp_hip = head.cuda().eval().log_softmax(out).float().cpu()
        lp_ref = EO.ctc_log_softmax(ref, {"ctc.ctc_lo.weight": W, "ctc.ctc_lo.bias": b}).float()
        lp_x = EO.ctc_log_softmax(exact, {"ctc.ctc_lo.weight": W.float(), "ctc.ctc_lo.bias": b.float()})
        n = float(valid.sum())
        top2 = lp_x.topk(2, dim=-1).values
        margin = top2[..., 0] - top2[..., 1]
        tok_x, tok_h, tok_r = lp_x.argmax(-1), lp_hip.argmax(-1), lp_ref.argmax(-1)
        fer_h = float(((tok_h != tok_x) & valid).sum()) / n
        fer_r = float(((tok_r != tok_x) & valid).sum()) / n
        nv = len(rows)                                           # (the padding rows sit at -60: never candidates, and a bf16
        e_h = ((lp_hip - lp_x)[..., :nv].abs().max(-1).values * valid)    # log-prob of that size is quantised to 0.25)
        e_r = ((lp_ref - lp_x)[..., :nv].abs().max(-1).values * valid)
        und = lambda e: float(((margin <= 2 * e) & valid).sum()) / n
        changes = int(((tok_x[:, 1:] != tok_x[:, :-1]) & valid[:, 1:]).sum())
        parity_log.record(f"decisive head n={npc}/{what}", vocab=len(rows), frames=int(n), exact_token_changes=changes,
                          frame_error_vs_exact_hip=fer_h, frame_error_vs_exact_oracle_bf16=fer_r,
                          max_abs_dlogp_hip_vs_exact=float(e_h.max()), max_abs_dlogp_oracle_vs_exact=float(e_r.max()),
                          undecided_global_rule_hip=und(e_h.max()), undecided_global_rule_oracle=und(e_r.max()),
                          undecided_per_frame_rule_hip=und(e_h), undecided_per_frame_rule_oracle=und(e_r),
                          decided_pct_per_frame_rule_hip=100.0 * (1.0 - und(e_h)))
        print(f"[decisive head n={npc}] {what}: token != exact model's on {fer_h:.4f} (HIP) / {fer_r:.4f} (oracle bf16) of the frames; "
              f"undecided per frame {und(e_h):.4f} / {und(e_r):.4f}, by the global max {und(e_h.max()):.4f} / {und(e_r.max()):.4f}")
        assert changes > 20                                      # the head emits a real token sequence, not a constant
        assert fer_h <= fer_r + 0.005, (npc, fer_h, fer_r)
        if npc == 1:
            assert und(e_h) < 0.05, und(e_h)                     # >= 95 % of the frames decided at the HIP path's own per-frame noise


def test_headline_bf16_bidirectional_reduced_vs_oracle(hip):
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_bf16slot")
    sd = {k: v for k, v in _sd(g).items() if not k.startswith("global_cmvn")}
    enc = ConformerEncoder(80, **g["conf"])
    enc.load_state_dict(sd)
    ctc = CTC(50, 128)
    ctc.load_state_dict(synth.synth_state_dict(g["ctc_spec"], g["ctc_seed"]))
    _bf16_headline(g["xs"], g["lens"], enc, ctc, g["conf"], "reduced 2-layer, ragged B=3")


def test_headline_bf16_bidirectional_full_size_c2_batch_vs_oracle(hip):
    """The bench's model (12 x 512, bidirectional, whole-model bf16) on a c2-shaped ragged batch -- decode batch trimmed
    from 64 to 8 utterances of 1-6 s so that the three CPU passes take seconds."""
    import bench
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    ctc = CTC(200, 512).eval()
    lens = torch.tensor([600, 577, 431, 402, 300, 222, 133, 100])
    xs = synth.randn((8, 600, 80), 903, 2.0)
    _bf16_headline(xs, lens, enc, ctc, conf, "full-size 12-layer, c2-shaped ragged B=8")


def test_headline_bf16_full_size_five_minute_file_vs_oracle(hip):
    """A 5-minute file (T = 30 000 frames, T' = 7 499) as ONE sequence through the bench's model and precision: the whole
    fused encoder + CTC head vs the matched-precision oracle and the exact model, element-wise and by token (the long-T
    whole-encoder comparison; the 30-minute shape itself is covered kernel by kernel in test_wkv6_gpu / test_fused_gpu)."""
    import bench
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    ctc = CTC(200, 512).eval()
    xs = synth.randn((1, 30000, 80), 904, 2.0)
    _bf16_headline(xs, torch.tensor([30000]), enc, ctc, conf, "full-size 12-layer, 5-minute file as one sequence")


def test_headline_bf16_layernorm_folded_schedule_vs_oracle(hip, monkeypatch):
    """The same 5-minute comparison through the schedule the 30-minute bench takes (it starts at 24 576 unmasked rows):
    norm_ff_macaron / norm_conv / norm_ff folded into the GEMMs either side of them (fused.layer_forward_lnfold), the
    normalised tensors never written.  Same bounds; the fold skips one bf16 rounding per folded norm, so it may only sit
    closer to the exact model."""
    import bench
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
            if ".norm_" in n and n.endswith("weight"):
                p.uniform_(0.7, 1.3)           # non-trivial gamma / beta: the fold multiplies them into the weights
            if ".norm_" in n and n.endswith("bias"):
                p.normal_(0, 0.1)
    ctc = CTC(200, 512).eval()
    xs = synth.randn((1, 30000, 80), 905, 2.0)
    monkeypatch.setattr(fused, "_LN_FOLD_MIN_ROWS", 6144)           # < 7 499 rows: the folded schedule is taken
    calls = []
    real = hip_ops.gemm_bf16_ln
    monkeypatch.setattr(hip_ops, "gemm_bf16_ln", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    _bf16_headline(xs, torch.tensor([30000]), enc, ctc, conf, "full-size 12-layer, 5-minute file, LayerNorms folded into the GEMMs")
    assert len(calls) == 12 * 5                                      # 3 consumers + 2 producers per layer


def test_bf16slot_full_size_vs_oracle(hip):
    """The YAML-default precision (fp32 model, bf16 slot returning fp32 -- what the reference CAN run) at full size on
    the same ragged batch: HIP fused path vs the oracle, bf16-inside tolerance, token rule as above."""
    import bench
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    ctc = CTC(200, 512).eval()
    lens = torch.tensor([600, 577, 431, 402, 300, 222, 133, 100])
    xs = synth.randn((8, 600, 80), 903, 2.0)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    ref, ref_masks = EO.encoder_forward(xs, lens, sd, conf, env={})
    ref_logp = EO.ctc_log_softmax(ref, {"ctc." + k: v for k, v in ctc.state_dict().items()})
    enc, ctc = enc.cuda(), ctc.cuda()
    with torch.no_grad():
        out, masks = enc(xs.cuda(), lens.cuda())
        logp = ctc.log_softmax(out)
    assert out.dtype == torch.float32 and torch.equal(masks.cpu(), ref_masks)
    valid = ref_masks.squeeze(1)
    d = (out.cpu()[valid] - ref[valid]).abs()
    parity_log.record("bf16slot full size", max_abs_err=float(d.max()), mean_abs_err=float(d.mean()))
    print(f"[bf16slot full size] max {float(d.max()):.4g} mean {float(d.mean()):.4g}")
    assert float(d.mean()) <= 1.6e-2 and float(d.max()) <= 0.12     # 24 bf16 slots deep; 2 x the recorded 0.0078 / 0.056
    _token_parity(logp, ref_logp, valid, 0.08, "bf16slot full size")   # recorded 0.035


def test_bf16slot_full_size_split_operand_path_vs_oracle(hip, monkeypatch):
    """The same comparison with the split-operand schedule of this precision (the default from 1 024 rows on) and with the
    library's exact fp32 products forced onto the same ragged batch: every fp32 projection of the layer, Linear(9728, 512) and the CTC head on the bf16 matrix cores with
    split operands, fp32 residual stream, bf16 slot.  Same bounds as the library-GEMM path above, and the two agree with
    each other to the noise of the bf16 slot."""
    import bench
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    ctc = CTC(256, 512).eval()
    lens = torch.tensor([600, 577, 431, 402, 300, 222, 133, 100])
    xs = synth.randn((8, 600, 80), 903, 2.0)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    ref, ref_masks = EO.encoder_forward(xs, lens, sd, conf, env={})
    ref_logp = EO.ctc_log_softmax(ref, {"ctc." + k: v for k, v in ctc.state_dict().items()})
    enc, ctc = enc.cuda(), ctc.cuda()
    with torch.no_grad():
        monkeypatch.setattr(fused, "_SPLIT_GEMM_MIN_ROWS", 1 << 40)       # the library's exact fp32 products first
        monkeypatch.setattr(hip_ops, "_SPLIT_GEMM_MIN_ROWS", 1 << 40)
        lib_out, _ = enc(xs.cuda(), lens.cuda())
        monkeypatch.setattr(fused, "_SPLIT_GEMM_MIN_ROWS", 0)
        monkeypatch.setattr(hip_ops, "_SPLIT_GEMM_MIN_ROWS", 0)
        assert all(fused.split_eligible(lp, lib_out) for lp in enc._fused(lib_out).layers)
        out, masks = enc(xs.cuda(), lens.cuda())
        logp = ctc.log_softmax(out)
    assert out.dtype == torch.float32 and torch.equal(masks.cpu(), ref_masks)
    valid = ref_masks.squeeze(1)
    d = (out.cpu()[valid] - ref[valid]).abs()
    dl = (out.cpu()[valid] - lib_out.cpu()[valid]).abs()
    parity_log.record("bf16slot full size, split-operand GEMMs", max_abs_err=float(d.max()), mean_abs_err=float(d.mean()),
                      vs_library_gemm_path_max=float(dl.max()), vs_library_gemm_path_mean=float(dl.mean()))
    assert float(d.mean()) <= 1.6e-2 and float(d.max()) <= 0.12
    assert float(dl.mean()) <= 1.6e-2 and float(dl.max()) <= 0.12
    _token_parity(logp, ref_logp, valid, 0.08, "bf16slot full size, split-operand GEMMs")


def test_bf16slot_unmasked_schedule_equals_masked_schedule(hip, monkeypatch):
    """The headline's schedule (fp32 model + bf16 slot, every row full length: the 30-minute file) drops the padding masks --
    pointwise_conv2's residual add rides on its GEMM, norm_conv zeroes nothing.  Forced here onto a short equal-length batch
    (it starts at 24 576 rows) and compared with the masked schedule of the same batch and with the oracle."""
    import bench
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    lens = torch.tensor([2403, 2403])
    xs = synth.randn((2, 2403, 80), 905, 2.0)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    ref, ref_masks = EO.encoder_forward(xs, lens, sd, conf, env={})
    enc = enc.cuda()
    calls = []
    real = fused.layer_forward_split
    monkeypatch.setattr(fused, "layer_forward_split", lambda plan, x, hp, lens_, *a: (calls.append(lens_ is None), real(plan, x, hp, lens_, *a))[1])
    with torch.no_grad():
        masked, m1 = enc(xs.cuda(), lens.cuda())
        assert calls and not any(calls)
        del calls[:]
        monkeypatch.setattr(fused, "_LN_FOLD_MIN_ROWS", 0)
        plain, m2 = enc(xs.cuda(), lens.cuda())
        assert calls and all(calls)                              # every layer ran without masks
    assert torch.equal(m1, m2) and torch.equal(m1.cpu(), ref_masks)
    dm = (plain - masked).abs()
    d = (plain.cpu() - ref).abs()
    parity_log.record("bf16slot unmasked schedule", vs_masked_schedule_max=float(dm.max()), vs_masked_schedule_mean=float(dm.mean()),
                      max_abs_err=float(d.max()), mean_abs_err=float(d.mean()))
    # the two schedules differ in where fp32 sums are rounded (GEMM epilogue vs LayerNorm pass): bf16-slot noise downstream
    assert float(dm.mean()) <= 1.6e-2 and float(dm.max()) <= 0.12
    assert float(d.mean()) <= 1.6e-2 and float(d.max()) <= 0.12


def test_bf16slot_full_size_five_minute_file_headline_schedule_vs_oracle(hip, monkeypatch):
    """The bench's precision AND schedule at a long-form shape: a 5-minute file (T = 30 000 -> 7 499 frames) as ONE sequence
    through the full-size fp32 model with the bf16 slot, on the schedule the 30-minute file takes (no padding masks, split-operand
    GEMMs with shared fragments, the chunked scan with its three passes), against the oracle in the same precision: element-wise,
    by token through a random 200-way head (margin rule) and through the deciding one-component head (flipped frames)."""
    import bench
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    ctc = CTC(200, 512).eval()
    xs = synth.randn((1, 30000, 80), 904, 2.0)
    lens = torch.tensor([30000])
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    ref, ref_masks = EO.encoder_forward(xs, lens, sd, conf, env={})
    ref_logp = EO.ctc_log_softmax(ref, {"ctc." + k: v for k, v in ctc.state_dict().items()})
    enc, ctc = enc.cuda(), ctc.cuda()
    ran = []
    real = fused.layer_forward_split
    monkeypatch.setattr(fused, "layer_forward_split", lambda plan, x, hp, lens_, *a: (ran.append(lens_ is None), real(plan, x, hp, lens_, *a))[1])
    monkeypatch.setattr(fused, "_LN_FOLD_MIN_ROWS", 4096)         # the unmasked schedule starts at 24 576 rows: brought down to this file
    with torch.no_grad():
        out, masks = enc(xs.cuda(), lens.cuda())
        logp = ctc.log_softmax(out)
    assert len(ran) == 12 and all(ran)                            # all twelve layers on the headline's schedule
    assert out.dtype == torch.float32 and torch.equal(masks.cpu(), ref_masks)
    valid = ref_masks.squeeze(1)
    d = (out.cpu()[valid] - ref[valid]).abs()
    parity_log.record("bf16slot 5-minute file, headline schedule", max_abs_err=float(d.max()), mean_abs_err=float(d.mean()),
                      frames=int(valid.sum()))
    print(f"[bf16slot 5-minute file] max {float(d.max()):.4g} mean {float(d.mean()):.4g}")
    # 24 bf16 slots deep over 7 499 frames: recorded max 0.107 / mean 0.0074 (short batches: 0.075 / 0.0077); bounds = 2 x
    assert float(d.mean()) <= 1.5e-2 and float(d.max()) <= 0.22
    _token_parity(logp, ref_logp, valid, 0.12, "bf16slot 5-minute file, headline schedule")
    # the deciding head: sign of the leading principal component of the oracle's output
    X = ref[valid]
    mu = X.mean(0)
    _, _, V = torch.pca_lowrank(X - mu, q=8, center=False, niter=4)
    W = torch.zeros(16, 512)
    W[1], W[2] = V[:, 0], -V[:, 0]
    b = -(W @ mu)
    b[3:] = -60.0
    head = CTC(16, 512)
    head.load_state_dict({"ctc_lo.weight": W, "ctc_lo.bias": b})
    with torch.no_grad():
        lp_hip = head.cuda().eval().log_softmax(out).float().cpu()
    lp_ref = EO.ctc_log_softmax(ref, {"ctc.ctc_lo.weight": W, "ctc.ctc_lo.bias": b})
    flipped = int(((lp_hip.argmax(-1) != lp_ref.argmax(-1)) & valid).sum())
    changes = int(((lp_ref.argmax(-1)[:, 1:] != lp_ref.argmax(-1)[:, :-1]) & valid[:, 1:]).sum())
    parity_log.record("bf16slot 5-minute file, headline schedule", deciding_head_frames_flipped=flipped, deciding_head_token_changes=changes)
    print(f"[bf16slot 5-minute file] deciding head: {flipped} of {int(valid.sum())} frames flipped, {changes} token changes")
    # recorded: 27 of 7 499 frames flipped among 2 925 token changes (the component changes sign every 2-3 frames on this model)
    assert changes > 100 and flipped <= 0.01 * float(valid.sum()), (flipped, changes)


def test_bf16slot_thirty_minute_file_vs_oracle(hip, monkeypatch):
    """The headline itself: `bench.build_model("bf16slot")` (fp32 model, bf16 time-mix slot, the 5000-way CTC head), the bench's
    own synthetic 30-minute file through the HIP fbank (T = 179 998 -> 44 998 frames) as ONE sequence, through
    `_forward_encoder` + `ctc_logprobs` exactly as `bench.py`'s timed step calls them (encoder-rtf.py:499-509), on the package's
    default dispatch -- nothing patched but a spy that records which schedule each layer took -- against the oracle on the WHOLE
    file in the same precision (one pass of `EO.encoder_forward` + `ctc_log_softmax` over all 179 998 frames on the host: about
    a minute on the GPU box's cores).  Element-wise at the 5-minute test's bounds, masks exact, tokens through the model's own
    5000-way head by the margin rule and through the deciding one-component head by flipped frames (<= 1 %).  This is the only
    place the split-operand GEMMs at 44 998 rows, conv2 over the 7.2 GB plane image (854 962 rows, ragged last tile) and the
    fp32 log-softmax at 44 998 x 5000 are compared with anything inside the model."""
    import time
    import bench
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    dev = torch.device("cuda")
    model, configs = bench.build_model("bf16slot", dev)
    conf = configs["encoder_conf"]
    wave = bench.synthetic_waveform(bench.AUDIO_SECONDS, 777)
    feats, _ = bench.front_end(wave, dev)
    assert feats.shape == (1, bench.FRAMES, 80) and feats.dtype == torch.float32
    lens = torch.tensor([bench.FRAMES], dtype=torch.int32, device=dev)
    ran = []
    real = fused.layer_forward_split
    monkeypatch.setattr(fused, "layer_forward_split", lambda plan, x, hp, lens_, *a: (ran.append(lens_ is None), real(plan, x, hp, lens_, *a))[1])
    with torch.no_grad():
        out, masks = model._forward_encoder(feats, lens)
        logp = model.ctc_logprobs(out)
        torch.cuda.synchronize()
        out2, _ = model._forward_encoder(feats, lens)              # a second pass on the warm plans: the timed steps' state
        logp2 = model.ctc_logprobs(out2)
    assert len(ran) == 24 and all(ran)                             # 12 layers x 2 passes, all on the unmasked split-operand schedule
    assert torch.equal(out, out2) and torch.equal(logp, logp2)     # run-to-run deterministic
    assert out.shape == (1, 44998, 512) and out.dtype == torch.float32 and logp.shape == (1, 44998, bench.VOCAB)
    out, logp = out.cpu(), logp.float().cpu()
    del out2, logp2
    # the oracle over the whole file (same state dict handling as bench.cpu_baseline)
    sd = {k: v.detach().float().cpu() for k, v in model.encoder.state_dict().items()}
    for k in list(sd):
        if ".tmix_block." in k and conf.get("rwkv_do_bfloat16", True):
            sd[k] = sd[k].to(torch.bfloat16)
    csd = {"ctc." + k: v.detach().float().cpu() for k, v in model.ctc.state_dict().items()}
    xs = feats.cpu()
    t0 = time.time()
    with torch.no_grad():
        ref, ref_masks = EO.encoder_forward(xs, torch.tensor([bench.FRAMES]), sd, conf, env={})
        ref_logp = EO.ctc_log_softmax(ref, csd)
    oracle_s = time.time() - t0
    assert torch.equal(masks.cpu(), ref_masks) and int(ref_masks.sum()) == 44998
    valid = ref_masks.squeeze(1)
    d = (out[valid] - ref[valid]).abs()
    what = "bf16slot 30-minute file (the headline), default schedule"
    parity_log.record(what, max_abs_err=float(d.max()), mean_abs_err=float(d.mean()), frames=int(valid.sum()),
                      ref_abs_max=float(ref.abs().max()), oracle_seconds=round(oracle_s, 1), oracle_threads=torch.get_num_threads())
    print(f"[bf16slot 30-minute file] max {float(d.max()):.4g} mean {float(d.mean()):.4g} (oracle {oracle_s:.0f} s)")
    # by quarter of the file: an indexing error late in the 7.2 GB image or in the last tiles would show as a jump
    q = [float((out[0, a:b] - ref[0, a:b]).abs().mean()) for a, b in ((0, 11250), (11250, 22500), (22500, 33750), (33750, 44998))]
    tail = float((out[0, -256:] - ref[0, -256:]).abs().max())
    parity_log.record(what, mean_abs_err_by_quarter=[round(v, 6) for v in q], max_abs_err_last_256_frames=tail)
    assert float(d.mean()) <= 1.5e-2 and float(d.max()) <= 0.22     # the 5-minute test's bounds
    assert max(q) <= 2.0 * min(q) + 1e-3 and tail <= 0.22
    _token_parity(logp, ref_logp, valid, 0.12, what)
    # the deciding head: sign of the leading principal component of the oracle's output
    X = ref[valid]
    mu = X.mean(0)
    _, _, V = torch.pca_lowrank(X - mu, q=8, center=False, niter=4)
    W = torch.zeros(16, 512)
    W[1], W[2] = V[:, 0], -V[:, 0]
    b = -(W @ mu)
    b[3:] = -60.0
    head = CTC(16, 512)
    head.load_state_dict({"ctc_lo.weight": W, "ctc_lo.bias": b})
    with torch.no_grad():
        lp_hip = head.cuda().eval().log_softmax(out.cuda()).float().cpu()
    lp_ref = EO.ctc_log_softmax(ref, {"ctc.ctc_lo.weight": W, "ctc.ctc_lo.bias": b})
    flipped = int(((lp_hip.argmax(-1) != lp_ref.argmax(-1)) & valid).sum())
    changes = int(((lp_ref.argmax(-1)[:, 1:] != lp_ref.argmax(-1)[:, :-1]) & valid[:, 1:]).sum())
    parity_log.record(what, deciding_head_frames_flipped=flipped, deciding_head_token_changes=changes)
    print(f"[bf16slot 30-minute file] deciding head: {flipped} of {int(valid.sum())} frames flipped, {changes} token changes")
    # recorded: 21 of 44 998 frames flipped among 208 token changes (on the bench's own weights -- zero-initialised LoRA matrices,
    # src/model.py:232-260 -- the leading component moves slowly; the 5-minute test above randomises them: 2 925 changes)
    assert changes > 100 and flipped <= 0.01 * float(valid.sum()), (flipped, changes)


@pytest.fixture(autouse=True)
def _restore_host_threads():
    n = torch.get_num_threads()
    yield
    torch.set_num_threads(n)


def test_bf16slot_token_lists_through_a_head_that_decides(hip):
    """Token LISTS in the reference's own precision (fp32 model + bf16 slot, the bench headline) through a head that decides.
    A c2-shaped ragged batch of 24 utterances (1-6 s) through the full-size 12-layer model; the CTC head reads the leading
    principal direction(s) of the oracle's output (token = sign pattern of the top n components, blank = zero row, V padded
    to 16), through the product's CTC module and GPU greedy search (search.py:106-121) for the HIP output and the oracle's own
    restatement for the reference.  With e_t = that frame's max |dlogp| (HIP vs oracle), a frame is DECIDED when the oracle's
    top-2 margin exceeds 2 e_t.  Asserted: (i) every utterance all of whose frames are decided yields the oracle's token list
    (collapsed, blanks removed); (ii) at most 0.5 % of the frames flip and >= 90 % of ALL utterances yield the oracle's list (a
    flip at a sign change moves the change by a frame, which the collapse absorbs -- lists differ only where the projection
    grazes zero).  The oracle runs on 16 host threads whatever the box has.  Recorded by tests/parity_log.py (parity_r06.json)."""
    import itertools
    import bench
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_greedy_search
    conf = bench.encoder_conf()
    torch.manual_seed(777)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    g = torch.Generator().manual_seed(4242)
    lens = torch.sort(torch.randint(100, 601, (24,), generator=g), descending=True).values
    xs = synth.randn((24, int(lens[0]), 80), 911, 2.0)
    for b, n in enumerate(lens.tolist()):
        xs[b, n:] = 0
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    # the oracle's fp32 sums follow the host's thread count (GEMM blocking, reduction splits): pinned, so that the reference
    # side of this comparison is the same computation on every box and what moves between boxes, if anything, is the HIP path
    torch.set_num_threads(16)                                     # (restored by the autouse fixture below, whatever happens)
    ref, ref_masks = EO.encoder_forward(xs, lens, sd, conf, env={})
    valid = ref_masks.squeeze(1)
    enc = enc.cuda()
    with torch.no_grad():
        out, masks = enc(xs.cuda(), lens.cuda())
    assert out.dtype == torch.float32 and torch.equal(masks.cpu(), ref_masks)
    X = ref[valid]
    mu = X.mean(0)
    _, _, V = torch.pca_lowrank(X - mu, q=8, center=False, niter=4)
    C = X.shape[1]
    olens = ref_masks.squeeze(1).sum(1)
    for npc in (1, 3):
        P = V[:, :npc]
        rows = [torch.zeros(C)] + [(P * torch.tensor(pat)).sum(1) for pat in itertools.product([1.0, -1.0], repeat=npc)]
        W = torch.zeros(16, C)
        W[:len(rows)] = torch.stack(rows)
        b = -(W @ mu)
        b[len(rows):] = -60.0
        head = CTC(16, C)
        head.load_state_dict({"ctc_lo.weight": W, "ctc_lo.bias": b})
        with torch.no_grad():
            lp_hip_dev = head.cuda().eval().log_softmax(out)
            toks_hip = [list(r.tokens) for r in ctc_greedy_search(lp_hip_dev, masks.squeeze(1).sum(1), 0)]
        lp_hip = lp_hip_dev.float().cpu()
        lp_ref = EO.ctc_log_softmax(ref, {"ctc.ctc_lo.weight": W, "ctc.ctc_lo.bias": b})
        toks_ref = EO.ctc_greedy_search(lp_ref, olens, 0)
        nv = len(rows)
        top2 = lp_ref.topk(2, dim=-1).values
        margin = top2[..., 0] - top2[..., 1]
        e_t = (lp_hip - lp_ref)[..., :nv].abs().max(-1).values
        decided = (margin > 2 * e_t) | ~valid
        same_frame = (lp_hip.argmax(-1) == lp_ref.argmax(-1)) | ~valid
        assert bool((same_frame | ~decided).all())               # (a decided frame cannot flip: the bound on e_t is what is tested)
        full = decided.all(1)
        equal = torch.tensor([a == b_ for a, b_ in zip(toks_hip, toks_ref)])
        n_utt = len(toks_ref)
        parity_log.record(f"bf16slot token lists, decisive head n={npc}", utterances=n_utt, vocab=nv,
                          utterances_fully_decided=int(full.sum()), token_lists_equal=int(equal.sum()),
                          token_lists_equal_among_fully_decided=int((equal & full).sum()),
                          frames=int(valid.sum()), frames_flipped=int((~same_frame).sum()),
                          frames_undecided=int((~decided).sum()), tokens_reference=int(sum(len(t) for t in toks_ref)),
                          max_abs_dlogp=float((e_t * valid).max()), oracle_threads=16)
        print(f"[bf16slot token lists n={npc}] {int(equal.sum())} of {n_utt} utterances decode to the oracle's token list "
              f"({int(full.sum())} fully decided, all of them equal: {bool((equal | ~full).all())}); "
              f"{int((~same_frame).sum())} of {int(valid.sum())} frames flipped, {int((~decided).sum())} undecided; "
              f"{sum(len(t) for t in toks_ref)} reference tokens")
        assert sum(len(t) for t in toks_ref) > 10 * n_utt         # a real token sequence per utterance, not a constant
        assert bool((equal | ~full).all()), "a fully decided utterance decodes to another token list"
        if npc == 1:
            # observed over five boxes: 24, 24, 24, 24 and 21 of 24 lists equal with 0-3 of 2 016 frames flipped (the oracle itself
            # moves by two tokens between boxes: its fp32 sums follow the host's thread count) -- a flipped frame at a sign change
            # that the collapse does not absorb costs one utterance, so the bar on the lists leaves room for four such frames
            assert int((~same_frame).sum()) <= 0.005 * float(valid.sum()), int((~same_frame).sum())
            assert int(equal.sum()) >= 0.9 * n_utt, (int(equal.sum()), n_utt)


def test_merged_window_launches_decode_the_same_token_lists(hip):
    """decode_windows(merge_frames=...) runs consecutive window batches as one launch -- the windows are independent, but kernel
    choice follows the rows per launch (below 1 024 rows the fp32 projections take exact fp32 products, above it split operands;
    the scan's chunking and the GEMM tiles differ too), so on a random-init 5000-way head, where most frames are near-ties, a few
    windows decode differently (bench.py counts them).  Through a head that DECIDES -- token = sign of the leading principal
    component of the encoder output, built from the literal schedule's own output -- the merged schedule must give the literal
    schedule's token list for (nearly) every window: full-size model in the headline precision, 24 windows of 1 000 frames in
    batches of 4 (996 rows per launch) against ONE launch of 24 windows (5 976 rows), both through the product's decode_windows."""
    import bench
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    from paper_accurate_fast_cheap_amd.utils.longform import decode_windows, feats_batcher
    torch.manual_seed(777)
    configs = dict(encoder="conformer", encoder_conf=bench.encoder_conf(), input_dim=80, output_dim=16, ctc="ctc",
                   ctc_conf={"ctc_blank_id": 0}, model_conf={}, dataset_conf={})

    class A:
        checkpoint = None

    model, _ = init_model(A(), configs)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    model = model.eval().cuda()
    chunk, batch, nwin = 1000, 4, 24
    feats = synth.randn((1, chunk * nwin, 80), 913, 2.0).cuda()
    with torch.no_grad():
        outs = [model._forward_encoder(fb, lens)[0] for fb, lens in feats_batcher(feats, chunk, batch, feats.device)]
    X = torch.cat([o.reshape(-1, 512) for o in outs]).float().cpu()
    mu = X.mean(0)
    _, _, V = torch.pca_lowrank(X - mu, q=8, center=False, niter=4)
    W = torch.zeros(16, 512)
    W[1], W[2] = V[:, 0], -V[:, 0]
    b = -(W @ mu)
    b[3:] = -60.0
    model.ctc.load_state_dict({"ctc_lo.weight": W, "ctc_lo.bias": b}, strict=False)
    model = model.cuda()
    with torch.no_grad():
        lit = decode_windows(model, feats, chunk, batch, streams=1, graph_cache=False)
        mer = decode_windows(model, feats, chunk, batch, streams=1, graph_cache=False, merge_frames=chunk * nwin)
        two = decode_windows(model, feats, chunk, batch, streams=2, merge_frames=2 * chunk * batch)     # 8 windows per launch, 2 in flight
        # frame by frame: the argmax of the literal schedule's log-probabilities against the one-launch schedule's
        lp_lit = torch.cat([model.ctc_logprobs(model._forward_encoder(fb, lens)[0]) for fb, lens in feats_batcher(feats, chunk, batch, feats.device)])
        fb_all, lens_all = next(iter(feats_batcher(feats, chunk, nwin, feats.device)))
        lp_mer = model.ctc_logprobs(model._forward_encoder(fb_all, lens_all)[0])
    assert len(lit["windows"]) == nwin == len(mer["windows"]) == len(two["windows"]) and lp_lit.shape == lp_mer.shape
    flipped = int((lp_lit.argmax(-1) != lp_mer.argmax(-1)).sum())
    frames = lp_lit.shape[0] * lp_lit.shape[1]

    def edits(x, y):                                               # Levenshtein distance of two token lists
        prev = list(range(len(y) + 1))
        for i, xi in enumerate(x, 1):
            cur = [i]
            for j, yj in enumerate(y, 1):
                cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (xi != yj)))
            prev = cur
        return prev[-1]
    same = sum(1 for x, y in zip(lit["windows"], mer["windows"]) if x == y)
    same2 = sum(1 for x, y in zip(lit["windows"], two["windows"]) if x == y)
    ed = sum(edits(x, y) for x, y in zip(lit["windows"], mer["windows"]))
    ed2 = sum(edits(x, y) for x, y in zip(lit["windows"], two["windows"]))
    ntok = sum(len(w) for w in lit["windows"])
    parity_log.record("merged window launches, decisive head", windows=nwin, tokens_literal_schedule=ntok, frames=frames,
                      frames_flipped_one_launch=flipped, windows_equal_one_launch=same, windows_equal_8_per_launch=same2,
                      token_edits_one_launch=ed, token_edits_8_per_launch=ed2)
    print(f"[merged windows] {flipped} of {frames} frames flipped; {same} / {same2} of {nwin} windows equal; {ed} / {ed2} token edits of {ntok} tokens")
    # the literal schedule runs 996 rows per launch (exact fp32 products below split_gemm_min_rows), the merged one 5 976 (split
    # operands, other scan chunking): bf16-slot noise on the frames where the component grazes zero.  The bars of the other
    # decisive-head tests: <= 0.5 % of the frames; a flipped frame that the collapse does not absorb costs two token edits
    assert ntok > 10 * nwin                                       # a real token sequence per window
    assert flipped <= 0.005 * frames, (flipped, frames)
    assert ed <= 0.02 * ntok and ed2 <= 0.02 * ntok, (ed, ed2, ntok)


@pytest.mark.parametrize("variant", ["bf16slot", "f32", "uni_bf16slot"])
def test_forward_chunk_by_chunk_golden(hip, variant):
    """BaseEncoder.forward_chunk_by_chunk vs the reference's own output (tests/golden/make_goldens_r2.py): the batched
    window path of the fused executor and the window-by-window module path both reproduce it."""
    from paper_accurate_fast_cheap_amd.transformer.cmvn import GlobalCMVN
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_chunk_by_chunk")
    c = g["cases"][variant]
    enc = ConformerEncoder(80, global_cmvn=GlobalCMVN(torch.zeros(80), torch.ones(80)), **c["conf"])
    enc.load_state_dict(_sd(c))
    enc = enc.cuda().eval()
    xs = g["xs"].cuda()
    bf = variant != "f32"
    with torch.no_grad():
        for chunk, want in c["outs"].items():
            for fused_on in (True, False):
                enc.fused_inference = fused_on
                ys, masks = enc.forward_chunk_by_chunk(xs, chunk, -1)
                assert torch.equal(masks.cpu(), want["masks"]) and ys.dtype == want["ys"].dtype
                _assert_close(ys, want["ys"], bf, f"{variant} chunk {chunk} fused={fused_on}")
        enc.fused_inference = True
        assert enc._windows_independent(xs) is not None            # the batched path is the one that ran above


@pytest.mark.parametrize("case", ["postnorm_f32", "postnorm_bf16slot", "abspos_f32", "abspos_bf16slot"])
def test_postnorm_and_abspos_goldens(hip, case):
    """Configurations outside the paper's YAMLs that the reference's classes support (tests/golden/make_goldens_r3.py):
    post-norm layers (module path; the fused executor is pre-norm only) and abs_pos, whose forward_chunk_by_chunk windows
    carry the running output offset and therefore must NOT take the batched-window path."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_postnorm_abspos")
    c = g["cases"][case]
    enc = ConformerEncoder(80, **c["conf"])
    enc.load_state_dict(_sd(c))
    enc = enc.cuda().eval()
    bf = case.endswith("bf16slot")
    with torch.no_grad():
        out, masks = enc(g["xs"].cuda(), g["lens"].cuda())
        assert torch.equal(masks.cpu(), c["masks"]) and out.dtype == c["out"].dtype
        _assert_close(out, c["out"], bf, case)
        if case.startswith("postnorm"):
            assert enc._fused(out) is None
        for chunk, want in c.get("chunks", {}).items():
            assert enc._windows_independent(out) is None
            ys, m = enc.forward_chunk_by_chunk(g["long"].cuda(), chunk, -1)
            assert torch.equal(m.cpu(), want["masks"])
            _assert_close(ys, want["ys"], bf, f"{case} chunk {chunk}")


def test_dir_dropout_train_golden(hip):
    """Train-time direction dropout: under torch.manual_seed(s) our modules make the reference's draws (same host
    generator, same order) and produce its outputs, every branch of both classes."""
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    g = load_golden("dir_dropout_train")
    sd = _sd(g)
    x = g["x"].cuda()
    mods = {}
    seen = set()
    for c in g["cases"]:
        if c["kind"] not in mods:
            m = WENET_ATTENTION_CLASSES[c["kind"]](64, 128, 4, "rwkv", "bi", 2048, True, 1)
            m.load_state_dict(sd)
            mods[c["kind"]] = m.cuda().train()
        torch.manual_seed(c["manual_seed"])
        with torch.no_grad():
            y, cache = mods[c["kind"]](x, x, x)
        assert y.dtype == c["y"].dtype
        _assert_close(y, c["y"], True, f"{c['kind']} seed {c['manual_seed']} ({c['branch']})")
        seen.add((c["both"], c["branch"]))
    assert seen == {(False, "bi"), (False, "left"), (True, "bi"), (True, "left"), (True, "right")}
    # and with autograd: the branch taken is the one that receives gradients
    m = mods["rwkv_tmix60_dir_layer_drop"]
    left_seed = next(c["manual_seed"] for c in g["cases"] if not c["both"] and c["branch"] == "left")
    torch.manual_seed(left_seed)
    m.zero_grad(set_to_none=True)
    y, _ = m(x, x, x)
    y.float().square().sum().backward()
    assert m.rwkv_wrapper_forward.tmix_block.receptance.weight.grad is not None
    assert m.rwkv_wrapper_backward.tmix_block.receptance.weight.grad is None


def test_cpu_tensors_fail_loudly(hip):
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    m = WENET_ATTENTION_CLASSES["rwkv_tmix60_bidirectional"](64, 128, 2, "rwkv", "bi", 2048, True, 0).eval()
    x = torch.randn(1, 9, 128)
    with pytest.raises(_lib.PafcError, match="no CPU fallback"):
        m(x, x, x)


@pytest.mark.parametrize("dtype", [torch.float32])
def test_state_carry_chunked_equals_full(hip, dtype):
    """Uni-directional slot + causal conv module: streaming with carried (token-shift, WKV state, conv cache)
    reproduces the full-sequence forward (BASELINE.md target c3; the reference has no carry at all)."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_uni_bf16slot")
    conf = dict(g["conf"], causal=True, rwkv_do_bfloat16=False, cnn_module_kernel=15)
    torch.manual_seed(5)
    enc = ConformerEncoder(80, **conf)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.05)
    enc = enc.cuda().eval()
    xs = synth.randn((1, 4 * 40 + 3, 80), 77, 2.0).cuda()
    with torch.no_grad():
        full, _ = enc(xs, torch.tensor([xs.size(1)], device="cuda"))
        chunk = 8
        stride, window = 4 * chunk, (chunk - 1) * 4 + 7
        outs, state, offset = [], None, 0
        for cur in range(0, xs.size(1) - 7 + 1, stride):
            y, state = enc.forward_chunk_carry(xs[:, cur:min(cur + window, xs.size(1))], offset, state)
            outs.append(y)
            offset += y.size(1)
    ys = torch.cat(outs, 1)
    assert ys.shape == full.shape
    torch.testing.assert_close(ys, full, rtol=1e-3, atol=2e-4)
    # stream_chunks = the same windows, the chunk step replayed from a captured hipGraph: equal to the eager loop up to
    # fp32 round-off (under capture the GEMM library may pick another algorithm) and to the full-sequence pass
    long = synth.randn((1, 4 * 8 * 14 + 3, 80), 78, 2.0).cuda()
    with torch.no_grad():
        eager = enc.stream_chunks(long, 8, use_graph=False)
        replayed = enc.stream_chunks(long, 8, use_graph=True)
        whole, _ = enc(long, torch.tensor([long.size(1)], device="cuda"))
    assert replayed.shape == eager.shape == whole.shape
    torch.testing.assert_close(replayed, eager, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(replayed, whole, rtol=1e-3, atol=2e-4)


def test_fused_state_carry_step_matches_module_path(hip):
    """bf16 stream (B = 1, causal conv): the chunk step on the fused kernels (fused.layer_forward_carry) carries the
    same three states and produces the module path's outputs to bf16 round-off; carried scan state to fp32 round-off."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_uni_bf16model")
    conf = dict(g["conf"], causal=True, cnn_module_kernel=15)
    torch.manual_seed(6)
    enc = ConformerEncoder(80, **conf)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.05)
    enc = enc.to(torch.bfloat16).cuda().eval()
    xs = synth.randn((1, 4 * 8 * 9 + 3, 80), 79, 2.0).to(torch.bfloat16).cuda()
    with torch.no_grad():
        enc.fused_inference = True
        a = enc.stream_chunks(xs, 8, use_graph=False)
        assert getattr(enc, "_carry_plans", None) is not None        # the fused step really ran
        _, st_f = enc.forward_chunk_carry(xs[:, :35], 0, None)
        enc.fused_inference = False
        b = enc.stream_chunks(xs, 8, use_graph=False)
        _, st_m = enc.forward_chunk_carry(xs[:, :35], 0, None)
        enc.fused_inference = True
        c = enc.stream_chunks(xs, 8, use_graph=True)
    assert a.shape == b.shape == c.shape
    d = (a.float() - b.float()).abs()
    assert float(d.mean()) < 2e-2 and float(d.max()) < 0.4, (float(d.mean()), float(d.max()))
    d = (a.float() - c.float()).abs()
    assert float(d.mean()) < 2e-2 and float(d.max()) < 0.4
    for f, m in zip(st_f, st_m):
        assert set(f) == set(m) == {"shift", "wkv", "cnn"}
        assert f["cnn"].shape == m["cnn"].shape and f["shift"].shape == m["shift"].shape
    torch.testing.assert_close(st_f[0]["wkv"], st_m[0]["wkv"], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(st_f[0]["cnn"].float(), st_m[0]["cnn"].float(), rtol=5e-2, atol=5e-2)


def test_fused_state_carry_captured_step_keeps_its_carries_in_place(hip, monkeypatch):
    """One stream, chunks at least as long as the causal conv's left context: the captured step keeps the conv module's input
    buffer across steps (no concatenation), updates the scan state where it lies and refreshes all carries in one
    multi-tensor copy -- replayed == eager == (to bf16 round-off) the whole sequence, and the public carries come back."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_uni_bf16model")
    conf = dict(g["conf"], causal=True, cnn_module_kernel=15)
    torch.manual_seed(6)
    enc = ConformerEncoder(80, **conf)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.05)
    enc = enc.to(torch.bfloat16).cuda().eval()
    chunk = 16                                                       # >= lorder = 14
    xs = synth.randn((1, 4 * chunk * 12 + 3, 80), 81, 2.0).to(torch.bfloat16).cuda()
    with torch.no_grad():
        enc.fused_inference = True
        eager = enc.stream_chunks(xs, chunk, use_graph=False)
        refreshed = []
        real = torch._foreach_copy_
        monkeypatch.setattr(torch, "_foreach_copy_", lambda d, s_: (refreshed.append(len(d)), real(d, s_))[1])
        replayed = enc.stream_chunks(xs, chunk, use_graph=True)
        monkeypatch.undo()
        assert refreshed == [2 * len(enc.encoders)]      # captured once: shift + conv-input refresh of every layer, one launch
        whole, _ = enc(xs, torch.tensor([xs.size(1)], device="cuda"))
        # the carries after a captured run are the public ones again
        sub, ctx = enc.embed.subsampling_rate, enc.embed.right_context + 1
        win = (chunk - 1) * sub + ctx
        _, st = enc.forward_chunk_carry(xs[:, :win], 0, None)
        _, st2 = enc.forward_chunk_carry(xs[:, sub * chunk:sub * chunk + win], 0, st)
    assert replayed.shape == eager.shape
    d = (replayed.float() - eager.float()).abs()
    assert float(d.mean()) < 2e-2 and float(d.max()) < 0.4, (float(d.mean()), float(d.max()))
    n = min(whole.shape[1], replayed.shape[1])
    d = (replayed[:, :n].float() - whole[:, :n].float()).abs()
    assert float(d.mean()) < 3e-2 and float(d.max()) < 0.6, (float(d.mean()), float(d.max()))
    assert set(st2[0]) == {"shift", "wkv", "cnn"} and st2[0]["cnn"].shape == st[0]["cnn"].shape


def test_fused_state_carry_step_serves_concurrent_streams(hip):
    """B independent streams per chunk step (the serving shape): stream b of a batched run equals the same stream run
    alone -- the carries are per stream, nothing leaks across the batch -- eagerly and from the replayed hipGraph."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_uni_bf16model")
    conf = dict(g["conf"], causal=True, cnn_module_kernel=15)
    torch.manual_seed(6)
    enc = ConformerEncoder(80, **conf)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.05)
    enc = enc.to(torch.bfloat16).cuda().eval()
    xs = synth.randn((3, 4 * 8 * 9 + 3, 80), 80, 2.0).to(torch.bfloat16).cuda()
    with torch.no_grad():
        enc.fused_inference = True                              # whatever PAFC_DISABLE_FUSED says
        both = enc.stream_chunks(xs, 8, use_graph=False)
        assert getattr(enc, "_carry_plans", None) is not None
        _, st = enc.forward_chunk_carry(xs[:, :35], 0, None)
        assert st[0]["wkv"].shape[0] == 3 and st[0]["shift"].shape == (3, 1, enc.output_size())
        assert st[0]["cnn"].shape[0] == 3
        graphed = enc.stream_chunks(xs, 8, use_graph=True)
        for b in range(3):
            alone = enc.stream_chunks(xs[b:b + 1].contiguous(), 8, use_graph=False)
            # same kernels on the same rows; only the GEMM tile a row lands in differs with the batch
            d = (both[b:b + 1].float() - alone.float()).abs()
            assert float(d.mean()) < 5e-3 and float(d.max()) < 0.15, (b, float(d.mean()), float(d.max()))
        d = (both.float() - graphed.float()).abs()
        assert float(d.mean()) < 5e-3 and float(d.max()) < 0.15
        enc.fused_inference = False
        module = enc.stream_chunks(xs, 8, use_graph=False)
    d = (both.float() - module.float()).abs()
    assert float(d.mean()) < 2e-2 and float(d.max()) < 0.4


def test_graph_cache_replays_recurring_batch_shapes(hip):
    """Opt-in hipGraph cache (encoder.graph_cache_size): the third batch of a shape is replayed from the graph captured
    at the second; outputs and masks equal the eager forward (fp32 round-off: the GEMM library may pick differently
    under capture), new lengths are honoured, other shapes stay eager, the cache stays bounded."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_f32")
    sd = {k: v for k, v in _sd(g).items() if not k.startswith("global_cmvn")}
    enc = ConformerEncoder(80, **g["conf"])
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    xs = [synth.randn((3, 95, 80), 90 + i, 2.0).cuda() for i in range(4)]
    lens = [torch.tensor(v, device="cuda") for v in ([95, 60, 33], [95, 95, 95], [95, 41, 17], [70, 95, 8])]
    with torch.no_grad():
        want = [enc(x, l) for x, l in zip(xs, lens)]
        enc.graph_cache_size = 1
        got = [enc(x, l) for x, l in zip(xs, lens)]
        assert isinstance(enc._graphs[((3, 95, 80), torch.float32, torch.int64, torch.cuda.current_stream().cuda_stream, None)], tuple)
        other = enc(xs[0][:, :71], torch.tensor([71, 30, 9], device="cuda"))         # another shape: eager, then captured
        other2 = enc(xs[0][:, :71], torch.tensor([71, 30, 9], device="cuda"))
        assert sum(isinstance(v, tuple) for v in enc._graphs.values()) == 1            # bounded: the older graph is gone
    for (wy, wm), (gy, gm) in zip(want, got):
        assert torch.equal(wm, gm)
        torch.testing.assert_close(gy, wy, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(other[0], other2[0], rtol=1e-4, atol=2e-5)


def test_graph_cache_two_batches_in_flight(hip):
    """Two decode batches in flight on two HIP streams (bench.py's window leg): the graph cache keeps one graph per (shape,
    stream), the replays of the two streams overlap, and every batch's output equals its one-stream replay bit for bit."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_f32")
    sd = {k: v for k, v in _sd(g).items() if not k.startswith("global_cmvn")}
    enc = ConformerEncoder(80, **g["conf"])
    enc.load_state_dict(sd)
    enc = enc.cuda().eval().to(torch.bfloat16)
    xs = [synth.randn((4, 203, 80), 300 + i, 2.0).cuda().to(torch.bfloat16) for i in range(6)]
    lens = torch.tensor([203, 203, 203, 203], device="cuda")
    side = [torch.cuda.Stream() for _ in range(2)]

    def one_pass(streams):
        main = torch.cuda.current_stream()
        for s_ in streams:
            s_.wait_stream(main)
        outs = []
        for i, x in enumerate(xs):
            if streams:
                with torch.cuda.stream(streams[i % 2]):
                    outs.append(enc(x, lens)[0])
            else:
                outs.append(enc(x, lens)[0])
        for s_ in streams:
            main.wait_stream(s_)
        torch.cuda.synchronize()
        return outs

    with torch.no_grad():
        enc.graph_cache_size = 4
        for _ in range(3):                       # seen, captured, replayed
            single = one_pass([])
        for _ in range(3):
            double = one_pass(side)
        assert sum(isinstance(v, tuple) for v in enc._graphs.values()) == 3       # the main stream's graph + one per side stream
    for a, b in zip(single, double):
        assert torch.equal(a, b)


def test_graph_replay_runs_the_schedule_of_the_eager_pass(hip, monkeypatch):
    """A long batch whose rows are all full length takes the schedule without padding masks, a decision that reads the lengths
    on the host.  The hipGraph cache takes it BEFORE capturing and keys the graph on it: replays of equal-length batches equal
    the eager pass bit for bit (whole-model bf16: the folded-LayerNorm schedule), and a batch of the same shape with a short row
    gets a graph of its own (the masked schedule) instead of a wrong replay.  "Full length" is counted in SUBSAMPLED frames, as the
    eager pass counts it: a row two input frames short of T that still yields all T' output frames takes the unmasked schedule
    eagerly and must replay that same schedule (the graph of the all-full batch)."""
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    import bench
    conf = dict(bench.encoder_conf(), num_blocks=2)
    torch.manual_seed(9)
    enc = ConformerEncoder(80, **conf).eval().to(torch.bfloat16).cuda()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.02)
    monkeypatch.setattr(fused, "_LN_FOLD_MIN_ROWS", 256)          # the schedule's threshold (24 576 rows) brought down to this batch
    xs = [synth.randn((2, 805, 80), 500 + i, 2.0).cuda().to(torch.bfloat16) for i in range(3)]
    full = torch.tensor([805, 805], device="cuda")
    ragged = torch.tensor([805, 411], device="cuda")
    almost = torch.tensor([805, 803], device="cuda")             # (803 - 7) // 4 + 1 = 200 = T': every output frame is valid
    seen = []
    real = fused.layer_forward_lnfold
    monkeypatch.setattr(fused, "layer_forward_lnfold", lambda *a, **k: (seen.append(torch.cuda.is_current_stream_capturing()), real(*a, **k))[1])
    with torch.no_grad():
        want = [enc(x, full)[0] for x in xs]
        want_r = enc(xs[0], ragged)[0]
        n_unmasked = len(seen)
        want_a = enc(xs[1], almost)[0]
        assert len(seen) == n_unmasked + 2 and not any(seen)     # eager: the almost-full batch took the unmasked schedule too
        del seen[:]
        enc.graph_cache_size = 4
        for _ in range(3):                                       # seen, captured, replayed
            got = [enc(x, full)[0] for x in xs]
            got_r = enc(xs[0], ragged)[0]
            got_a = enc(xs[1], almost)[0]
        assert any(seen)                                         # the folded-LayerNorm schedule was CAPTURED
        keys = [k for k, v in enc._graphs.items() if isinstance(v, tuple)]
        assert sorted(k[-1] for k in keys) == [False, True]      # one graph per answer
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert torch.equal(want_r, got_r)
    assert torch.equal(want_a, got_a) and torch.equal(want_a, want[1])   # (frames 803, 804 are read by no valid output frame)
    enc.graph_cache_size = 0
    enc._graphs.clear()


def test_graph_cache_follows_parameter_updates(hip):
    """A captured graph holds the addresses of the plans' derived weights and never refreshes them: after ANY parameter change
    -- an in-place update (optimizer step: Tensor._version moves), load_state_dict, a fused-optimizer style write behind torch's
    back followed by hip_ops.bump_param_epoch(), .to() -- the next decode_windows must not replay a stale graph.  Compared with
    the eager pass of an identical model after every change."""
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    from paper_accurate_fast_cheap_amd.utils.longform import decode_windows
    g = load_golden("encoder_reduced_f32")
    conf = dict(g["conf"], rwkv_do_bfloat16=True)
    configs = dict(encoder="conformer", encoder_conf=conf, input_dim=80, output_dim=40, ctc="ctc",
                   ctc_conf={"ctc_blank_id": 0}, model_conf={}, dataset_conf={})

    class A:
        checkpoint = None

    torch.manual_seed(5)
    model, _ = init_model(A(), configs)
    model = model.eval().to(torch.bfloat16).cuda()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):
                p.normal_(0, 0.05)
    feats = synth.randn((1, 6 * 4 * 203, 80), 77, 2.0).cuda().to(torch.bfloat16)

    def eager_reference():              # a FRESH model with the same parameters, no graph, one stream
        ref, _ = init_model(A(), configs)
        ref = ref.eval().to(torch.bfloat16).cuda()
        ref.load_state_dict(model.state_dict())
        return decode_windows(ref, feats, 203, 4, streams=1, graph_cache=False)

    def graphed():
        out = None
        for _ in range(3):                    # seen, captured, replayed
            out = decode_windows(model, feats, 203, 4, streams=2)
        assert any(isinstance(v, tuple) for v in model.encoder._graphs.values())
        return out

    first = graphed()
    assert first["windows"] == eager_reference()["windows"]
    changes = []
    with torch.no_grad():
        w = model.encoder.encoders[0].feed_forward.w_2.weight
        w.mul_(-1.0)                                                        # in place: _version moves
        changes.append("in-place update")
        got = graphed()
        assert got["windows"] == eager_reference()["windows"], changes[-1]
        assert got["windows"] != first["windows"]                           # (the change matters)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        k0 = "encoder.encoders.1.self_attn.rwkv_wrapper_forward.tmix_block.output.weight"
        sd[k0] = -sd[k0]
        model.load_state_dict(sd)
        changes.append("load_state_dict")
        got2 = graphed()
        assert got2["windows"] == eager_reference()["windows"], changes[-1]
        model.encoder.encoders[1].feed_forward.w_1.weight.data.neg_()        # .data write: no version bump -> the caller's duty
        hip_ops.bump_param_epoch()
        changes.append("data write + bump_param_epoch")
        got3 = graphed()
        assert got3["windows"] == eager_reference()["windows"], changes[-1]
    model.encoder.graph_cache_size = 0
    model.encoder._graphs.clear()


_REFUSED_CAPTURE_CHILD = r"""
import os, sys, torch
sys.path.insert(0, os.environ["PAFC_ROOT"])
from tests import synth
from tests.conftest import load_golden
from paper_accurate_fast_cheap_amd.transformer import fused
from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
g = load_golden("encoder_reduced_f32")
sd = {k: v for k, v in synth.synth_state_dict(g["spec"], g["seed"]).items() if not k.startswith("global_cmvn")}
enc = ConformerEncoder(80, **g["conf"])
enc.load_state_dict(sd)
enc = enc.cuda().eval()
x = synth.randn((2, 95, 80), 31, 2.0).cuda()
lens = torch.tensor([95, 60], device="cuda")
real = fused.encoder_layers_forward
def refused(*a, **kw):
    if torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize()              # not permitted under capture: the runtime refuses (hipErrorStreamCapture*)
    return real(*a, **kw)
with torch.no_grad():
    want = enc(x, lens)[0].cpu()
    enc.graph_cache_size = 2
    enc(x, lens)                              # first sighting: eager
    fused.encoder_layers_forward = refused
    try:
        got = enc(x, lens)[0]                 # second sighting: the capture is refused -> this shape stays eager
        states = [v for v in enc._graphs.values()]
        ok = states == ["eager"] and torch.allclose(got.cpu(), want, rtol=1e-4, atol=2e-5)
        print("FALLBACK", "OK" if ok else f"WRONG {states}", flush=True)
    except BaseException as e:                # (a runtime that cannot recover inside this process says so here)
        print("FALLBACK RAISED", type(e).__name__, str(e)[:200], flush=True)
os._exit(0)                                   # the refused capture may have left the process's HIP state unusable: no teardown
"""


def test_refused_capture_is_never_silent_in_a_child_process(hip):
    """BaseEncoder._forward_graphed marks a shape "eager" when the RUNTIME refuses its capture (an operation the capture mode does
    not permit), as opposed to an error of the captured work, which surfaces (next test), ends the refused capture by hand
    (encoder._abandon_capture) and runs the call eagerly.  Staged in a child process (a synchronize under capture), because on
    this runtime (ROCm 7.0 HIP inside torch 2.10) an invalidated capture poisons the process: every later HIP call reports
    hipErrorStreamCaptureInvalidated, whatever is done to the stream -- found in round 5 the hard way, re-measured in round 6 with
    hipStreamEndCapture + hipGetLastError by hand.  What is asserted is what a caller can rely on: EITHER the call returns the
    eager result and the shape is marked "eager" (a runtime that recovers), OR the error that comes back names the capture
    (this runtime) -- never a wrong result, never a hang.  Which of the two happened is recorded by tests/parity_log.py
    (parity_r06.json)."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    env = dict(os.environ, PAFC_ROOT=ROOT, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _REFUSED_CAPTURE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout
    recovered = "FALLBACK OK" in out
    named = "FALLBACK RAISED" in out and "captur" in out.lower()
    parity_log.record("refused hipGraph capture (child process)", outcome="eager fallback" if recovered else
                      "error naming the capture" if named else "UNEXPECTED")
    assert recovered or named, (r.returncode, out[-500:], r.stderr[-1500:])


def test_graph_capture_errors_surface(hip, monkeypatch):
    """An error of the captured work itself (a failing launch, a PafcError from the C ABI) is raised to the caller, not turned
    into "eager from now on"; only a capture the runtime REFUSES (hipErrorStreamCapture*) falls back (previous test, in a child
    process: on this runtime an operation that invalidates a global-mode capture also fails the next unrelated call)."""
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_f32")
    sd = {k: v for k, v in _sd(g).items() if not k.startswith("global_cmvn")}
    enc = ConformerEncoder(80, **g["conf"])
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    x = synth.randn((2, 95, 80), 31, 2.0).cuda()
    lens = torch.tensor([95, 60], device="cuda")
    real = fused.encoder_layers_forward
    with torch.no_grad():
        want = enc(x, lens)[0]
        enc.graph_cache_size = 2
        enc(x, lens)                                                       # first sighting: eager

        def failing(*a, **kw):
            if torch.cuda.is_current_stream_capturing():
                raise _lib.PafcError("pafc_add_layernorm: PAFC_ERR_LAUNCH (injected)")
            return real(*a, **kw)
        monkeypatch.setattr(fused, "encoder_layers_forward", failing)
        with pytest.raises(_lib.PafcError, match="injected"):
            enc(x, lens)                                                   # second sighting: capture -> the error surfaces
        torch.cuda.synchronize()
        # ... and leaves the encoder usable: the same shape runs eagerly, is captured on its next sighting and replays
        monkeypatch.setattr(fused, "encoder_layers_forward", real)
        enc._graphs.clear()
        for _ in range(3):
            got = enc(x, lens)[0]
        assert any(isinstance(v, tuple) for v in enc._graphs.values())
        torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-5)
    enc.graph_cache_size = 0
    enc._graphs.clear()


def test_minimal_and_ragged_edge_inputs(hip):
    """Shortest input the subsampling accepts (7 frames -> T' = 1), a batch whose shortest member is that short, and
    lengths that are not multiples of anything: fused executor == module path, masks exact, outputs finite."""
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    g = load_golden("encoder_reduced_f32")
    sd = {k: v for k, v in _sd(g).items() if not k.startswith("global_cmvn")}
    enc = ConformerEncoder(80, **g["conf"])
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    for xs, lens in ((synth.randn((1, 7, 80), 1), torch.tensor([7])),
                     (synth.randn((3, 45, 80), 2), torch.tensor([45, 7, 23]))):
        ref, ref_masks = EO.encoder_forward(xs, lens, sd, g["conf"], env={})
        with torch.no_grad():
            out, masks = enc(xs.cuda(), lens.cuda())
        assert torch.equal(masks.cpu(), ref_masks) and torch.isfinite(out).all()
        _assert_close(out, ref, False, "edge")


def test_full_size_encoder_properties(hip):
    """BASELINE sizes (12 layers x 512, bf16 model, 5-minute and 30-minute files): the fused executor agrees with
    the op-by-op module path on the 5-minute file (bf16 tolerance), and the 30-minute single-sequence pass (T' =
    44 998, the bench workload) is finite with the expected shape."""
    import bench
    model, configs = bench.build_model("bf16", torch.device("cuda"))
    enc = model.encoder
    g = torch.Generator(device="cuda").manual_seed(3)
    x5 = (torch.randn(1, 30000, 80, device="cuda", generator=g) * 2 + 8).to(torch.bfloat16)
    lens5 = torch.tensor([30000], device="cuda")
    with torch.no_grad():
        a, ma = enc(x5, lens5)
        enc.fused_inference = False
        b, mb = enc(x5, lens5)
        enc.fused_inference = True
        assert a.shape == (1, 7499, 512) and torch.equal(ma, mb)
        d = (a.float() - b.float()).abs()
        assert float(d.mean()) < 2e-2 and float(d.max()) < 0.6, (float(d.mean()), float(d.max()))
        x30 = (torch.randn(1, 179998, 80, device="cuda", generator=g) * 2 + 8).to(torch.bfloat16)
        out, m = enc(x30, torch.tensor([179998], device="cuda"))
        assert out.shape == (1, 44998, 512) and int(m.sum()) == 44998 and bool(torch.isfinite(out).all())
