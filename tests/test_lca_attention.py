"""Limited-context attention of the Conformer baseline (`limited_rel_selfattn`), the parts that need no GPU: the float64
restatement (tests/lca_ref.py) against the fixtures captured from the reference (tests/golden/make_goldens_lca.py), the plugin
surface (registry, constructor, state dict, encoder, init_model, install_into), the argument errors, and pafc_mha_band's checks
before any launch."""
import pytest
import torch

from tests import lca_ref, synth
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("lca_attention")


def _case_inputs(g, c, dtype=torch.float64):
    x = synth.randn((c["B"], c["T"], g["d"]), c["seed"]).to(dtype)
    pos = g["pos_rows"][:, :c["T"]].to(dtype)
    sd = {k: v.to(dtype) for k, v in synth.synth_state_dict(g["spec"], g["weight_seed"]).items()}
    return x, pos, sd


def test_restatement_equals_every_attention_golden(gold):
    assert synth.checksum(synth.synth_state_dict(gold["spec"], gold["weight_seed"])) == pytest.approx(gold["checksum"], rel=1e-12)
    assert {(c["w"], c["B"], c["T"]) for c in gold["cases"]} == {
        (w, B, T) for w in (2, 5, 16) for B, T in ((1, 1), (2, 2 * w), (3, 2 * w + 1), (2, 4 * w + 3), (1, 67))}
    # the fixture's position rows are the table at a non-zero offset
    assert gold["pos_offset"] > 0
    assert torch.equal(gold["pos_rows"], lca_ref.position_rows(gold["pos_offset"], 67, gold["d"], torch.float32))
    for c in gold["cases"]:
        x, pos, sd = _case_inputs(gold, c)
        out, cache = lca_ref.lca_attention(x, pos, sd, gold["heads"], c["w"])
        assert out.dtype == torch.float64
        err = (out - c["out"]).abs().max().item()
        assert err <= 1e-12, (c["w"], c["B"], c["T"], err)
        assert tuple(cache.shape) == c["cache_shape"]
        assert (cache[:, :, c["cache_frames"]] - c["cache_at"]).abs().max().item() <= 1e-12


def test_fixture_pins_the_padding_keys(gold):
    """Restated with T_pad = T (padding keys masked, what a tidy implementation would do) the output must DIFFER from the
    reference's at (3, 2w + 1): there T_pad = 4w and the last w frames see unmasked zero keys."""
    for c in gold["cases"]:
        if (c["B"], c["T"]) != (3, 2 * c["w"] + 1):
            continue
        x, pos, sd = _case_inputs(gold, c)
        out, _ = lca_ref.lca_attention(x, pos, sd, gold["heads"], c["w"], t_pad=c["T"])
        diff = (out - c["out"]).abs().amax(dim=(0, 2))                       # per frame
        w, T = c["w"], c["T"]
        assert diff[T - w:].min().item() > 1e-6, (w, diff)                   # every one of the last w frames
        assert diff[:T - w].max().item() <= 1e-12, (w, diff)                 # and no other


def test_registry_constructor_and_state_dict(gold):
    from paper_accurate_fast_cheap_amd.transformer.attention import LimitedRelPositionMultiHeadedAttention
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES
    assert WENET_ATTENTION_CLASSES["limited_rel_selfattn"] is LimitedRelPositionMultiHeadedAttention
    # the positional constructor as the reference encoder calls it: (n_head, n_feat, dropout_rate, key_bias, att_context_size,
    # global_tokens, global_tokens_spacing, global_attn_separate) + layer_id
    m = WENET_ATTENTION_CLASSES["limited_rel_selfattn"](2, 128, 0.1, True, [16, 16], 0, 1, False, 3)
    assert synth.spec_of(m.state_dict()) == gold["spec"]
    m.load_state_dict(synth.synth_state_dict(gold["spec"], gold["weight_seed"]), strict=True)
    assert m.att_context_size == [16, 16] and m.h == 2 and m.d_k == 64
    nb = WENET_ATTENTION_CLASSES["limited_rel_selfattn"](2, 128, 0.0, False, [4, 4], 0, 1, False, 0)
    assert nb.linear_k.bias is None and "linear_k.bias" not in nb.state_dict()


def test_argument_errors():
    from paper_accurate_fast_cheap_amd.transformer.attention import LimitedRelPositionMultiHeadedAttention as A
    with pytest.raises(ValueError, match="att_context_size"):
        A(2, 128, 0.0, True, [4, 2])
    with pytest.raises(ValueError, match="att_context_size"):
        A(2, 128, 0.0, True, [1, 1])
    with pytest.raises(NotImplementedError, match="global_tokens"):
        A(2, 128, 0.0, True, [4, 4], 1)
    with pytest.raises(NotImplementedError, match="global_attn_separate"):
        A(2, 128, 0.0, True, [4, 4], 0, 1, True)
    m = A(2, 128, 0.0, True, [4, 4]).eval()
    x = torch.zeros(1, 5, 128)
    with torch.no_grad(), pytest.raises(ValueError, match="cache"):
        m(x, x, x, torch.ones(1, 1, 5, dtype=torch.bool), torch.zeros(1, 5, 128), torch.zeros(1, 2, 3, 128))
    # inference only: with gradients enabled and trainable parameters the call is refused, not answered without a graph
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x, x, x, torch.ones(1, 1, 5, dtype=torch.bool), torch.zeros(1, 5, 128))


# encoder_conf of the reference's conf/conformer/giga.conformer_ds4k31nc_12le.LCA256-GT-FT-LFXL.max.yaml (settings only)
SHIPPED_ENCODER_CONF = dict(
    activation_type="swish", attention_dropout_rate=0.0, attention_heads=8, cnn_module_kernel=31, cnn_module_norm="layer_norm",
    dropout_rate=0.1, input_layer="conv2d", linear_units=2048, normalize_before=True, num_blocks=12, output_size=512,
    pos_enc_layer_type="rel_pos", positional_dropout_rate=0.1, use_cnn_module=True,
    selfattention_layer_type="limited_rel_selfattn", att_context_size=[256, 256], global_tokens=0, global_tokens_spacing=1)


def test_encoder_and_init_model_build_the_slot():
    from paper_accurate_fast_cheap_amd.transformer.attention import LimitedRelPositionMultiHeadedAttention
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    from paper_accurate_fast_cheap_amd.transformer import fused
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    from paper_accurate_fast_cheap_amd.transformer.cmvn import GlobalCMVN
    g = load_golden("encoder_lca")
    enc = ConformerEncoder(80, global_cmvn=GlobalCMVN(torch.zeros(80), torch.ones(80)), **g["conf"])
    assert synth.spec_of(enc.state_dict()) == g["spec"]                    # the reference encoder's names, shapes and dtypes
    assert all(isinstance(l.self_attn, LimitedRelPositionMultiHeadedAttention) for l in enc.encoders)
    assert [l.self_attn.layer_id for l in enc.encoders] == [0, 1]
    assert enc.fp32_split_operands is False and enc.embed.fp32_split_operands is False     # no bf16 slot: pure fp32
    assert not any(fused.eligible(l) for l in enc.encoders)                # the module path
    with pytest.raises(ValueError, match="att_context_size"):
        ConformerEncoder(80, **dict(g["conf"], att_context_size=[4, 2]))
    with pytest.raises(NotImplementedError, match="global_tokens"):
        ConformerEncoder(80, **dict(g["conf"], global_tokens=1))
    with pytest.raises(NotImplementedError, match="limited_rel_selfattn"):  # the text names what IS implemented
        ConformerEncoder(80, output_size=128, attention_heads=2, selfattention_layer_type="selfattn")

    configs = dict(input_dim=80, output_dim=50, encoder="conformer", encoder_conf=dict(SHIPPED_ENCODER_CONF),
                   ctc="ctc", ctc_conf=dict(ctc_blank_id=0), model="asr_model", model_conf=dict(ctc_weight=1.0))

    class Args:
        checkpoint = None
    model, _ = init_model(Args(), configs)
    slots = [l.self_attn for l in model.encoder.encoders]
    assert len(slots) == 12 and all(isinstance(s, LimitedRelPositionMultiHeadedAttention) for s in slots)
    assert slots[0].att_context_size == [256, 256] and slots[0].h == 8 and slots[0].d_k == 64
    assert model.ctc.fp32_split_operands is False


def test_install_into_adds_the_baseline_only_on_request():
    from paper_accurate_fast_cheap_amd.utils.class_utils import WENET_ATTENTION_CLASSES, install_into

    class FakeRef:
        WENET_ATTENTION_CLASSES = {"limited_rel_selfattn": object, "selfattn": object, "rwkv_tmix60": object}
    install_into(FakeRef)
    assert FakeRef.WENET_ATTENTION_CLASSES["limited_rel_selfattn"] is object          # a live process may be training
    assert FakeRef.WENET_ATTENTION_CLASSES["rwkv_tmix60"] is WENET_ATTENTION_CLASSES["rwkv_tmix60"]
    install_into(FakeRef, baseline=True)
    assert FakeRef.WENET_ATTENTION_CLASSES["limited_rel_selfattn"] is WENET_ATTENTION_CLASSES["limited_rel_selfattn"]
    assert FakeRef.WENET_ATTENTION_CLASSES["selfattn"] is object


def test_mha_band_validates_before_it_launches():
    """pafc_mha_band answers every bad argument with its PAFC_ERR_* before anything is launched: callable on a machine without a
    GPU (the library builds here with hipcc; skipped where neither hipcc nor a built library exists)."""
    import ctypes
    import os
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    L.pafc_mha_band.restype, L.pafc_mha_band.argtypes = _lib.SIGNATURES["pafc_mha_band"]      # (a private handle)
    one, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)      # non-null, 16-byte aligned, never dereferenced

    def band(dtype=0, B=1, T=5, H=2, dk=64, w=2, t_pad=8, q=one, k=one, v=one, p=one, u=one, vb=one, out=one, ldq=128, ldkv=128,
             ldp=128, ldo=128):
        return L.pafc_mha_band(dtype, B, T, H, dk, w, t_pad, q, ldq, k, v, ldkv, p, ldp, u, vb, out, ldo, NULL)

    for name in ("q", "k", "v", "p", "u", "vb", "out"):
        assert band(**{name: NULL}) == -1, name                                     # PAFC_ERR_NULL_POINTER
        assert band(**{name: ctypes.c_void_p(8)}) == -8, name                       # PAFC_ERR_ALIGNMENT
    assert band(dtype=3) == -6                                                      # PAFC_ERR_DTYPE
    assert band(B=0) == -2 and band(H=0) == -2 and band(T=0) == -2 and band(w=-1) == -2         # PAFC_ERR_BAD_DIMS
    assert band(T=9, t_pad=8) == -2                                                 # t_pad below T
    assert band(dk=32) == -7 and band(H=1, dk=128) == -7                            # PAFC_ERR_UNSUPPORTED: heads of 64 only
    for name in ("ldq", "ldkv", "ldp", "ldo"):
        assert band(**{name: 120}) == -2 and band(**{name: 130}) == -2, name        # pitch below H * dk / not 16-byte rows
        assert band(dtype=1, **{name: 132}) == -2, name                             # bf16: rows of 8 elements


def test_band_tile_remap_is_a_bijection():
    """The kernel deals the query tiles of a head to the blocks so that the blocks x, x + 8, ... get consecutive tiles
    (csrc/mha_band.hip: band_tile_of_block); restated here, every tile must be computed exactly once for every grid width."""
    def tile_of_block(bid, n):
        q, r, x, idx = n >> 3, n & 7, bid & 7, bid >> 3
        return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + idx
    for n in list(range(1, 70)) + [704, 1000, 1023]:
        assert sorted(tile_of_block(b, n) for b in range(n)) == list(range(n)), n
