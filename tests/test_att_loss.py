"""The attention term of the training objective on the CPU: the host functions against what the reference's own functions
returned (tests/golden/att_loss_host.pt, written by tests/golden/make_goldens_att_loss.py), the framework backend of
transformer/attn_train.att_loss in float64 against the restatement of tests/att_loss_ref.py, the two containers' forward,
init_model's switches, and the argument checks of the new entry points of include/pafc_attention.h."""
import types

import pytest
import torch

from tests import att_loss_ref as REF
from tests import attn_rescore_cases as C
from tests.conftest import load_golden


def test_host_functions_reproduce_the_reference_outputs():
    from paper_accurate_fast_cheap_amd.transformer.label_smoothing_loss import LabelSmoothingLoss
    from paper_accurate_fast_cheap_amd.utils.common import IGNORE_ID, add_sos_eos, reverse_pad_list, th_accuracy
    g = load_golden("att_loss_host")
    assert IGNORE_ID == g["ignore"] == -1
    assert (g["lens"] == 0).any()                                                    # the batch has an empty transcript
    ys_in, ys_out = add_sos_eos(g["text"], g["sos"], g["eos"], g["ignore"])
    assert torch.equal(ys_in, g["ys_in"]) and torch.equal(ys_out, g["ys_out"]) and ys_in.dtype == g["ys_in"].dtype
    r_text = reverse_pad_list(g["text"], g["lens"], float(g["ignore"]))
    assert torch.equal(r_text, g["r_text"]) and r_text.dtype == g["r_text"].dtype
    r_in, r_out = add_sos_eos(r_text, g["sos"], g["eos"], g["ignore"])
    assert torch.equal(r_in, g["r_ys_in"]) and torch.equal(r_out, g["r_ys_out"]) and r_in.dtype == g["r_ys_in"].dtype
    acc = th_accuracy(g["logits"].view(-1, g["V"]), ys_out, g["ignore"])
    assert 0 < g["acc"] < 1 and torch.equal(acc, g["acc"])
    for smoothing in (0.0, 0.1):
        for norm in (False, True):
            crit = LabelSmoothingLoss(g["V"], g["ignore"], smoothing, norm)
            for key, tgt in (((smoothing, norm), ys_out), ((smoothing, norm, "r"), r_out)):
                got, want = crit(g["logits"], tgt), g["losses"][key]
                assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item()), (key, got.item(), want.item())
            # ... and the restatement the other tests lean on says the same
            rows = REF.lsm_rows(g["logits"].view(-1, g["V"]), ys_out.view(-1), smoothing)["loss"].sum()
            denom = int((ys_out != -1).sum()) if norm else ys_out.size(0)
            assert abs((rows / denom).item() - g["losses"][(smoothing, norm)].item()) <= 1e-12 * abs(rows.item())


TEXT_LENS = [0, 1, 16, 17]
MEM_LENS = [1, 17, 40, 40]


def _batch(dtype=torch.float64, d=C.D, seed=31):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(4, 40, d, generator=g, dtype=torch.float64).to(dtype)
    texts = [[int(v) for v in torch.randint(1, C.V - 1, (n,), generator=g)] for n in TEXT_LENS]
    text = torch.full((4, max(TEXT_LENS)), -1, dtype=torch.int64)
    for b, t in enumerate(texts):
        text[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
    mask = (torch.arange(40)[None, :] < torch.tensor(MEM_LENS)[:, None]).unsqueeze(1)
    return enc, mask, texts, text, torch.tensor(TEXT_LENS)


@pytest.mark.parametrize("reverse_weight", [0.0, 0.3])
@pytest.mark.parametrize("normalize_before", [True, False])
def test_framework_backend_equals_the_float64_restatement(normalize_before, reverse_weight):
    from paper_accurate_fast_cheap_amd.transformer.attn_train import att_loss
    enc, mask, texts, text, lens = _batch()
    for length_normalized in (False, True):
        model = C.model(normalize_before, enc_out=enc)
        model.reverse_weight, model.lsm_weight, model.length_normalized_loss = reverse_weight, 0.1, length_normalized
        x = enc.clone().requires_grad_(True)
        loss, acc = att_loss(model, x, mask, text, lens, backend="framework")
        loss.backward()
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.decoder.state_dict().items()}
        xr = enc.clone().requires_grad_(True)
        want, want_acc = REF.att_loss(sd, C.ref_conf(normalize_before), xr, MEM_LENS, texts, model.sos, model.eos, reverse_weight,
                                      0.1, length_normalized)
        want.backward()
        assert abs(loss.item() - want.item()) <= 1e-10, (loss.item(), want.item())
        assert abs(acc.item() - want_acc) <= 1e-12
        assert (x.grad - xr.grad).abs().max().item() <= 1e-10
        assert (x.grad[0, 1:] == 0).all() and x.grad[1, :17].abs().max() > 0              # padded memory rows get nothing
        params = dict(model.decoder.named_parameters())
        assert set(params) == set(sd)
        for name, p in params.items():
            unused = (reverse_weight == 0 and name.startswith("right_decoder.")) or (not normalize_before and "after_norm" in name)
            if unused:                                       # the right decoder at weight 0; post-norm has no final norm
                assert p.grad is None and sd[name].grad is None, name
                continue
            assert p.grad is not None and (p.grad - sd[name].grad).abs().max().item() <= 1e-10, name


def _asr_model(decoder: str, ctc_weight=0.3):
    """float32 ASRModel over a fixed encoder output: decoder 'none' | 'frozen' | 'trainable'."""
    enc, mask, texts, text, lens = _batch(torch.float32)
    m = C.model(True, dtype=torch.float32, enc_out=enc)
    m.ctc_weight, m.reverse_weight, m.lsm_weight = ctc_weight, 0.3, 0.1
    if decoder == "none":
        m.decoder = None
    elif decoder == "frozen":
        m.decoder.requires_grad_(False)
    batch = dict(feats=torch.zeros(4, 40, 2), feats_lengths=torch.tensor(MEM_LENS), target=text, target_lengths=lens)
    return m, batch


def test_asr_model_forward_adds_the_attention_term():
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.attn_train import att_loss
    bare = ASRModel(5, torch.nn.Identity(), None)
    assert (bare.reverse_weight, bare.lsm_weight, bare.length_normalized_loss) == (0.0, 0.0, False)     # the reference's defaults
    cpu = torch.device("cpu")
    plain, batch = _asr_model("none")
    frozen, _ = _asr_model("frozen")
    out_plain, out_frozen = plain(batch, cpu), frozen(batch, cpu)
    assert set(out_plain) == set(out_frozen) == {"loss", "loss_ctc"}                  # exactly what they returned before
    assert torch.equal(out_plain["loss"], out_frozen["loss"]) and out_plain["loss"] is out_plain["loss_ctc"]
    model, _ = _asr_model("trainable")
    out = model(batch, cpu)
    assert set(out) == {"loss", "loss_att", "loss_ctc", "th_accuracy"}
    assert torch.equal(out["loss_ctc"], out_plain["loss_ctc"])
    enc_out, mask = model.encoder(batch["feats"], batch["feats_lengths"])
    want_att, want_acc = att_loss(model, enc_out, mask, batch["target"], batch["target_lengths"], backend="framework")
    assert torch.equal(out["loss_att"], want_att) and torch.equal(out["th_accuracy"], want_acc)
    assert torch.allclose(out["loss"], 0.3 * out["loss_ctc"] + 0.7 * out["loss_att"], rtol=1e-6)
    out["loss"].backward()
    assert model.decoder.left_decoder.embed[0].weight.grad.abs().max() > 0
    assert model.decoder.right_decoder.output_layer.weight.grad.abs().max() > 0
    only_ctc, _ = _asr_model("trainable", ctc_weight=1.0)                             # asr_model.py:188: no attention term at weight 1
    assert set(only_ctc(batch, cpu)) == {"loss", "loss_ctc"}
    with pytest.raises(ValueError, match="right_decoder"):
        one_way = C.model(True, dtype=torch.float32, bidirectional=False, enc_out=enc_out)
        one_way.reverse_weight = 0.3
        att_loss(one_way, enc_out, mask, batch["target"], batch["target_lengths"])
    with pytest.raises(NotImplementedError):
        att_loss(plain, enc_out, mask, batch["target"], batch["target_lengths"])


def _transducer(decoder: str, **weights):
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder
    torch.manual_seed(3)
    vocab, dim = 8, 6
    enc_out = torch.randn(3, 6, dim) * 1.5
    dec = None if decoder == "none" else BiTransformerDecoder(vocab, dim, attention_heads=2, linear_units=10, num_blocks=1,
                                                              r_num_blocks=1, dropout_rate=0.0, positional_dropout_rate=0.0)
    if decoder == "frozen":
        dec.requires_grad_(False)
    torch.manual_seed(4)
    model = Transducer(vocab, 0, C.FixedEncoder(enc_out), RNNPredictor(vocab, 4, 7, 0.0, 7, 1, dropout=0.0),
                       TransducerJoint(vocab, dim, 7, 5), ctc=CTC(vocab, dim), attention_decoder=dec, **weights)
    text = torch.tensor([[1, 2, 3], [4, -1, -1], [-1, -1, -1]])
    batch = dict(feats=torch.zeros(3, 6, 2), feats_lengths=torch.tensor([6, 4, 1]), target=text,
                 target_lengths=torch.tensor([3, 1, 0]))
    return model, batch


def test_transducer_forward_adds_the_attention_term():
    from paper_accurate_fast_cheap_amd.transformer.attn_train import att_loss
    w = dict(transducer_weight=0.3, ctc_weight=0.2, attention_weight=0.5, reverse_weight=0.3, lsm_weight=0.1)    # the YAMLs' weights
    cpu = torch.device("cpu")
    plain, batch = _transducer("none", **w)
    frozen, _ = _transducer("frozen", **w)
    out_plain, out_frozen = plain(batch, cpu), frozen(batch, cpu)
    keys = {"loss", "loss_att", "loss_ctc", "loss_rnnt", "th_accuracy"}
    for out in (out_plain, out_frozen):
        assert set(out) == keys and out["loss_att"] is None and out["th_accuracy"] == -1.0
    assert torch.equal(out_plain["loss"], out_frozen["loss"])
    model, _ = _transducer("trainable", **w)
    assert (model.reverse_weight, model.lsm_weight, model.length_normalized_loss) == (0.3, 0.1, False)
    out = model(batch, cpu)
    assert set(out) == keys and torch.equal(out["loss_rnnt"], out_plain["loss_rnnt"])
    enc_out, mask = model.encoder(batch["feats"], batch["feats_lengths"])
    want_att, want_acc = att_loss(model, enc_out, mask, batch["target"], batch["target_lengths"], backend="framework")
    assert torch.equal(out["loss_att"], want_att) and torch.equal(out["th_accuracy"], want_acc)
    assert torch.isfinite(out["loss_att"]) and out["loss_att"] > 0
    assert torch.allclose(out["loss"], 0.3 * out["loss_rnnt"] + 0.2 * out["loss_ctc"].sum() + 0.5 * out["loss_att"], rtol=1e-6)
    zero, _ = _transducer("trainable", **dict(w, attention_weight=0.0))
    assert zero(batch, cpu)["loss_att"] is None


def test_init_model_switches():
    from tests.test_attn_rescore import _configs
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    for transducer in (False, True):
        frozen, _ = init_model(types.SimpleNamespace(checkpoint=None, attention_decoder=True), _configs(transducer=transducer))
        assert all(not p.requires_grad for p in frozen.decoder.parameters())
        train, _ = init_model(types.SimpleNamespace(checkpoint=None, train_attention_decoder=True), _configs(transducer=transducer))
        assert all(p.requires_grad for p in train.decoder.parameters())                   # reverse_weight 0.3: both directions
        assert train.reverse_weight == 0.3 and train.lsm_weight == 0.0 and train.length_normalized_loss is False
        cfg = _configs(transducer=transducer)
        cfg["model_conf"].update(reverse_weight=0.0, lsm_weight=0.1, length_normalized_loss=True)
        left_only, _ = init_model(types.SimpleNamespace(checkpoint=None, train_attention_decoder=True), cfg)
        assert all(p.requires_grad for p in left_only.decoder.left_decoder.parameters())
        assert all(not p.requires_grad for p in left_only.decoder.right_decoder.parameters())
        assert left_only.lsm_weight == 0.1 and left_only.length_normalized_loss is True
        neither, _ = init_model(types.SimpleNamespace(checkpoint=None), _configs(transducer=transducer))
        assert neither.decoder is None


def test_kernels_backend_is_never_a_fallback():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer.attn_train import att_loss, att_loss_unmet
    model, batch = _asr_model("trainable")
    enc_out, mask = model.encoder(batch["feats"], batch["feats_lengths"])
    assert att_loss_unmet(model, enc_out) == "the operands are not on the GPU"
    with pytest.raises(PafcError, match="not on the GPU"):
        att_loss(model, enc_out, mask, batch["target"], batch["target_lengths"], backend="kernels")
    with pytest.raises(ValueError, match="backend"):
        att_loss(model, enc_out, mask, batch["target"], batch["target_lengths"], backend="triton")
    loss, _ = att_loss(model, enc_out, mask, batch["target"], batch["target_lengths"])          # None: the framework backend here
    assert torch.isfinite(loss)


def check_bad_arguments(L):
    """Every new entry point of include/pafc_attention.h answers bad arguments with a PAFC_ERR_* before any launch.  L: a
    library handle whose signatures are set; the addresses are never dereferenced, so this runs without a GPU."""
    import ctypes
    one, NULL, odd = ctypes.c_void_p(16), ctypes.c_void_p(0), ctypes.c_void_p(8)

    def lse(dtype=0, G=1, H=2, dk=64, q=one, ld=128, stats=one):
        return L.pafc_mha_rows_lse(dtype, G, H, dk, q, ld, one, one, ld, one, one, one, 1, one, ld, stats, NULL)

    assert lse(q=NULL) == -1 and lse(stats=NULL) == -1 and lse(dtype=3) == -6 and lse(G=0) == -2
    assert lse(dk=32) == -7 and lse(ld=120) == -2 and lse(ld=130) == -2 and lse(q=odd) == -8

    def bwd(dtype=0, G=1, H=2, dk=64, rows=4, q=one, ld=128, lddo=128, lddkv=128, stats=one, dq=one, ws=one, nbytes=1 << 20):
        return L.pafc_mha_rows_bwd(dtype, G, H, dk, rows, q, ld, one, one, ld, one, ld, one, lddo, stats, one, one, one, 0, dq, ld,
                                   one, one, lddkv, ws, nbytes, NULL)

    assert bwd(q=NULL) == -1 and bwd(stats=NULL) == -1 and bwd(dq=NULL) == -1 and bwd(ws=NULL) == -1
    assert bwd(dtype=2) == -6 and bwd(G=0) == -2 and bwd(H=0) == -2 and bwd(rows=0) == -2
    assert bwd(dk=32) == -7 and bwd(H=1, dk=128) == -7                              # PAFC_ERR_UNSUPPORTED: heads of 64 only
    assert bwd(ld=120) == -2 and bwd(lddo=130) == -2 and bwd(dtype=1, lddkv=132) == -2   # pitch below H * dk / not 16-byte rows
    assert bwd(q=odd) == -8 and bwd(dq=odd) == -8
    assert bwd(nbytes=4 * 2 * 4 - 1) == -4                                           # PAFC_ERR_WORKSPACE
    assert L.pafc_mha_rows_bwd_workspace_bytes(160, 8) == 160 * 8 * 4 and L.pafc_mha_rows_bwd_workspace_bytes(0, 8) == 0

    def loss(dtype=0, rows=4, V=5, x=one, ldl=5, smoothing=0.1, out=one):
        return L.pafc_lsm_loss_rows(dtype, rows, V, x, ldl, one, smoothing, out, one, one, NULL)

    assert loss(x=NULL) == -1 and loss(out=NULL) == -1 and loss(dtype=7) == -6
    assert loss(rows=0) == -2 and loss(ldl=4) == -2 and loss(V=1, ldl=1) == -2 and loss(smoothing=1.5) == -2

    def lbwd(dtype=0, rows=4, V=5, x=one, ldl=5, smoothing=0.1, g=one, dx=ctypes.c_void_p(32), ldd=8):
        return L.pafc_lsm_loss_rows_bwd(dtype, rows, V, x, ldl, one, smoothing, one, g, dx, ldd, NULL)

    assert lbwd(x=NULL) == -1 and lbwd(g=NULL) == -1 and lbwd(dx=NULL) == -1 and lbwd(dtype=7) == -6
    assert lbwd(rows=0) == -2 and lbwd(ldl=4) == -2 and lbwd(ldd=4) == -2 and lbwd(smoothing=-0.1) == -2
    assert lbwd(dx=one, ldd=8) == -2                                                 # in place needs the logits' own pitch


def test_new_entry_points_validate_before_they_launch():
    """Callable on a machine without a GPU (the library builds here with hipcc; skipped where neither hipcc nor a built
    library exists)."""
    import ctypes
    import os
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    for name in ("pafc_mha_rows_lse", "pafc_mha_rows_bwd", "pafc_mha_rows_bwd_workspace_bytes", "pafc_lsm_loss_rows",
                 "pafc_lsm_loss_rows_bwd"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]   # (a private handle, not the package's)
    check_bad_arguments(L)
