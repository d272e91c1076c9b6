"""The attention decoder and its second pass, the checks that need no GPU: the framework backend of score_attention against the
float64 restatement (tests/attn_decoder_ref.py), strict loading of the upstream key list, init_model's switch, the arithmetic,
order and tie rule of the three decode modes, and the refusals."""
import math
import types

import pytest
import torch

from tests import attn_decoder_ref as REF
from tests import attn_rescore_cases as C


def _dec_sd(model):
    return {k: v for k, v in model.decoder.state_dict().items()}


@pytest.mark.parametrize("normalize_before", [True, False])
def test_framework_backend_equals_the_float64_restatement(normalize_before):
    model, hyps = C.model(normalize_before), C.hypotheses()
    enc = model.encoder.enc_out
    for rw in (0.0, 0.3):
        got = model.score_attention(enc, torch.tensor(C.LENS), hyps, rw, backend="framework")
        want_l, want_r = REF.score_attention(_dec_sd(model), C.ref_conf(normalize_before), enc, C.LENS, hyps, model.sos,
                                             model.eos, rw)
        assert [[len(t) for t in nb] for nb in got.l2r_logp] == [[len(h) + 1 for h in nb] for nb in hyps]
        err = max(abs(a - b) for a, b in zip(C.flatten(got.l2r_logp), C.flatten(want_l)))
        assert err <= 1e-10, err
        for b, nb in enumerate(hyps):
            for i in range(len(nb)):
                assert got.l2r[b][i] == pytest.approx(sum(want_l[b][i]), abs=1e-9)
        if rw > 0:
            err = max(abs(a - b) for a, b in zip(C.flatten(got.r2l_logp), C.flatten(want_r)))
            assert err <= 1e-10, err
            assert got.r2l[2][1] == pytest.approx(sum(want_r[2][1]), abs=1e-9)
        else:
            assert got.r2l is None and got.r2l_logp is None
    assert model.score_attention(enc, C.LENS, hyps, 0.3).l2r == got.l2r        # None on the CPU: the framework backend
    # the empty hypothesis scores log p(eos | sos): one term
    assert len(got.l2r_logp[0][0]) == 1 and got.l2r[0][0] == got.l2r_logp[0][0][0] < 0
    # the seeded scores separate the best two hypotheses of every utterance by more than 1e-2 (the GPU test's pick-the-same-best
    # check excludes an utterance whose gap is below ten times the measured error)
    for rw in (0.0, 0.3):
        s = model.score_attention(enc, C.LENS, hyps, rw, backend="framework").attn(rw)
        for nb in s:
            if len(nb) > 1:
                top = sorted(nb, reverse=True)
                assert top[0] - top[1] > 1e-2


def test_padding_and_batching_do_not_change_a_hypothesis_score():
    """A hypothesis scored alone equals the same hypothesis scored beside longer ones (the masks hide every padded position)."""
    model, hyps = C.model(True), C.hypotheses()
    enc = model.encoder.enc_out
    full = model.score_attention(enc, C.LENS, hyps, 0.3, backend="framework")
    alone = model.score_attention(enc[2:3], [C.LENS[2]], [[hyps[2][2]]], 0.3, backend="framework")
    assert alone.l2r[0][0] == pytest.approx(full.l2r[2][2], abs=1e-10)
    assert alone.r2l[0][0] == pytest.approx(full.r2l[2][2], abs=1e-10)


def test_multi_headed_attention_fixture_of_the_reference():
    """tests/golden/mha_decoder.pt (make_goldens_mha.py: the reference's own MultiHeadedAttention, d = 64, 4 heads, float64, a
    mask with padded keys and a pad-and-subsequent one) holds both the restatement and the product module; float64 round-off
    of sums of 64 and of at most 9 terms of magnitude ~1 stays far below 1e-12."""
    from tests.conftest import load_golden
    from paper_accurate_fast_cheap_amd.transformer.attention import MultiHeadedAttention
    gold = load_golden("mha_decoder")
    m = MultiHeadedAttention(gold["heads"], 64, 0.0).double().eval()
    m.load_state_dict(gold["state_dict"], strict=True)
    sd = {"att." + k: v for k, v in gold["state_dict"].items()}
    q, mem = gold["query"], gold["memory"]
    assert not gold["memory_mask"].all() and not gold["tgt_mask"].all()
    with torch.no_grad():
        for want, key, mask in ((gold["cross"], mem, gold["memory_mask"]), (gold["self_out"], q, gold["tgt_mask"])):
            assert (m(q, key, key, mask) - want).abs().max().item() <= 1e-12
            assert (REF.mha(sd, "att", gold["heads"], q, key, key, mask) - want).abs().max().item() <= 1e-12


def _upstream_keys(prefix, blocks):
    keys = [prefix + "embed.0.weight"]
    for n in range(blocks):
        for att in ("self_attn", "src_attn"):
            for lin in ("q", "k", "v", "out"):
                keys += [f"{prefix}decoders.{n}.{att}.linear_{lin}.weight", f"{prefix}decoders.{n}.{att}.linear_{lin}.bias"]
        for w in ("w_1", "w_2"):
            keys += [f"{prefix}decoders.{n}.feed_forward.{w}.weight", f"{prefix}decoders.{n}.feed_forward.{w}.bias"]
        for nm in ("norm1", "norm2", "norm3"):
            keys += [f"{prefix}decoders.{n}.{nm}.weight", f"{prefix}decoders.{n}.{nm}.bias"]
    return keys + [prefix + k for k in ("after_norm.weight", "after_norm.bias", "output_layer.weight", "output_layer.bias")]


def test_strict_loading_of_the_upstream_key_list():
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder, TransformerDecoder
    shapes = {"embed.0.weight": (11, 16), "output_layer.weight": (11, 16), "output_layer.bias": (11,),
              "feed_forward.w_1.weight": (24, 16), "feed_forward.w_1.bias": (24,), "feed_forward.w_2.weight": (16, 24)}

    def tensor_for(key):
        for tail, shape in shapes.items():
            if key.endswith(tail):
                return torch.randn(*shape)
        return torch.randn(16, 16) if key.endswith("weight") and "norm" not in key else torch.randn(16)

    one = TransformerDecoder(11, 16, attention_heads=2, linear_units=24, num_blocks=2)
    sd = {k: tensor_for(k) for k in _upstream_keys("", 2)}
    one.load_state_dict(sd, strict=True)
    assert sorted(one.state_dict()) == sorted(sd)
    two = BiTransformerDecoder(11, 16, attention_heads=2, linear_units=24, num_blocks=3, r_num_blocks=2)
    sd = {k: tensor_for(k) for k in _upstream_keys("left_decoder.", 3) + _upstream_keys("right_decoder.", 2)}
    two.load_state_dict(sd, strict=True)
    assert sorted(two.state_dict()) == sorted(sd)
    key = "right_decoder.decoders.1.src_attn.linear_k.weight"
    assert torch.equal(two.right_decoder.decoders[1].src_attn.linear_k.weight, sd[key])
    # constructor keys of a reference YAML's decoder_conf, and an unknown one
    BiTransformerDecoder(11, 16, attention_heads=2, linear_units=24, num_blocks=1, r_num_blocks=1, dropout_rate=0.1,
                         positional_dropout_rate=0.1, self_attention_dropout_rate=0.1, src_attention_dropout_rate=0.1,
                         some_future_key=3)


def _configs(decoder="bitransformer", transducer=False):
    enc = dict(output_size=64, attention_heads=1, linear_units=64, num_blocks=1, input_layer="conv2d", cnn_module_kernel=15,
               cnn_module_norm="layer_norm", activation_type="swish", pos_enc_layer_type="rel_pos",
               selfattention_layer_type="rwkv_tmix60_bidirectional", rnn_att_version="rwkv", rnn_att_direction="bi")
    cfg = dict(encoder="conformer", encoder_conf=enc, input_dim=80, output_dim=31, ctc="ctc", ctc_conf={"ctc_blank_id": 0},
               decoder=decoder, decoder_conf=dict(attention_heads=1, linear_units=48, num_blocks=2, r_num_blocks=1,
                                                  dropout_rate=0.1, positional_dropout_rate=0.1,
                                                  self_attention_dropout_rate=0.1, src_attention_dropout_rate=0.1),
               model_conf=dict(ctc_weight=0.3, reverse_weight=0.3), dataset_conf={})
    if decoder == "transformer":
        cfg["decoder_conf"].pop("r_num_blocks")
    if transducer:
        cfg.update(model="transducer", predictor="rnn",
                   predictor_conf=dict(embed_size=16, output_size=16, embed_dropout=0.0, hidden_size=16, num_layers=1, dropout=0.0),
                   joint="transducerjoint", joint_conf=dict(enc_output_size=64, pred_output_size=16, join_dim=16))
    return cfg


@pytest.mark.parametrize("transducer", [False, True])
def test_init_model_builds_the_decoder_only_on_request(transducer):
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder, TransformerDecoder
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    plain, _ = init_model(types.SimpleNamespace(checkpoint=None), _configs(transducer=transducer))
    assert plain.decoder is None and not plain.is_bidirectional_decoder()
    assert not any(k.startswith("decoder.") for k in plain.state_dict())
    with_dec, _ = init_model(types.SimpleNamespace(checkpoint=None, attention_decoder=True), _configs(transducer=transducer))
    assert isinstance(with_dec.decoder, BiTransformerDecoder) and with_dec.is_bidirectional_decoder()
    assert len(with_dec.decoder.left_decoder.decoders) == 2 and len(with_dec.decoder.right_decoder.decoders) == 1
    assert all(not p.requires_grad for p in with_dec.decoder.parameters())               # frozen
    extra = sorted(set(with_dec.state_dict()) - set(plain.state_dict()))
    assert extra == sorted("decoder." + k for k in _upstream_keys("left_decoder.", 2) + _upstream_keys("right_decoder.", 1))
    assert set(plain.state_dict()) <= set(with_dec.state_dict())
    one_way, _ = init_model(types.SimpleNamespace(checkpoint=None, attention_decoder=True),
                            _configs("transformer", transducer=transducer))
    assert isinstance(one_way.decoder, TransformerDecoder) and not one_way.is_bidirectional_decoder()
    with pytest.raises(NotImplementedError, match="decoder 'lstm'"):
        init_model(types.SimpleNamespace(checkpoint=None, attention_decoder=True), _configs("lstm", transducer=transducer))


# ---- the decode modes ------------------------------------------------------------------------------------------------------------
def _check_mode(first, second, l_logp, r_logp, rw, wc, wa=1.0, td=None, wt=0.0):
    for b, (r1, r2) in enumerate(zip(first, second)):
        final, attn, order, conf, tcs = REF.rescore(r1.nbest_scores, l_logp[b], None if r_logp is None else r_logp[b], rw, wc, wa,
                                                    None if td is None else td[b], wt)
        assert r2.nbest == [r1.nbest[i] for i in order]
        assert r2.nbest_scores == pytest.approx([final[i] for i in order], rel=1e-12)
        assert r2.nbest_attn_scores == pytest.approx([attn[i] for i in order], rel=1e-12)
        assert all(x >= y for x, y in zip(r2.nbest_scores, r2.nbest_scores[1:]))
        assert r2.tokens == r2.nbest[0] and r2.score == r2.nbest_scores[0]
        assert r2.confidence == pytest.approx(conf[order[0]], rel=1e-12)
        assert r2.tokens_confidence == pytest.approx(tcs[order[0]], rel=1e-12) and len(r2.tokens_confidence) == len(r2.tokens)
        if td is None:
            assert r2.nbest_td_scores is None
        else:
            assert r2.nbest_td_scores == pytest.approx([td[b][i] for i in order], rel=1e-12)
        if r1.nbest_times is not None:
            assert r2.nbest_times == [r1.nbest_times[i] for i in order] and r2.times == r2.nbest_times[0]
        else:
            assert r2.nbest_times is None and r2.times is None


def test_attention_rescoring_on_the_asr_model():
    model = C.model(True)
    speech, lens = torch.zeros(3, 70, 2, dtype=torch.float64), torch.tensor(C.LENS)
    enc = model.encoder.enc_out
    for rw, wc in ((0.0, 0.5), (0.3, 0.7)):
        out = model.decode(["ctc_prefix_beam_search", "attention_rescoring"], speech, lens, beam_size=4, ctc_weight=wc,
                           reverse_weight=rw)
        first, second = out["ctc_prefix_beam_search"], out["attention_rescoring"]
        assert any(len(r.nbest) > 1 for r in first)
        sc = model.score_attention(enc, lens, [r.nbest for r in first], rw)
        _check_mode(first, second, sc.l2r_logp, sc.r2l_logp, rw, wc)
        assert all(r.nbest_times is not None for r in second)
    alone = model.decode(["attention_rescoring"], speech, lens, beam_size=4, ctc_weight=0.7, reverse_weight=0.3)
    assert list(alone) == ["attention_rescoring"]                                  # the first pass is not reported unasked
    assert [r.nbest for r in alone["attention_rescoring"]] == [r.nbest for r in second]


def _transducer(seed=3):
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder
    torch.manual_seed(seed)
    vocab, dim = 8, 6
    enc_out = torch.randn(3, 6, dim) * 1.5
    dec = BiTransformerDecoder(vocab, dim, attention_heads=2, linear_units=10, num_blocks=1, r_num_blocks=1)
    model = Transducer(vocab, 0, C.FixedEncoder(enc_out), RNNPredictor(vocab, 4, 7, 0.0, 7, 1, dropout=0.0),
                       TransducerJoint(vocab, dim, 7, 5), ctc=CTC(vocab, dim), attention_decoder=dec).eval()
    return model.to(torch.float64), torch.zeros(3, 6, 2, dtype=torch.float64), torch.tensor([6, 4, 1])


def test_transducer_attention_modes():
    model, speech, lens = _transducer()
    enc = model.encoder.enc_out
    assert model.is_bidirectional_decoder()
    rw, wa, wc, wt = 0.3, 0.6, 0.4, 1.3
    out = model.decode(["ctc_prefix_beam_search", "attention_rescoring", "ctc_beam_td_attn_rescoring", "ctc_beam_td_rescoring"],
                       speech, lens, beam_size=4, ctc_weight=wc, transducer_weight=wt)
    assert sorted(out) == sorted(["ctc_prefix_beam_search", "attention_rescoring", "ctc_beam_td_attn_rescoring",
                                  "ctc_beam_td_rescoring"])
    out = model.decode(["ctc_prefix_beam_search", "attention_rescoring", "ctc_beam_td_attn_rescoring"], speech, lens, beam_size=4,
                       ctc_weight=wc, transducer_weight=wt, attn_weight=wa, reverse_weight=rw)
    first = out["ctc_prefix_beam_search"]
    assert any(len(r.nbest) > 1 for r in first)
    hyps = [r.nbest for r in first]
    sc = model.score_attention(enc, lens, hyps, rw)
    td = model.score_hypotheses(enc, lens, hyps)
    _check_mode(first, out["attention_rescoring"], sc.l2r_logp, sc.r2l_logp, rw, wc)
    _check_mode(first, out["ctc_beam_td_attn_rescoring"], sc.l2r_logp, sc.r2l_logp, rw, wc, wa, td, wt)
    # the rnnt first pass: beam_search_decode with the search weights
    first = model.decode(["rnnt_beam_search"], speech, lens, beam_size=4, ctc_weight=0.3, transducer_weight=0.7)["rnnt_beam_search"]
    second = model.decode(["rnnt_beam_attn_rescoring"], speech, lens, beam_size=4, ctc_weight=wc, transducer_weight=wt,
                          attn_weight=wa, reverse_weight=rw)["rnnt_beam_attn_rescoring"]
    hyps = [r.nbest for r in first]
    sc = model.score_attention(enc, lens, hyps, rw)
    _check_mode(first, second, sc.l2r_logp, sc.r2l_logp, rw, wc, wa, model.score_hypotheses(enc, lens, hyps), wt)
    # weights (attn, ctc, td) = (0, 1, 0): the first pass's order and scores
    for mode, ref_mode, kw in (("ctc_beam_td_attn_rescoring", "ctc_prefix_beam_search", {}),
                               ("rnnt_beam_attn_rescoring", "rnnt_beam_search",
                                dict(search_ctc_weight=0.9, search_transducer_weight=0.1))):
        base = model.decode([ref_mode], speech, lens, beam_size=4, ctc_weight=0.9, transducer_weight=0.1)[ref_mode]
        same = model.decode([mode], speech, lens, beam_size=4, ctc_weight=1.0, transducer_weight=0.0, attn_weight=0.0,
                            reverse_weight=rw, **kw)[mode]
        for r1, r2 in zip(base, same):
            assert r2.nbest == r1.nbest and r2.nbest_scores == r1.nbest_scores


def test_ties_go_to_the_earlier_first_pass_rank():
    from paper_accurate_fast_cheap_amd.transformer.attn_rescore import AttentionScores, attention_rescore
    from paper_accurate_fast_cheap_amd.transformer.search import DecodeResult
    first = DecodeResult(tokens=[1], score=-1.0, times=[0], nbest=[[1], [2], [3], [4]], nbest_scores=[-1.0, -2.0, -3.0, -4.0],
                         nbest_times=[[0], [1], [2], [3]])
    lp = [[[-3.0, -1.0], [-1.5, -0.5], [-0.5, -0.5], [-0.25, -0.75]]]              # l2r: -4, -2, -1, -1 -> final -5, -4, -4, -5
    sc = AttentionScores([[sum(t) for t in lp[0]]], lp)
    out = attention_rescore([first], sc, 0.0, 1.0)[0]
    assert out.nbest == [[2], [3], [1], [4]] and out.nbest_scores == [-4.0, -4.0, -5.0, -5.0]
    assert out.nbest_times == [[1], [2], [0], [3]] and out.times == [1] and out.tokens == [2] and out.score == -4.0
    assert out.nbest_attn_scores == [-2.0, -1.0, -4.0, -1.0] and out.nbest_td_scores is None
    assert out.confidence == math.exp(-2.0 / 2) and out.tokens_confidence == [math.exp(-1.5)]
    assert DecodeResult([1]).nbest_attn_scores is None                             # existing constructions are unaffected
    none = DecodeResult(tokens=[], score=0.0, nbest=[], nbest_scores=[])
    empty = attention_rescore([none], AttentionScores([[]], [[]]), 0.0, 1.0)[0]
    assert empty.nbest == [] and empty.tokens == [] and empty.nbest_attn_scores == []


def test_refusals():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    hyps = C.hypotheses()
    one_way = C.model(True, bidirectional=False)
    enc = one_way.encoder.enc_out
    assert not one_way.is_bidirectional_decoder()
    one_way.score_attention(enc, C.LENS, hyps, 0.0)
    with pytest.raises(ValueError, match="needs the right_decoder"):
        one_way.score_attention(enc, C.LENS, hyps, 0.3)
    model = C.model(True)
    with pytest.raises(PafcError, match="not on the GPU"):                         # never a fallback
        model.score_attention(enc, C.LENS, hyps, 0.0, backend="kernels")
    with pytest.raises(ValueError, match="backend must be one of"):
        model.score_attention(enc, C.LENS, hyps, 0.0, backend="eager")
    with pytest.raises(ValueError, match=r"utterance 1, hypothesis 0: token 53 outside the vocabulary"):
        model.score_attention(enc, C.LENS, [[[1]], [[C.V]], []], 0.0)
    with pytest.raises(ValueError, match="3 utterances, 2 n-best lists"):
        model.score_attention(enc, C.LENS, hyps[:2], 0.0)
    assert model.score_attention(enc, C.LENS, [[], [], []], 0.3).l2r == [[], [], []]
    long = model.score_attention(enc, C.LENS, [[], [[3] * 2600], []], 0.0)            # no length limit of another kernel's
    assert len(long.l2r_logp[1][0]) == 2601 and long.stats is None
    with pytest.raises(ValueError, match=r"utterance 2, hypothesis 1: token -1 outside"):
        model.score_attention(enc, C.LENS, [[], [], [[1], [2, -1]]], 0.0)
    # no decoder: the three modes and score_attention are NotImplementedError; "attention" stays one
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    bare = ASRModel(C.V, C.FixedEncoder(enc), CTC(C.V, C.D)).eval().double()
    speech, lens = torch.zeros(3, 70, 2, dtype=torch.float64), torch.tensor(C.LENS)
    assert bare.decoder is None and not bare.is_bidirectional_decoder()
    with pytest.raises(NotImplementedError, match="attention decoder"):
        bare.decode(["attention_rescoring"], speech, lens)
    with pytest.raises(NotImplementedError):
        bare.score_attention(enc, C.LENS, hyps)
    with pytest.raises(NotImplementedError):
        model.decode(["attention"], speech, lens)
    # the transducer-only modes still refuse an attention weight, and say where the attention term lives
    tmodel, tspeech, tlens = _transducer()
    for mode in ("ctc_beam_td_rescoring", "rnnt_beam_td_rescoring"):
        with pytest.raises(ValueError, match="attention decoder was not released.*ctc_beam_td_attn_rescoring"):
            tmodel.decode([mode], tspeech, tlens, beam_size=4, attn_weight=0.5)
    tmodel.decoder = None
    for mode in ("attention_rescoring", "ctc_beam_td_attn_rescoring", "rnnt_beam_attn_rescoring"):
        with pytest.raises(NotImplementedError, match="needs an attention decoder"):
            tmodel.decode([mode], tspeech, tlens, beam_size=4)


def test_attention_kernels_validate_before_they_launch():
    """pafc_mha_rows / pafc_logp_gather_rows answer bad arguments with a PAFC_ERR_* before anything is launched: callable on a
    machine without a GPU (the library builds here with hipcc; skipped where neither hipcc nor a built library exists)."""
    import ctypes
    import os
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    for name in ("pafc_mha_rows", "pafc_logp_gather_rows"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]   # (a private handle, not the package's)
    one, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)      # non-null, 16-byte aligned, never dereferenced

    def mha(dtype=0, G=1, H=2, dk=64, q=one, ld=128):
        return L.pafc_mha_rows(dtype, G, H, dk, q, ld, one, one, ld, one, one, one, 1, one, ld, NULL)

    assert mha(q=NULL) == -1 and mha(dtype=3) == -6 and mha(G=0) == -2 and mha(H=0) == -2
    assert mha(dk=32) == -7 and mha(H=1, dk=128) == -7                              # PAFC_ERR_UNSUPPORTED: heads of 64 only
    assert mha(ld=120) == -2 and mha(ld=130) == -2 and mha(dtype=1, ld=132) == -2   # pitch below H * dk / not 16-byte rows
    assert mha(q=ctypes.c_void_p(8)) == -8
    assert L.pafc_logp_gather_rows(0, 4, 5, NULL, 5, one, one, NULL) == -1
    assert L.pafc_logp_gather_rows(0, 0, 5, one, 5, one, one, NULL) == -2
    assert L.pafc_logp_gather_rows(0, 4, 5, one, 4, one, one, NULL) == -2           # pitch below V
    assert L.pafc_logp_gather_rows(7, 4, 5, one, 5, one, one, NULL) == -6


def test_logits_chunks_cover_every_row_under_the_cap():
    from paper_accurate_fast_cheap_amd.transformer.attn_rescore import _logits_chunks
    for ends, cap in (([5, 9, 30], 10), ([5, 9, 30], 4), ([3], 100), ([40, 41, 42], 1), ([2, 4, 6, 8], 4), ([7, 7, 12], 5)):
        chunks = _logits_chunks(ends, cap)
        assert chunks[0][0] == 0 and chunks[-1][1] == ends[-1]
        assert all(a1 == e0 for (_, e0), (a1, _) in zip(chunks, chunks[1:]))       # contiguous
        assert all(0 < e - a <= cap for a, e in chunks)
    assert _logits_chunks([5, 9, 30], 10) == [(0, 9), (9, 19), (19, 29), (29, 30)]
