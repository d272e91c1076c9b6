"""The full-sum transducer score of n-best lists on the MI355X (csrc/rnnt_loss.hip: pafc_rnnt_score through
hip_ops.rnnt_score_hypotheses, Transducer.score_hypotheses(backend="kernels") and the two rescoring decode modes).

The rows of the scorer go through the join, stats and lse kernels of the training forward and its lattice repeats that forward's
fp32 recurrence, so a hypothesis scored over the shared prefix trie must have the BITS of -rnnt_joint_loss fed that hypothesis
alone (its utterance's encoder rows, its own predictor rows, its labels).  The predictor rows of a test are a function of the
prefix, as a predictor's are: hypotheses that share a prefix hold equal rows there."""
import warnings

import pytest
import torch

from tests import parity_log
from tests.test_rnnt_joint_loss_gpu import _brute, _inputs, _restated_fp64
from tests.test_rnnt_rescore import _check_second_pass, _FixedEncoder

pytestmark = pytest.mark.gpu


def _labels(n, V, blank, g):
    lab = torch.randint(0, V - 1, (n,), generator=g)
    return (lab + (lab >= blank).to(torch.int64)).tolist()            # never the blank (the convention of _targets)


def _patterned(V, blank, seed, umax=6):
    """Five hypotheses of up to umax tokens: a long one, a strict prefix of it, one that leaves it in the middle, one that
    diverges at the root, a duplicate."""
    g = torch.Generator().manual_seed(seed)
    a = _labels(umax, V, blank, g)
    other = _labels(umax, V, blank, g)
    mid = a[:2] + [t for t in other[2:4]]
    if mid[2] == a[2]:
        mid[2] = a[2] + 1 if a[2] + 1 not in (blank, V) else a[2] - 1
    root = [other[0] if other[0] != a[0] else (a[0] + 1 if a[0] + 1 not in (blank, V) else a[0] - 1)] + a[1:2]
    return [a, a[:3], mid, root, list(a)]


def _pred_rows(hyps, J, seed):
    """(N, Umax + 1, J) bf16: row (n, u) depends on the prefix h_n[:u] alone; rows beyond U_n hold other values (never read)."""
    g = torch.Generator().manual_seed(seed)
    flat = [h for nbest in hyps for h in nbest]
    up1 = max(len(h) for h in flat) + 1
    P = (torch.randn(len(flat), up1, J, generator=g) * 0.6).to(torch.bfloat16)
    seen = {}
    for n, h in enumerate(flat):
        for u in range(len(h) + 1):
            key = tuple(h[:u])
            if key in seen:
                P[n, u] = seen[key]
            else:
                seen[key] = P[n, u].clone()
    return P.cuda()


def _ys(flat):
    ys = torch.zeros(len(flat), max(max(len(h) for h in flat), 1), dtype=torch.int64)
    for n, h in enumerate(flat):
        ys[n, :len(h)] = torch.tensor(h, dtype=torch.int64)
    return ys


def _score(E, P, W, b, lens, hyps, blank, device_lens=True, **kw):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transducer.search.rescoring import build_arc_tables
    tb = build_arc_tables(hyps, lens, W.shape[0], blank, pred_stride=P.shape[1], share=kw.pop("share", True))
    hl = torch.tensor(lens, device="cuda") if device_lens else None
    return hip_ops.rnnt_score_hypotheses(E.float(), P.float(), W.float(), b.float(), hl, tb, blank, **kw), tb


def _training_forward(E, P, W, b, lens, hyps, blank):
    """-nll of hip_ops.rnnt_joint_loss on the repeated operands: one 'utterance' per hypothesis."""
    from paper_accurate_fast_cheap_amd import hip_ops
    utt_of = [bi for bi, nbest in enumerate(hyps) for _ in nbest]
    flat = [h for nbest in hyps for h in nbest]
    with torch.no_grad():
        nll = hip_ops.rnnt_joint_loss(E[utt_of].float(), P.float(), W.float(), b.float(),
                                      torch.tensor([lens[bi] for bi in utt_of], device="cuda"), _ys(flat).cuda(),
                                      torch.tensor([len(h) for h in flat], device="cuda"), blank)
    return -nll


@pytest.mark.parametrize("blank", [0, 7])
@pytest.mark.parametrize("V", [40, 264])                   # one column tile; three, the last partial
def test_bitwise_equal_to_the_training_forward(hip, V, blank):
    J, T, lens = 64, 12, [12, 5, 1]
    g = torch.Generator().manual_seed(V + blank)
    hyps = [_patterned(V, blank, seed=V + blank), [[], _labels(1, V, blank, g)], [_labels(3, V, blank, g)]]   # U = 3 > T = 1
    E, _, W, b = _inputs(3, T, 1, J, V, seed=31 + blank)
    P = _pred_rows(hyps, J, seed=5)
    score, tb = _score(E, P, W, b, lens, hyps, blank)
    assert tb.rows < tb.rows_repeated
    want = _training_forward(E, P, W, b, lens, hyps, blank)
    assert torch.isfinite(score).all()
    assert torch.equal(score, want), (score.tolist(), want.tolist())
    again, _ = _score(E, P, W, b, lens, hyps, blank)
    assert torch.equal(score, again)                       # two calls: the same bits
    assert score[0] == score[4]                            # the duplicate


def test_bitwise_over_several_row_tiles(hip):
    """T = 40 and 14 arcs: 560 rows, four full 128-row tiles and a partial one."""
    J, V, blank, T = 64, 264, 0, 40
    hyps = [[[10, 20, 30, 40, 50], [10, 20, 30], [10, 20, 31, 41], [11, 20], [10, 20, 30, 40, 50], [12], []]]   # 10 edges + 4 leaves
    E, _, W, b = _inputs(1, T, 1, J, V, seed=17)
    P = _pred_rows(hyps, J, seed=6)
    score, tb = _score(E, P, W, b, [T], hyps, blank)
    assert tb.arcs(0) == 14 and tb.rows == 560 and tb.rows % 128 != 0
    assert torch.equal(score, _training_forward(E, P, W, b, [T], hyps, blank))


def test_sharing_and_grouping_change_nothing(hip):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    J, V, blank, T, lens = 64, 264, 7, 12, [12, 5, 9]
    g = torch.Generator().manual_seed(2)
    hyps = [_patterned(V, blank, seed=3), [[], _labels(1, V, blank, g)], _patterned(V, blank, seed=4, umax=4)]
    E, _, W, b = _inputs(3, T, 1, J, V, seed=23)
    P = _pred_rows(hyps, J, seed=7)
    together, tb = _score(E, P, W, b, lens, hyps, blank)
    n = 0
    for bi, nbest in enumerate(hyps):                      # each hypothesis scored alone: N = 1 calls
        for h in nbest:
            alone, _ = _score(E[bi:bi + 1], P[n:n + 1], W, b, lens[bi:bi + 1], [[h]], blank)
            assert torch.equal(alone[0], together[n]), (bi, h)
            n += 1
    grouped, _ = _score(E, P, W, b, lens, hyps, blank, max_rows=max(tb.utt_rows))     # every utterance its own group
    assert max(tb.utt_rows) < tb.rows and torch.equal(grouped, together)
    unshared, tu = _score(E, P, W, b, lens, hyps, blank, share=False)                 # every hypothesis its own utterance
    assert tu.nutt == tb.nhyp and tu.rows == tb.rows_repeated and torch.equal(unshared, together)
    host_lens, _ = _score(E, P, W, b, lens, hyps, blank, device_lens=False)
    assert torch.equal(host_lens, together)
    with pytest.raises(PafcError, match=r"utterance 0 alone has \d+ rows"):
        _score(E, P, W, b, lens, hyps, blank, max_rows=max(tb.utt_rows) - 1)


def test_device_length_that_is_not_the_tables_gives_nan(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    J, V, blank, T, lens = 64, 40, 0, 8, [8, 6]
    g = torch.Generator().manual_seed(4)
    hyps = [[_labels(2, V, blank, g), []], [_labels(3, V, blank, g)]]
    E, _, W, b = _inputs(2, T, 1, J, V, seed=29)
    P = _pred_rows(hyps, J, seed=8)
    good, tb = _score(E, P, W, b, lens, hyps, blank)
    for bad_len in (5, 9, 0):                              # not the tables'; beyond E; no frames
        bad = hip_ops.rnnt_score_hypotheses(E.float(), P.float(), W.float(), b.float(), torch.tensor([8, bad_len], device="cuda"),
                                            tb, blank)
        assert torch.equal(bad[:2], good[:2]) and torch.isnan(bad[2])


@pytest.mark.parametrize("blank", [0, 7])
def test_equals_brute_force_enumeration(hip, blank):
    J, V = 64, 40
    g = torch.Generator().manual_seed(blank)
    lens = [1, 3, 5, 4, 2]
    a = _labels(4, V, blank, g)
    hyps = [[[]], [a[:2], a[:1]], [a, a[:3] + _labels(1, V, blank, g), []], [a[:1], _labels(1, V, blank, g)], [a, []]]
    E, _, W, b = _inputs(5, 5, 1, J, V, seed=11 + blank)
    P = _pred_rows(hyps, J, seed=9)
    score, _ = _score(E, P, W, b, lens, hyps, blank)
    score = score.cpu()
    Wd, bd = W.double(), b.double()
    n = 0
    for bi, nbest in enumerate(hyps):
        for h in nbest:
            T, U = lens[bi], len(h)
            hh = torch.tanh(E[bi, :T, None, :].double() + P[n, None, :U + 1, :].double()).to(torch.bfloat16).double()
            logp = (hh @ Wd.t() + bd).log_softmax(-1).cpu()
            want = -_brute(logp, h, blank)
            assert float(score[n]) == pytest.approx(want, rel=1e-5), (T, U, float(score[n]), want)
            n += 1


def test_full_dims_against_fp64_restatement(hip):
    J, V, blank, lens = 640, 5000, 0, [37, 60]
    hyps = [_patterned(V, blank, seed=1, umax=12)[:4], _patterned(V, blank, seed=2, umax=9)[1:]]
    assert [len(nb) for nb in hyps] == [4, 4]
    E, _, W, b = _inputs(2, 64, 1, J, V, seed=3)          # padded beyond every length
    P = _pred_rows(hyps, J, seed=10)
    score, _ = _score(E, P, W, b, lens, hyps, blank)
    utt_of = [bi for bi, nbest in enumerate(hyps) for _ in nbest]
    flat = [h for nbest in hyps for h in nbest]
    with torch.no_grad():
        nll = _restated_fp64(E[utt_of].double(), P.double(), W.double(), b.double(), [lens[bi] for bi in utt_of],
                             [len(h) for h in flat], _ys(flat).cuda(), blank)
    rel = ((score.double() + nll).abs() / nll.abs()).max().item()
    assert rel <= 1e-4, (score.tolist(), nll.tolist())


# ---- through the model --------------------------------------------------------------------------------------------------------------
def _model(dtype, joint_kw=None, seed=0):
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    V, D, B, T = 56, 128, 3, 24
    torch.manual_seed(seed)
    enc_out = torch.randn(B, T, D) * 1.5
    pred = RNNPredictor(V, 64, 64, 0.1, 64, 2, True, "lstm", 0.1)
    joint = TransducerJoint(V, D, 64, 64, **(joint_kw or {}))
    model = Transducer(V, 0, _FixedEncoder(enc_out), pred, joint, ctc=CTC(V, D)).eval()
    speech = torch.zeros(B, T, 2, device="cuda", dtype=dtype)
    return model.to("cuda", dtype), speech, torch.tensor([24, 17, 5], device="cuda")


def test_decode_modes_through_the_kernels(hip):
    model, speech, lens = _model(torch.bfloat16)
    enc_out = model.encoder.enc_out
    wc, wt = 0.4, 1.1
    out = model.decode(["ctc_prefix_beam_search", "ctc_beam_td_rescoring"], speech, lens, beam_size=4, ctc_weight=wc,
                       transducer_weight=wt)
    first, second = out["ctc_prefix_beam_search"], out["ctc_beam_td_rescoring"]
    assert any(len(r.nbest) > 1 for r in first)
    td = model.score_hypotheses(enc_out, lens, [r.nbest for r in first], backend="kernels")
    assert all(all(t == t and t < 0 for t in td_b) for td_b in td)
    _check_second_pass(first, second, td, wc, wt)
    assert model.score_hypotheses(enc_out, lens, [r.nbest for r in first]) == td          # None on the GPU: the kernels
    first = model.decode(["rnnt_beam_search"], speech, lens, beam_size=4, ctc_weight=0.3, transducer_weight=0.7)["rnnt_beam_search"]
    for body in ("framework", "kernels"):
        second = model.decode(["rnnt_beam_td_rescoring"], speech, lens, beam_size=4, ctc_weight=wc, transducer_weight=wt,
                              frame_body=body)["rnnt_beam_td_rescoring"]
        if body == "framework":
            td = model.score_hypotheses(enc_out, lens, [r.nbest for r in first], backend="kernels")
            _check_second_pass(first, second, td, wc, wt)
        else:                                                  # frame_body is honoured: its own first pass, rescored
            assert all(len(r.nbest) == len(r.nbest_td_scores) >= 1 for r in second)


def test_score_hypotheses_reads_the_host_once(hip):
    model, speech, lens = _model(torch.bfloat16, seed=1)
    enc_out = model.encoder.enc_out
    hyps = [[[3, 9, 11], [3, 9], [5]], [[], [7, 7]], [[20]]]
    host_lens = lens.tolist()
    model.score_hypotheses(enc_out, host_lens, hyps, backend="kernels")                     # warm-up (binding, allocator)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            td = model.score_hypotheses(enc_out, host_lens, hyps, backend="kernels")
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    syncs = [w for w in caught if "called a synchronizing" in str(w.message)]
    assert len(syncs) <= 1, [str(w.message) for w in syncs]                               # the fetch of the scores
    assert [len(t) for t in td] == [3, 2, 1]


def test_fp32_model_kernels_against_framework_is_recorded(hip):
    """The kernels backend scores an fp32 model with the bf16 joint (the training kernel's contract).  No bound for that against
    the fp32 joint can be derived here, so the difference is recorded (tests/parity_log.py), not asserted."""
    model, speech, lens = _model(torch.float32, seed=2)
    enc_out = model.encoder.enc_out
    hyps = [[[3, 9, 11, 2, 40], [3, 9], [5]], [[], [7, 7]], [[20, 21, 22]]]
    k = model.score_hypotheses(enc_out, lens, hyps, backend="kernels")
    f = model.score_hypotheses(enc_out, lens, hyps, backend="framework")
    diff = [abs(a - c) for kb, fb in zip(k, f) for a, c in zip(kb, fb)]
    rel = [abs(a - c) / abs(c) for kb, fb in zip(k, f) for a, c in zip(kb, fb)]
    print("fp32 model: max |kernels - framework| td =", max(diff), "relative", max(rel))
    parity_log.record("rnnt_rescore_fp32_model_kernels_vs_framework", max_abs_td_diff=max(diff), max_rel_td_diff=max(rel),
                      hypotheses=len(diff))
    assert all(d == d for d in diff)


def test_ineligible_joint_raises(hip):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    model, speech, lens = _model(torch.bfloat16, joint_kw={"postjoin_linear": True})
    with pytest.raises(PafcError, match="postjoin_linear: true"):
        model.score_hypotheses(model.encoder.enc_out, lens, [[[3]], [[4]], [[5]]], backend="kernels")
    with pytest.raises(PafcError, match="postjoin_linear: true"):
        model.decode(["ctc_beam_td_rescoring"], speech, lens, beam_size=4, transducer_weight=1.0, score_backend="kernels")
    got = model.score_hypotheses(model.encoder.enc_out, lens, [[[3]], [[4]], [[5]]], backend="framework")     # asked for: fine
    assert all(len(g) == 1 for g in got)
