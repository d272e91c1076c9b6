"""Transducer rescoring of n-best lists (transducer/search/rescoring.py, Transducer.score_hypotheses and the decode modes
"ctc_beam_td_rescoring" / "rnnt_beam_td_rescoring"): checks that need no GPU -- the arc table of the prefix trie, the framework
backend against the enumeration of every alignment, and the second pass's arithmetic, order and tie rule."""
import itertools
import math
import random

import pytest
import torch

V, D, BLANK = 8, 6, 0


# ---- the arc table ----------------------------------------------------------------------------------------------------------------
def _nbest_lists():
    rng = random.Random(5)

    def rand_list(m, umax):
        return [[rng.randrange(1, V) for _ in range(rng.randrange(0, umax + 1))] for _ in range(m)]

    return [
        [[3, 4, 5]],                                         # one hypothesis
        [[]],                                                # the empty hypothesis alone
        [[], [2], [2, 6]],                                   # ... and beside others, each a strict prefix of the next
        [[1, 2, 3], [1, 2], [1, 2, 3, 4]],                   # a strict prefix that comes AFTER its extension
        [[1, 2], [3, 2]],                                    # two that diverge at the root
        [[5, 5], [5, 5], [5], [5, 5]],                       # duplicates
        [],                                                  # an utterance without hypotheses
        rand_list(6, 5), rand_list(8, 3), rand_list(3, 9),
    ]


def _trie_counts(nbest):
    """(edges, leaves) of the prefix trie of one n-best list, computed from sets of prefixes."""
    if not nbest:
        return 0, 0
    nodes = {tuple(h[:u]) for h in nbest for u in range(len(h) + 1)}
    edges = len(nodes) - 1
    inner = {p[:-1] for p in nodes if p}
    return edges, len(nodes - inner)


def test_arc_table_reconstructs_every_hypothesis_and_counts_rows():
    from paper_accurate_fast_cheap_amd.transducer.search.rescoring import build_arc_tables
    hyps = _nbest_lists()
    lens = [3 + b for b in range(len(hyps))]
    tb = build_arc_tables(hyps, lens, V, BLANK)
    flat = [h for nbest in hyps for h in nbest]
    assert tb.nutt == len(hyps) and tb.nhyp == len(flat)
    assert tb.pred_stride == max(len(h) for h in flat) + 1
    assert tb.packed.dtype == torch.int32 and tb.packed.numel() == 4 * tb.nutt + 2 + 2 * tb.narc + 3 * tb.nhyp + 1 + tb.ncol
    n = 0
    for b, nbest in enumerate(hyps):
        edges, leaves = _trie_counts(nbest)
        K = tb.arcs(b)
        assert K == edges + leaves, b
        a0 = int(tb.arc_off[b])
        assert int(tb.utt_enc[b]) == b and int(tb.utt_T[b]) == lens[b]
        assert int(tb.hyp_off[b]) == n
        for i, h in enumerate(nbest):
            assert int(tb.hyp_utt[n]) == b and int(tb.hyp_len[n]) == len(h)
            c0 = int(tb.col_off[n])
            assert int(tb.col_off[n + 1]) - c0 == len(h) + 1
            cols = tb.col[c0:c0 + len(h) + 1].tolist()
            assert all(0 <= k < K for k in cols)
            assert [int(tb.arc_label[a0 + k]) for k in cols[:-1]] == h            # the hypothesis, from col + labels
            for u, k in enumerate(cols):                                          # the arc's node is the prefix h[:u]
                n1, u1 = divmod(int(tb.arc_prow[a0 + k]), tb.pred_stride)
                assert u1 == u and int(tb.hyp_off[b]) <= n1 <= n
                assert flat[n1][:u] == h[:u], (b, i, u)
            n += 1
        # equal hypotheses share their columns
        for i, j in itertools.combinations(range(len(nbest)), 2):
            if nbest[i] == nbest[j]:
                ni, nj = int(tb.hyp_off[b]) + i, int(tb.hyp_off[b]) + j
                ci = tb.col[int(tb.col_off[ni]):int(tb.col_off[ni + 1])].tolist()
                assert ci == tb.col[int(tb.col_off[nj]):int(tb.col_off[nj + 1])].tolist()
    assert tb.arcs(0) == 4 and tb.arcs(1) == 1 and tb.arcs(6) == 0                # one hypothesis alone: U + 1 arcs; none: no rows
    assert tb.rows == sum(lens[b] * sum(_trie_counts(nbest)) for b, nbest in enumerate(hyps))
    assert tb.rows_repeated == sum(lens[b] * (len(h) + 1) for b, nbest in enumerate(hyps) for h in nbest)
    assert tb.rows < tb.rows_repeated
    # without sharing: every hypothesis its own utterance, the repeated rows
    alone = build_arc_tables(hyps, lens, V, BLANK, share=False)
    assert alone.nutt == alone.nhyp == len(flat) and alone.rows == alone.rows_repeated == tb.rows_repeated
    assert alone.utt_enc.tolist() == [b for b, nbest in enumerate(hyps) for _ in nbest]
    assert alone.pred_stride == tb.pred_stride
    for n, h in enumerate(flat):
        a0 = int(alone.arc_off[n])
        assert alone.arc_label[a0:a0 + len(h) + 1].tolist() == h + [-1]
        assert alone.arc_prow[a0:a0 + len(h) + 1].tolist() == [n * alone.pred_stride + u for u in range(len(h) + 1)]


def test_arc_table_refuses_bad_hypotheses():
    from paper_accurate_fast_cheap_amd.transducer.search.rescoring import build_arc_tables
    with pytest.raises(ValueError, match=r"utterance 1, hypothesis 2: the blank"):
        build_arc_tables([[[1]], [[1], [2], [3, BLANK, 4]]], [4, 4], V, BLANK)
    with pytest.raises(ValueError, match=r"utterance 0, hypothesis 1: token 8 outside"):
        build_arc_tables([[[1], [2, V]]], [4], V, BLANK)
    with pytest.raises(ValueError, match=r"utterance 0, hypothesis 0: token -1 outside"):
        build_arc_tables([[[-1]]], [4], V, BLANK)
    with pytest.raises(ValueError, match=r"utterance 2, hypothesis 0: 2559 tokens"):
        build_arc_tables([[], [[1]], [[1] * 2559]], [4, 4, 4], V, BLANK)
    build_arc_tables([[[1] * 2558]], [2], V, BLANK)                                # the longest lattice the kernels take


# ---- the model --------------------------------------------------------------------------------------------------------------------
class _FixedEncoder(torch.nn.Module):
    def __init__(self, enc_out):
        super().__init__()
        self.register_buffer("enc_out", enc_out)

    def output_size(self):
        return self.enc_out.shape[-1]

    def forward(self, x, lens, *a, **k):
        mask = (torch.arange(self.enc_out.shape[1], device=lens.device)[None, :] < lens[:, None]).unsqueeze(1)
        return self.enc_out[:x.shape[0]], mask


def tiny_model(T, B=2, seed=0, dtype=torch.float64, vocab=V, dim=D, join_dim=5, joint_kw=None):
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    torch.manual_seed(seed)
    enc_out = torch.randn(B, T, dim) * 1.5
    model = Transducer(vocab, BLANK, _FixedEncoder(enc_out), RNNPredictor(vocab, 4, 7, 0.0, 7, 1, dropout=0.0),
                       TransducerJoint(vocab, dim, 7, join_dim, **(joint_kw or {})), ctc=CTC(vocab, dim)).eval()
    return model.to(dtype)


def brute(logp, y, blank):
    """log of the sum over every monotone alignment of T blanks and U labels through the (T, U + 1) lattice."""
    T, U1, _ = logp.shape
    U = U1 - 1
    total = []
    for pos in itertools.combinations(range(T + U), U):
        t = u = 0
        s, ok = 0.0, True
        for step in range(T + U):
            if step in pos:
                if t >= T:
                    ok = False
                    break
                s += float(logp[t, u, y[u]])
                u += 1
            else:
                s += float(logp[t, u, blank])
                t += 1
        if ok and t == T and u == U:
            total.append(s)
    m = max(total)
    return m + math.log(sum(math.exp(v - m) for v in total))


def test_framework_score_equals_brute_force_enumeration():
    from paper_accurate_fast_cheap_amd.transducer.transducer import add_blank
    model = tiny_model(T=4)
    enc_out = model.encoder.enc_out
    lens = [4, 2]
    hyps = [[[3, 1, 6], [3, 1], [], [7], [3, 1, 6]], [[2, 2, 5], [4]]]
    got = model.score_hypotheses(enc_out, torch.tensor(lens), hyps, backend="framework")
    assert [len(g) for g in got] == [5, 2]
    assert model.score_hypotheses(enc_out, lens, hyps) == got                      # None on the CPU: the framework backend
    with torch.no_grad():
        for b, nbest in enumerate(hyps):
            for i, h in enumerate(nbest):
                ys = torch.tensor([h], dtype=torch.int64).view(1, len(h))
                pred = model.predictor(add_blank(ys, BLANK, -1))
                logp = model.joint(enc_out[b:b + 1, :lens[b]], pred)[0].log_softmax(-1)
                assert got[b][i] == pytest.approx(brute(logp, h, BLANK), rel=1e-9), (b, i)
    assert got[0][0] == got[0][4]                                                  # duplicates
    assert model.score_hypotheses(enc_out, lens, [[], []]) == [[], []]


def test_score_hypotheses_validates_its_arguments():
    from paper_accurate_fast_cheap_amd._lib import PafcError
    model = tiny_model(T=3)
    enc_out = model.encoder.enc_out
    with pytest.raises(ValueError, match="backend must be one of"):
        model.score_hypotheses(enc_out, [3, 3], [[[1]], [[2]]], backend="eager")
    with pytest.raises(ValueError, match="utterance 1, hypothesis 0: the blank"):
        model.score_hypotheses(enc_out, [3, 3], [[[1]], [[BLANK]]], backend="framework")
    with pytest.raises(ValueError, match="2 utterances, 1 n-best lists"):
        model.score_hypotheses(enc_out, [3, 3], [[[1]]])
    with pytest.raises(PafcError, match="not on the GPU"):                         # never a fallback
        model.score_hypotheses(enc_out, [3, 3], [[[1]], [[2]]], backend="kernels")
    post = tiny_model(T=3, joint_kw={"postjoin_linear": True})
    with pytest.raises(PafcError, match="postjoin_linear: true"):
        post.score_hypotheses(post.encoder.enc_out, [3, 3], [[[1]], [[2]]], backend="kernels")


# ---- the second pass --------------------------------------------------------------------------------------------------------------
def _check_second_pass(first, second, td, wc, wt):
    for r1, r2, td_b in zip(first, second, td):
        assert sorted(map(tuple, r2.nbest)) == sorted(map(tuple, r1.nbest))        # the first pass's hypothesis set
        final = [wc * s + wt * t for s, t in zip(r1.nbest_scores, td_b)]
        order = sorted(range(len(final)), key=lambda i: -final[i])                 # stable: ties to the earlier rank
        assert r2.nbest == [r1.nbest[i] for i in order]
        assert r2.nbest_scores == pytest.approx([final[i] for i in order], rel=1e-12)
        assert r2.nbest_td_scores == pytest.approx([td_b[i] for i in order], rel=1e-12)
        assert all(a >= b for a, b in zip(r2.nbest_scores, r2.nbest_scores[1:]))
        assert r2.tokens == r2.nbest[0] and r2.score == r2.nbest_scores[0]
        if r1.nbest_times is not None:
            assert r2.nbest_times == [r1.nbest_times[i] for i in order] and r2.times == r2.nbest_times[0]
        else:
            assert r2.nbest_times is None and r2.times is None


@pytest.fixture(scope="module")
def decode_model():
    model = tiny_model(T=6, B=3, seed=3)
    speech = torch.zeros(3, 6, 2, dtype=torch.float64)
    return model, speech, torch.tensor([6, 4, 1])


def test_decode_ctc_beam_td_rescoring(decode_model):
    model, speech, lens = decode_model
    wc, wt = 0.4, 1.3
    out = model.decode(["ctc_prefix_beam_search", "ctc_beam_td_rescoring"], speech, lens, beam_size=4, ctc_weight=wc,
                       transducer_weight=wt)
    first, second = out["ctc_prefix_beam_search"], out["ctc_beam_td_rescoring"]
    assert any(len(r.nbest) > 1 for r in first)
    td = model.score_hypotheses(model.encoder.enc_out, lens, [r.nbest for r in first])
    _check_second_pass(first, second, td, wc, wt)
    assert all(r.nbest_times is not None for r in second)
    alone = model.decode(["ctc_beam_td_rescoring"], speech, lens, beam_size=4, ctc_weight=wc, transducer_weight=wt)
    assert list(alone) == ["ctc_beam_td_rescoring"]                                # the first pass is not reported unasked
    assert [r.nbest for r in alone["ctc_beam_td_rescoring"]] == [r.nbest for r in second]
    same = model.decode(["ctc_beam_td_rescoring"], speech, lens, beam_size=4, ctc_weight=1.0, transducer_weight=0.0)
    for r1, r2 in zip(first, same["ctc_beam_td_rescoring"]):                       # weights (1, 0): the first pass's order
        assert r2.nbest == r1.nbest and r2.nbest_scores == r1.nbest_scores and r2.nbest_times == r1.nbest_times


def test_decode_rnnt_beam_td_rescoring(decode_model):
    model, speech, lens = decode_model
    first = model.decode(["rnnt_beam_search"], speech, lens, beam_size=4, ctc_weight=0.3, transducer_weight=0.7)["rnnt_beam_search"]
    wc, wt = 0.5, 0.5
    second = model.decode(["rnnt_beam_td_rescoring"], speech, lens, beam_size=4, ctc_weight=wc,
                          transducer_weight=wt)["rnnt_beam_td_rescoring"]         # search weights: 0.3 / 0.7 by default
    assert any(len(r.nbest) > 1 for r in first)
    td = model.score_hypotheses(model.encoder.enc_out, lens, [r.nbest for r in first])
    _check_second_pass(first, second, td, wc, wt)
    other = model.decode(["rnnt_beam_search"], speech, lens, beam_size=4, ctc_weight=0.9, transducer_weight=0.1)["rnnt_beam_search"]
    second = model.decode(["rnnt_beam_td_rescoring"], speech, lens, beam_size=4, ctc_weight=1.0, transducer_weight=0.0,
                          search_ctc_weight=0.9, search_transducer_weight=0.1)["rnnt_beam_td_rescoring"]
    for r1, r2 in zip(other, second):                                              # weights (1, 0): the first pass's order
        assert r2.nbest == r1.nbest and r2.nbest_scores == r1.nbest_scores


def test_decode_refuses_the_attention_term_and_unknown_modes(decode_model):
    model, speech, lens = decode_model
    for mode in ("ctc_beam_td_rescoring", "rnnt_beam_td_rescoring"):
        with pytest.raises(ValueError, match="attention decoder was not released"):
            model.decode([mode], speech, lens, beam_size=4, reverse_weight=0.3)
        with pytest.raises(ValueError, match="attention decoder was not released"):
            model.decode([mode], speech, lens, beam_size=4, attn_weight=0.5)
    with pytest.raises(NotImplementedError):
        model.decode(["rnnt_beam_attn_rescoring"], speech, lens, beam_size=4)


def test_rescore_ties_go_to_the_earlier_first_pass_rank():
    from paper_accurate_fast_cheap_amd.transducer.search.rescoring import rescore
    from paper_accurate_fast_cheap_amd.transformer.search import DecodeResult
    first = DecodeResult(tokens=[1], score=-1.0, times=[0], nbest=[[1], [2], [3], [4]], nbest_scores=[-1.0, -2.0, -3.0, -4.0],
                         nbest_times=[[0], [1], [2], [3]])
    # final = first + td: -5, -4, -4, -5 -> ranks 1 and 2 tie for the top, then 0 and 3 tie
    out = rescore([first], [[-4.0, -2.0, -1.0, -1.0]], 1.0, 1.0)[0]
    assert out.nbest == [[2], [3], [1], [4]] and out.nbest_scores == [-4.0, -4.0, -5.0, -5.0]
    assert out.nbest_times == [[1], [2], [0], [3]] and out.times == [1] and out.tokens == [2] and out.score == -4.0
    assert out.nbest_td_scores == [-2.0, -1.0, -4.0, -1.0]
    assert DecodeResult([1]).nbest_td_scores is None                               # existing constructions are unaffected
    empty = rescore([DecodeResult(tokens=[], score=0.0, nbest=[], nbest_scores=[])], [[]], 1.0, 1.0)[0]
    assert empty.nbest == [] and empty.tokens == []


# ---- the C boundary: everything a kernel indexes with is checked on the host copy of the tables, before any launch ----------------
@pytest.fixture(scope="module")
def lib():
    import ctypes
    import os
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    L = ctypes.CDLL(build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT)
    for name in ("pafc_rnnt_score_workspace_bytes", "pafc_rnnt_score"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    return L


def test_entry_validates_the_tables_before_touching_the_device(lib):
    import ctypes
    from paper_accurate_fast_cheap_amd.transducer.search.rescoring import build_arc_tables
    ERR_NULL, ERR_DIMS, ERR_WS, ERR_UNSUP, ERR_ALIGN = -1, -2, -4, -7, -8
    NULL, one = ctypes.c_void_p(0), ctypes.c_void_p(256)          # aligned, never dereferenced: validation fails first
    Benc, T, J, Vk, prows = 2, 6, 64, 40, 12
    hyps = [[[3, 4, 5], [3, 9]], [[7]]]

    def call(tb=None, mutate=None, J=J, V=Vk, E=one, utt=(0, 2), blank=0, ws_bytes=0, prows=prows, lde=None):
        lde = J if lde is None else lde
        tb = tb or build_arc_tables(hyps, [6, 4], Vk, 0)
        packed = tb.packed.clone()
        if mutate:
            name, idx, val = mutate
            at = sum(len(getattr(tb, f)) for f in tb.FIELDS[:tb.FIELDS.index(name)])
            packed[at + idx] = val
        host = ctypes.c_void_p(packed.data_ptr())
        return lib.pafc_rnnt_score(Benc, T, J, V, E, lde, T * lde, one, J, prows, one, NULL, NULL, tb.nutt, tb.nhyp, tb.narc, tb.ncol,
                                   host, one, utt[0], utt[1], blank, one, one, ws_bytes, NULL)

    assert call() == ERR_WS                                       # sound tables: the next check is the workspace
    assert call(E=NULL) == ERR_NULL
    assert call(J=96) == ERR_UNSUP and call(V=42) == ERR_UNSUP
    assert call(lde=68) == ERR_ALIGN
    assert call(blank=Vk) == ERR_DIMS and call(utt=(1, 1)) == ERR_DIMS and call(utt=(0, 3)) == ERR_DIMS
    for mutate in (("utt_enc", 1, 2), ("utt_enc", 0, -1), ("utt_T", 0, 7), ("utt_T", 1, 0), ("arc_off", 1, 99), ("arc_off", 1, -1),
                   ("hyp_off", 1, 5), ("arc_prow", 0, prows), ("arc_prow", 2, -1), ("arc_label", 0, Vk), ("arc_label", 1, -2),
                   ("hyp_utt", 0, 1), ("hyp_len", 0, 4), ("hyp_len", 1, -1), ("col_off", 1, 3), ("col", 0, 5), ("col", 1, -1)):
        assert call(mutate=mutate) == ERR_DIMS, mutate
    tb = build_arc_tables(hyps, [6, 4], Vk, 0)
    leaf = int(tb.col[int(tb.col_off[1]) - 1])                    # the label-less arc at the end of hypothesis 0 ...
    assert int(tb.arc_label[leaf]) == -1
    assert call(mutate=("col", 0, leaf)) == ERR_DIMS              # ... cannot stand at a position that emits a label
    assert call(mutate=("hyp_len", 0, 2559)) in (ERR_DIMS, ERR_UNSUP)
    assert call(utt=(1, 2), mutate=("utt_T", 0, 99)) == ERR_WS    # only the group's utterances are read
    rows = 6 * tb.arcs(0) + 4 * tb.arcs(1)
    need = lib.pafc_rnnt_score_workspace_bytes(2, J, Vk, rows)
    assert need >= rows * (2 * J + 8 + 16) and lib.pafc_rnnt_score_workspace_bytes(2, J, Vk, 0) == 0
    assert call(ws_bytes=need - 1) == ERR_WS
