"""Context biasing and token time stamps of the GPU CTC prefix beam search (csrc/ctc_beam.hip:
pafc_ctc_prefix_beam_search_ex): the reference's golden on the device, device against the host loop at the decode tail's
size, the old entry point against the new one, and decode() of both model families with a context graph."""
import ctypes
import os
import random

import pytest
import torch

from tests.conftest import load_golden
from tests.test_ctc_context import make_graph, same_results

pytestmark = pytest.mark.gpu


def synthetic_graph(tmp_path, n_phrases, vocab, seed, context_score=3.0, pool=400):
    """A char-mode graph over a made-up table (one CJK character per token id): phrases of 1-6 tokens from a pool of
    `pool` ids, many sharing prefixes, some made of the tail of another (suffix overlaps, output arcs)."""
    from paper_accurate_fast_cheap_amd.utils.context_graph import ContextGraph
    rng = random.Random(seed)
    ids = rng.sample(range(1, vocab), pool)
    phrases = []
    for _ in range(n_phrases):
        r = rng.random()
        if phrases and r < 0.3:                              # shared prefix
            base = rng.choice(phrases)
            p = base[:rng.randint(1, len(base))] + [rng.choice(ids) for _ in range(rng.randint(0, 3))]
        elif phrases and r < 0.5:                            # a suffix of another phrase (+ maybe more)
            base = rng.choice(phrases)
            p = base[rng.randint(0, len(base) - 1):] + [rng.choice(ids) for _ in range(rng.randint(0, 2))]
        else:
            p = [rng.choice(ids) for _ in range(rng.randint(1, 6))]
        phrases.append(p[:6])
    table = {chr(0x4E00 + i): i for i in range(vocab)}
    path = tmp_path / f"phrases_{seed}.txt"
    path.write_text("\n".join("".join(chr(0x4E00 + t) for t in p) for p in phrases) + "\n", encoding="utf-8")
    return ContextGraph(str(path), table, None, context_score=context_score), phrases


def planted_logp(B, T, V, phrases, seed):
    """Random posteriors with blank runs, repeated tokens and phrases planted below a decoy (ranks 2-4)."""
    g = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)
    logits = torch.randn(B, T, V, generator=g)
    for b in range(B):
        t = 0
        while t < T:
            k = rng.random()
            if k < 0.3:
                n = rng.randint(1, 3)
                logits[b, t:t + n, 0] += 8.0
                t += n
            elif k < 0.6:
                u, n = rng.randrange(1, V), rng.randint(1, 3)
                logits[b, t:t + n, u] += 8.0
                t += n
            else:
                for tok in rng.choice(phrases):
                    if t + 3 > T:
                        break
                    logits[b, t:t + 2, rng.randrange(1, V)] += 8.0
                    logits[b, t:t + 2, tok] += 8.0 - rng.uniform(0.2, 2.0)
                    logits[b, t + 2, 0] += 6.0
                    t += 3
    return logits.log_softmax(-1)


@pytest.mark.parametrize("beam", [4, 8])
@pytest.mark.parametrize("cs", [None, 6.0, 2.5])
def test_golden_on_the_device(hip, beam, cs):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    gold = load_golden("ctc_context")
    graph = None if cs is None else make_graph("bpe", cs)
    got = ctc_prefix_beam_search(gold["logp"].cuda(), gold["lens"].cuda(), beam, graph, 0)
    same_results(got, gold["beam"][(beam, cs)], atol=1e-9, rel=1e-12)


def test_c5_times_on_the_device(hip):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    gold = load_golden("ctc_context")
    g = load_golden("search_c5")
    res = ctc_prefix_beam_search(g["logp"].cuda(), g["enc_lens"].cuda(), 8)
    for r, w in zip(res, gold["c5_times"]):
        assert list(r.tokens) == w["tokens"] and list(r.times) == w["times"]
        assert [list(x) for x in r.nbest_times] == w["nbest_times"]


@pytest.mark.parametrize("beam", [4, 8, 16])
@pytest.mark.parametrize("with_graph", [False, True])
def test_device_matches_host_at_decode_size(hip, tmp_path, beam, with_graph):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    B, T, V = 8, 500, 5000
    graph, phrases = synthetic_graph(tmp_path, 1000, V, seed=beam)
    logp = planted_logp(B, T, V, phrases, seed=100 + beam)
    lens = torch.randint(T // 3, T + 1, (B,), generator=torch.Generator().manual_seed(beam))
    lens[0] = T
    g = graph if with_graph else None
    want = ctc_prefix_beam_search(logp, lens, beam, g, 0)
    got = ctc_prefix_beam_search(logp.cuda(), lens.cuda(), beam, g, 0)
    for w, r in zip(want, got):
        assert [tuple(n) for n in r.nbest] == [tuple(n) for n in w.nbest]
        assert r.times == w.times and r.nbest_times == w.nbest_times
        assert r.nbest_scores == pytest.approx(w.nbest_scores, rel=1e-12, abs=1e-9)
    if with_graph:   # the graph is exercised: the host loop itself ranks differently without it
        plain = ctc_prefix_beam_search(logp, lens, beam, None, 0)
        assert any(p.nbest != w.nbest for p, w in zip(plain, want))


def test_old_and_new_entry_points_agree_bitwise(hip):
    from paper_accurate_fast_cheap_amd import _lib
    from paper_accurate_fast_cheap_amd.hip_ops import ctc_prefix_beam
    B, T, V, beam = 6, 300, 5000, 8
    logp = planted_logp(B, T, V, [[5, 6, 7]], seed=3).cuda()
    lens = torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(5)).cuda()
    top_p, top_i = logp.topk(beam, dim=-1)
    top_p, idx32 = top_p.contiguous(), top_i.to(torch.int32).contiguous()
    L = _lib.lib()
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.pafc_ctc_prefix_beam_workspace_bytes.restype = Z
    L.pafc_ctc_prefix_beam_workspace_bytes.argtypes = [I, I, I]
    L.pafc_ctc_prefix_beam_search.restype = I
    L.pafc_ctc_prefix_beam_search.argtypes = [I, I, I, P, P, P, I, I, P, P, P, P, Z, P]
    nws = L.pafc_ctc_prefix_beam_workspace_bytes(B, T, beam)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    toks = torch.full((B, beam, T), -7, dtype=torch.int32, device="cuda")
    ln = torch.empty(B, beam, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, beam, dtype=torch.float64, device="cuda")
    assert L.pafc_ctc_prefix_beam_search(B, T, beam, _lib.ptr(top_p), _lib.ptr(idx32), _lib.ptr(lens.to(torch.int64)),
                                         beam, 0, _lib.ptr(toks), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(ws), nws,
                                         _lib.stream_of(top_p)) == 0
    torch.cuda.synchronize()
    for want_times in (False, True):
        t2, l2, s2, tim = ctc_prefix_beam(top_p, top_i, lens, beam, 0, None, want_times)
        assert (tim is not None) == want_times
        assert torch.equal(l2, ln) and torch.equal(s2.view(torch.int64), sc.view(torch.int64))
        for b in range(B):
            for n in range(beam):
                k = int(ln[b, n])
                if k > 0:
                    assert torch.equal(t2[b, n, :k], toks[b, n, :k])


@pytest.mark.parametrize("family", ["asr", "transducer"])
def test_model_decode_with_context_graph(hip, tmp_path, family):
    """ASRModel.decode and Transducer.decode hand context_graph to the device search; the result equals the host loop on
    the same log-probs copied to the CPU."""
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    from tests.test_rnnt_greedy import D, V, _FixedEncoder, golden_model
    g = load_golden("rnnt_greedy_c5")
    torch.manual_seed(0)
    if family == "asr":
        model = ASRModel(V, _FixedEncoder(g["enc_out"]), CTC(V, D)).eval().cuda()
    else:
        model = golden_model(g, device="cuda")
    lens = g["enc_lens"].cuda()
    speech = torch.zeros(lens.shape[0], 37, 80, device="cuda")
    graph, _ = synthetic_graph(tmp_path, 40, V, seed=11, context_score=2.0, pool=20)
    with torch.no_grad():
        res = model.decode(["ctc_prefix_beam_search"], speech, lens, beam_size=4,
                           context_graph=graph)["ctc_prefix_beam_search"]
        logp = model.ctc.log_softmax(g["enc_out"].cuda())
    want = ctc_prefix_beam_search(logp.cpu(), lens.cpu(), 4, graph, 0)
    plain = ctc_prefix_beam_search(logp.cpu(), lens.cpu(), 4, None, 0)
    for w, r in zip(want, res):
        assert [tuple(n) for n in r.nbest] == [tuple(n) for n in w.nbest]
        assert r.times == w.times and r.nbest_times == w.nbest_times
        assert r.nbest_scores == pytest.approx(w.nbest_scores, rel=1e-12, abs=1e-9)
    assert [w.nbest_scores for w in want] != [p.nbest_scores for p in plain]     # the graph reached the search


def test_device_tables_built_once(hip, monkeypatch):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    graph = make_graph("bpe")
    calls = []
    orig = torch.Tensor.to

    def counting_to(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    gold = load_golden("ctc_context")
    logp, lens = gold["logp"].cuda(), gold["lens"].cuda()
    first = graph.device_tables("cuda")
    monkeypatch.setattr(torch.Tensor, "to", counting_to)
    n0 = len(calls)
    assert graph.device_tables(torch.device("cuda")) is first
    assert len(calls) == n0                                  # cached: nothing rebuilt or copied
    monkeypatch.undo()
    ctc_prefix_beam_search(logp, lens, 4, graph, 0)
    ctc_prefix_beam_search(logp, lens, 4, graph, 0)
    assert graph.device_tables("cuda") is first and len(graph._tables) == 1
