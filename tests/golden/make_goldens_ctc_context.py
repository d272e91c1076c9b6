"""Capture the context-biasing / time-stamp golden of the CTC prefix beam search from the reference's own code.

Run ONCE where the reference tree is available:
    python tests/golden/make_goldens_ctc_context.py
It imports the reference through oracle/ref_shim.py and runs, on CPU, its `tokenize` and `ContextGraph`
(wenet/utils/context_graph.py) and its `ctc_prefix_beam_search` (wenet/transformer/search.py:124-248), and stores in
ctc_context.pt:
  * graph_bpe / graph_char: the reference graph of text/context_list.txt (spm_tiny.model + units.txt) and of
    text/context_list_char.txt (char mode, same table), flattened like ContextGraph.device_tables: children sorted by
    token, node ids as the reference numbers them;
  * walks: forward_one_step (state id, token) -> (score, next state id) over every node x a token set;
  * beam: synthetic log-probs (V = 100, ragged T <= 80) with phrase tokens planted at ranks 2-4 of a frame's top-k, and the
    reference's tokens / score / times / nbest / nbest_scores / nbest_times for beam 4 and 8, without a graph and with the
    graph at context_score 6.0 and 2.5;
  * c5_times: times / nbest_times without a graph for search_c5.pt's own logp (beam 8).
The script asserts that the fixture covers what the port must reproduce: a 1-best that biasing changes, a hypothesis that
ends mid-phrase (finalize backs off), fail arcs between overlapping phrases and an output arc, and both repeat transitions
(*uu -> *u, counted through the reference's misspelt `vs_ns` assignment, and *u-u -> *uu, a doubled token in a result).
The fixture holds data only.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

TEXT = os.path.join(HERE, "text")
V, SEED = 100, 7
LENS = [80, 61, 47, 72, 33, 0, 55]
BEAMS = (4, 8)
SCORES = (6.0, 2.5)


def symbol_table():
    table = {}
    with open(os.path.join(TEXT, "units.txt"), encoding="utf-8") as f:
        for line in f:
            name, idx = line.split()
            table[name] = int(idx)
    return table


def flatten(graph):
    nodes = {}
    stack = [graph.root]
    while stack:
        n = stack.pop()
        nodes[n.id] = n
        stack.extend(n.next.values())
    assert sorted(nodes) == list(range(len(nodes)))
    begin, ctok, cnode = [0], [], []
    for i in range(len(nodes)):
        for tok in sorted(nodes[i].next):
            ctok.append(tok)
            cnode.append(nodes[i].next[tok].id)
        begin.append(len(ctok))
    return nodes, dict(child_begin=begin, child_token=ctok, child_node=cnode,
                       fail=[nodes[i].fail.id for i in range(len(nodes))],
                       token_score=[float(nodes[i].token_score) for i in range(len(nodes))],
                       node_score=[float(nodes[i].node_score) for i in range(len(nodes))],
                       output_score=[float(nodes[i].output_score) for i in range(len(nodes))],
                       is_end=[bool(nodes[i].is_end) for i in range(len(nodes))],
                       phrases=[list(p) for p in graph.context_list])


def synth_logp(phrases):
    """Frames in segments: blank runs, token runs (1-3 frames; a token run may repeat after one blank), and planted
    phrases whose tokens sit just below a random top token (rank 2-4 of the top-k)."""
    g = torch.Generator().manual_seed(SEED)
    B, T = len(LENS), max(LENS)
    logits = torch.randn(B, T, V, generator=g)
    for b in range(B):
        t = 0
        while t < T:
            kind = int(torch.randint(0, 4, (1,), generator=g))
            if kind == 0:                                   # blank run
                n = int(torch.randint(1, 4, (1,), generator=g))
                logits[b, t:t + n, 0] += 6.0
                t += n
            elif kind == 1:                                 # token run, maybe "u - u"
                u = int(torch.randint(3, V - 1, (1,), generator=g))
                n = int(torch.randint(1, 4, (1,), generator=g))
                logits[b, t:t + n, u] += 6.0
                t += n
                if t + 2 <= T and float(torch.rand(1, generator=g)) < 0.4:
                    logits[b, t, 0] += 6.0
                    logits[b, t + 1, u] += 6.0
                    t += 2
            else:                                           # a phrase (or its first half) below a decoy
                p = phrases[int(torch.randint(0, len(phrases), (1,), generator=g))]
                if kind == 3:
                    p = p[:max(1, len(p) - 1)]
                for tok in p:
                    if t + 2 > T:
                        break
                    decoy = int(torch.randint(3, V - 1, (1,), generator=g))
                    gap = 0.3 + 1.5 * float(torch.rand(1, generator=g))
                    logits[b, t:t + 2, decoy] += 6.0
                    logits[b, t:t + 2, tok] += 6.0 - gap
                    logits[b, t + 2:t + 3, 0] += 5.0
                    t += 3
    return logits.log_softmax(-1)


def main():
    from oracle import ref_shim
    ref_shim.install()
    import wenet.transformer.search as RS
    from wenet.utils.context_graph import ContextGraph, tokenize

    table = symbol_table()
    bpe = os.path.join(TEXT, "spm_tiny.model")
    phrase_path = os.path.join(TEXT, "context_list.txt")
    char_path = os.path.join(TEXT, "context_list_char.txt")
    out = dict(V=V, lens=torch.tensor(LENS), beams=BEAMS, context_scores=SCORES,
               tokenized_bpe=tokenize(phrase_path, table, bpe), tokenized_char=tokenize(char_path, table, None))

    graphs = {}
    for name, path, model in (("bpe", phrase_path, bpe), ("char", char_path, None)):
        gr = ContextGraph(path, table, model, context_score=6.0)
        nodes, flat = flatten(gr)
        out["graph_" + name] = flat
        graphs[name] = (gr, nodes)
        walks = []
        toks = sorted({t for p in gr.context_list for t in p} | {0, 2, 50})
        for i in range(len(nodes)):
            for tok in toks:
                sc, nxt = gr.forward_one_step(nodes[i], tok)
                walks.append((i, tok, float(sc), nxt.id))
        out["walks_" + name] = walks
    # coverage of the graph: fail arcs between phrases, an output arc, a negative fail-path score
    flat = out["graph_bpe"]
    assert any(f != 0 for f in flat["fail"][1:]), "no fail arc between phrases"
    assert any(n.output is not None for n in graphs["bpe"][1].values()), "no output arc"
    assert any(sc < 0 for _, _, sc, _ in out["walks_bpe"]), "no negative fail-path score"

    # the *uu -> *u branch: the reference assigns `vs_ns` there -- count it
    hits = {"uu_u": 0}

    class Counting(RS.PrefixScore):
        @property
        def vs_ns(self):
            return self._vs_ns

        @vs_ns.setter
        def vs_ns(self, v):
            hits["uu_u"] += 1
            self._vs_ns = v

    RS.PrefixScore = Counting

    phrases = [p for p in flat["phrases"] if p]
    logp = synth_logp(phrases)
    lens = torch.tensor(LENS)
    out["logp"] = logp
    beam_res = {}
    gr_bpe, nodes_bpe = graphs["bpe"]
    for beam in BEAMS:
        for cs in (None,) + SCORES:
            graph = None if cs is None else ContextGraph(phrase_path, table, bpe, context_score=cs)
            res = RS.ctc_prefix_beam_search(logp, lens, beam, graph, 0)
            beam_res[(beam, cs)] = [dict(tokens=list(r.tokens), score=float(r.score), times=list(r.times),
                                         nbest=[list(n) for n in r.nbest], nbest_scores=[float(s) for s in r.nbest_scores],
                                         nbest_times=[list(x) for x in r.nbest_times]) for r in res]
    out["beam"] = beam_res

    # coverage of the search
    changed = any(beam_res[(bm, cs)][b]["tokens"] != beam_res[(bm, None)][b]["tokens"]
                  for bm in BEAMS for cs in SCORES for b in range(len(LENS)))
    assert changed, "biasing never changes a 1-best"
    mid = False
    for bm in BEAMS:
        for cs in SCORES:
            for r in beam_res[(bm, cs)]:
                for hyp in r["nbest"]:
                    st = gr_bpe.root
                    for tok in hyp:
                        st = gr_bpe.forward_one_step(st, tok)[1]
                    mid |= st.id != 0 and not st.is_end
    assert mid, "no hypothesis ends mid-phrase"
    assert hits["uu_u"] > 0, "no *uu -> *u transition"
    assert any(h[i] == h[i + 1] for rs in beam_res.values() for r in rs for h in r["nbest"] for i in range(len(h) - 1)), \
        "no *u-u -> *uu transition"
    assert beam_res[(4, 6.0)][LENS.index(0)]["times"] == []

    c5 = torch.load(os.path.join(HERE, "search_c5.pt"), weights_only=False)
    res = RS.ctc_prefix_beam_search(c5["logp"], c5["enc_lens"], 8, None, 0)
    out["c5_times"] = [dict(tokens=list(r.tokens), times=list(r.times), nbest_times=[list(x) for x in r.nbest_times])
                       for r in res]
    path = os.path.join(HERE, "ctc_context.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes); *uu->*u hits {hits['uu_u']}")


if __name__ == "__main__":
    main()
