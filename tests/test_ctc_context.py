"""Context biasing and token time stamps of the CTC prefix beam search, on CPU: the ContextGraph port and the host loop
against the reference's own output (tests/golden/ctc_context.pt, captured by make_goldens_ctc_context.py), plus the
argument checks and register use of the new kernel entry point (cross-compiled here, no GPU)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.conftest import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = os.path.join(GOLDEN, "text")


@pytest.fixture(scope="module")
def gold():
    return load_golden("ctc_context")


def symbol_table():
    table = {}
    with open(os.path.join(TEXT, "units.txt"), encoding="utf-8") as f:
        for line in f:
            name, idx = line.split()
            table[name] = int(idx)
    return table


def make_graph(mode="bpe", context_score=6.0):
    from paper_accurate_fast_cheap_amd.utils.context_graph import ContextGraph
    if mode == "bpe":
        return ContextGraph(os.path.join(TEXT, "context_list.txt"), symbol_table(), os.path.join(TEXT, "spm_tiny.model"),
                            context_score=context_score)
    return ContextGraph(os.path.join(TEXT, "context_list_char.txt"), symbol_table(), None, context_score=context_score)


def same_results(got, want, atol=1e-9, rel=0.0):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g.tokens) == w["tokens"]
        assert [list(n) for n in g.nbest] == w["nbest"]
        assert list(g.times) == w["times"]
        assert [list(x) for x in g.nbest_times] == w["nbest_times"]
        assert g.score == pytest.approx(w["score"], rel=rel, abs=atol)
        assert g.nbest_scores == pytest.approx(w["nbest_scores"], rel=rel, abs=atol)


def test_tokenize_matches_reference(gold):
    from paper_accurate_fast_cheap_amd.utils.context_graph import tokenize
    assert tokenize(os.path.join(TEXT, "context_list.txt"), symbol_table(),
                    os.path.join(TEXT, "spm_tiny.model")) == gold["tokenized_bpe"]
    assert tokenize(os.path.join(TEXT, "context_list_char.txt"), symbol_table(), None) == gold["tokenized_char"]


@pytest.mark.parametrize("mode", ["bpe", "char"])
def test_graph_tables_and_walks_match_reference(gold, mode):
    g = make_graph(mode)
    want = gold["graph_" + mode]
    tab = g.device_tables("cpu")
    for k in ("child_begin", "child_token", "child_node", "fail"):
        assert tab[k].dtype == torch.int32 and tab[k].tolist() == want[k], k
    for k in ("token_score", "node_score", "output_score"):
        assert tab[k].dtype == torch.float64 and tab[k].tolist() == want[k], k
    assert g.device_tables("cpu") is tab                         # built once per device
    nodes = {0: g.root}
    stack = [g.root]
    while stack:
        n = stack.pop()
        nodes[n.id] = n
        stack.extend(n.next.values())
    for state, tok, score, nxt in gold["walks_" + mode]:
        sc, st = g.forward_one_step(nodes[state], tok)
        assert (sc, st.id) == (score, nxt), (state, tok)
    fsc, fst = g.finalize(nodes[len(nodes) - 1])
    assert fst is g.root and fsc == -nodes[len(nodes) - 1].node_score


@pytest.mark.parametrize("beam", [4, 8])
@pytest.mark.parametrize("cs", [None, 6.0, 2.5])
def test_host_loop_matches_reference(gold, beam, cs):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    graph = None if cs is None else make_graph("bpe", cs)
    got = ctc_prefix_beam_search(gold["logp"], gold["lens"], beam, graph, 0)
    same_results(got, gold["beam"][(beam, cs)])


def test_biasing_changes_the_result(gold):
    """the fixture is not vacuous: some 1-best differs with the graph"""
    b = gold["beam"]
    assert any(b[(8, 6.0)][i]["tokens"] != b[(8, None)][i]["tokens"] for i in range(len(gold["lens"])))


def test_zero_length_utterance_has_no_times():
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    logp = torch.log_softmax(torch.randn(1, 4, 100), -1)
    r = ctc_prefix_beam_search(logp, torch.tensor([0]), 4, make_graph(), 0)[0]
    assert r.times == [] and r.nbest_times == [[]] and list(r.tokens) == [] and r.score == 0.0


def test_c5_times_without_graph(gold):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_prefix_beam_search
    g = load_golden("search_c5")
    res = ctc_prefix_beam_search(g["logp"], g["enc_lens"], 8, None, 0)
    for r, w in zip(res, gold["c5_times"]):
        assert list(r.tokens) == w["tokens"]
        assert list(r.times) == w["times"] and [list(x) for x in r.nbest_times] == w["nbest_times"]


def test_asr_model_decode_accepts_context_graph():
    """ASRModel.decode names context_graph and hands it to the search (it used to vanish into **kwargs)."""
    import inspect
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    assert "context_graph" in inspect.signature(ASRModel.decode).parameters


# ---- the C entry point, cross-compiled here ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def so_path():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    return build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT


class Graph(ctypes.Structure):
    _fields_ = [("num_nodes", ctypes.c_int), ("child_begin", ctypes.c_void_p), ("child_token", ctypes.c_void_p),
                ("child_node", ctypes.c_void_p), ("fail", ctypes.c_void_p), ("token_score", ctypes.c_void_p),
                ("node_score", ctypes.c_void_p), ("output_score", ctypes.c_void_p)]


def test_ex_entry_point_validates_arguments(so_path):
    L = ctypes.CDLL(so_path)
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    NULL, one = P(0), P(16)
    ERR_NULL, ERR_DIMS, ERR_WS, ERR_UNSUP = -1, -2, -4, -7
    L.pafc_ctc_prefix_beam_ex_workspace_bytes.restype = Z
    L.pafc_ctc_prefix_beam_ex_workspace_bytes.argtypes = [I, I, I]
    ws = L.pafc_ctc_prefix_beam_ex_workspace_bytes(2, 10, 4)
    assert ws >= L.pafc_ctc_prefix_beam_ex_workspace_bytes(2, 10, 3) > 0
    assert L.pafc_ctc_prefix_beam_ex_workspace_bytes(0, 10, 4) == 0
    f = L.pafc_ctc_prefix_beam_search_ex
    f.argtypes = [I, I, I, P, P, P, I, I, ctypes.POINTER(Graph), P, P, P, P, P, Z, P]
    g = Graph(3, one, one, one, one, one, one, one)
    gp = ctypes.byref(g)
    ok = (2, 10, 4, one, one, NULL, 4, 0)
    assert f(2, 10, 4, NULL, one, NULL, 4, 0, gp, one, one, one, one, one, ws, NULL) == ERR_NULL
    assert f(*ok, gp, one, one, one, one, NULL, ws, NULL) == ERR_NULL                 # workspace
    assert f(0, 10, 4, one, one, NULL, 4, 0, gp, one, one, one, one, one, ws, NULL) == ERR_DIMS
    assert f(2, 10, 4, one, one, NULL, 4, -1, gp, one, one, one, one, one, ws, NULL) == ERR_DIMS
    assert f(2, 10, 17, one, one, NULL, 17, 0, gp, one, one, one, one, one, 1 << 20, NULL) == ERR_UNSUP
    assert f(2, 10, 4, one, one, NULL, 17, 0, None, one, one, one, NULL, one, 1 << 20, NULL) == ERR_UNSUP
    assert f(*ok, gp, one, one, one, one, one, ws - 1, NULL) == ERR_WS
    for i in range(1, 8):                                                             # every table pointer
        bad = Graph(3, *[0 if j == i else 16 for j in range(1, 8)])
        assert f(*ok, ctypes.byref(bad), one, one, one, one, one, ws, NULL) == ERR_NULL, i
    assert f(*ok, ctypes.byref(Graph(0, *[16] * 7)), one, one, one, one, one, ws, NULL) == ERR_DIMS


def test_ex_kernels_do_not_spill(tmp_path):
    src = os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc", "ctc_beam.hip")
    out = tmp_path / "ctc_beam.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.dirname(src), "-S", "--cuda-device-only", src,
                           "-o", str(out)], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    names = set(re.findall(r"^(_ZN4pafc[^\s:]*ctc_prefix_beam_kernel[^\s:]*):", asm, flags=re.M))
    assert len(names) == 4, names                                  # <CTX, TIMES> in all four combinations
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)     # (SGPR spills go to VGPR lanes, not to memory)
    assert spills and all(int(v) == 0 for v in spills)
    priv = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm)
    assert priv and all(int(v) == 0 for v in priv)
    assert "scratch_" not in asm
