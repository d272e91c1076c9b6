"""Hotword / context biasing graph of the CTC prefix beam search (``wenet/utils/context_graph.py``).

A ContextGraph is a trie of boosted phrases with Aho-Corasick fail arcs: every matched token of a phrase earns
``context_score``; leaving a phrase part-way takes back what the partial match earned (the fail arc's score is the
difference of the two nodes' accumulated scores); a node whose phrase -- or a phrase that is a suffix of it -- ends there
adds ``output_score``.  Names, signatures and arithmetic follow the reference, node numbering included (creation order,
root 0), so scores agree bit for bit.

``device_tables(device)`` flattens the graph for the GPU search (csrc/ctc_beam.hip): children sorted by token (CSR),
fail arcs and the three score columns, built once per device.
"""
import re
from collections import deque
from typing import Dict, List, Optional, Tuple

import torch

_CJK = re.compile(r"([\u4e00-\u9fff])")   # CJK unified ideographs


def _bpe_pieces(sp, txt: str) -> List[str]:
    """Upper-cased text, CJK characters one token each, everything else SentencePiece pieces
    (``tokenize_by_bpe_model``, ``wenet/text/tokenize_utils.py``)."""
    out: List[str] = []
    for part in _CJK.split(txt.upper()):
        if len(part.strip()) == 0:
            continue
        if _CJK.fullmatch(part) is not None:
            out.append(part)
        else:
            out.extend(sp.encode_as_pieces(part))
    return out


def tokenize(context_list_path: str, symbol_table: Dict[str, int], bpe_model: Optional[str] = None) -> List[List[int]]:
    """One token-id list per line of the phrase file.  BPE mode: see _bpe_pieces; char mode: one token per character, a
    space becomes ``▁``.  Pieces missing from the table become ``<unk>`` if the table has one and are dropped otherwise."""
    sp = None
    if bpe_model is not None:
        import sentencepiece as spm
        sp = spm.SentencePieceProcessor()
        sp.load(bpe_model)
    with open(context_list_path, "r") as f:
        lines = f.readlines()
    phrases = []
    for line in lines:
        line = line.strip()
        pieces = _bpe_pieces(sp, line) if sp is not None else ["▁" if ch == " " else ch for ch in line]
        ids = []
        for p in pieces:
            if p in symbol_table:
                ids.append(symbol_table[p])
            elif "<unk>" in symbol_table:
                ids.append(symbol_table["<unk>"])
        phrases.append(ids)
    return phrases


class ContextState:
    """A node of the graph.  node_score: bonus accumulated from the root; output_score: bonus of every phrase that ends
    here (this node's own, if it ends one, plus its output node's)."""

    def __init__(self, id: int, token: int, token_score: float, node_score: float, output_score: float, is_end: bool):
        self.id = id
        self.token = token
        self.token_score = token_score
        self.node_score = node_score
        self.output_score = output_score
        self.is_end = is_end
        self.next: Dict[int, "ContextState"] = {}
        self.fail: Optional["ContextState"] = None
        self.output: Optional["ContextState"] = None


class ContextGraph:

    def __init__(self, context_list_path: str, symbol_table: Dict[str, int], bpe_model: Optional[str] = None,
                 context_score: float = 6.0):
        self.context_score = context_score
        self.context_list = tokenize(context_list_path, symbol_table, bpe_model)
        self.num_nodes = 0
        self.root = ContextState(id=0, token=-1, token_score=0, node_score=0, output_score=0, is_end=False)
        self.root.fail = self.root
        self._nodes: List[ContextState] = [self.root]
        self._tables: Dict[str, Dict[str, torch.Tensor]] = {}
        self.build_graph(self.context_list)

    def build_graph(self, token_ids: List[List[int]]):
        """The trie (a node's is_end / output_score are fixed when it is created), then the fail and output arcs."""
        for phrase in token_ids:
            node = self.root
            for i, tok in enumerate(phrase):
                child = node.next.get(tok)
                if child is None:
                    self.num_nodes += 1
                    end = i == len(phrase) - 1
                    acc = node.node_score + self.context_score
                    child = ContextState(id=self.num_nodes, token=tok, token_score=self.context_score, node_score=acc,
                                         output_score=acc if end else 0, is_end=end)
                    node.next[tok] = child
                    self._nodes.append(child)
                node = child
        self._fill_fail_output()
        self._tables.clear()

    def _fill_fail_output(self):
        """Breadth first, so a node's fail target (always shallower) is complete before the node is visited."""
        queue = deque()
        for child in self.root.next.values():
            child.fail = self.root
            queue.append(child)
        while queue:
            cur = queue.popleft()
            for tok, child in cur.next.items():
                f = cur.fail
                if tok in f.next:
                    f = f.next[tok]
                else:
                    f = f.fail
                    while tok not in f.next:
                        f = f.fail
                        if f.token == -1:
                            break
                    if tok in f.next:
                        f = f.next[tok]
                child.fail = f
                out = child.fail
                while not out.is_end:
                    out = out.fail
                    if out.token == -1:
                        out = None
                        break
                child.output = out
                child.output_score += 0 if out is None else out.output_score
                queue.append(child)

    def forward_one_step(self, state: ContextState, token: int) -> Tuple[float, ContextState]:
        """(bonus, next state) for `token` after `state`: a matching child earns its token_score; otherwise follow fail
        arcs to the longest suffix that continues with `token` (or the root), and the bonus is the difference of the
        accumulated scores -- negative when a partial match is abandoned.  Plus the output score of the new state."""
        if token in state.next:
            node = state.next[token]
            score = node.token_score
        else:
            node = state.fail
            while token not in node.next:
                node = node.fail
                if node.token == -1:
                    break
            if token in node.next:
                node = node.next[token]
            score = node.node_score - state.node_score
        return (score + node.output_score, node)

    def finalize(self, state: ContextState) -> Tuple[float, ContextState]:
        """At the end of a hypothesis: the score of an implicit fail arc to the root, -node_score (also for a state that
        ends a phrase), and the root."""
        return (-state.node_score, self.root)

    def device_tables(self, device) -> Dict[str, torch.Tensor]:
        """The graph as flat tensors on `device` (cached per device; node i is the node of id i, the root is 0):
        child_begin (N+1) / child_token (E) / child_node (E) int32, each node's children sorted by token; fail (N) int32;
        token_score / node_score / output_score (N) float64."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:      # "cuda" and "cuda:<current>" share one entry
            device = torch.device("cuda", torch.cuda.current_device())
        key = str(device)
        if key not in self._tables:
            nodes = self._nodes
            begin, ctok, cnode = [0], [], []
            for n in nodes:
                for tok in sorted(n.next):
                    ctok.append(tok)
                    cnode.append(n.next[tok].id)
                begin.append(len(ctok))
            if not ctok:                       # no phrase: keep the child arrays non-empty (never read)
                ctok, cnode = [-1], [0]
            i32 = dict(dtype=torch.int32)
            f64 = dict(dtype=torch.float64)
            host = dict(child_begin=torch.tensor(begin, **i32), child_token=torch.tensor(ctok, **i32),
                        child_node=torch.tensor(cnode, **i32), fail=torch.tensor([n.fail.id for n in nodes], **i32),
                        token_score=torch.tensor([float(n.token_score) for n in nodes], **f64),
                        node_score=torch.tensor([float(n.node_score) for n in nodes], **f64),
                        output_score=torch.tensor([float(n.output_score) for n in nodes], **f64))
            self._tables[key] = {k: v.to(device) for k, v in host.items()}
        return self._tables[key]
