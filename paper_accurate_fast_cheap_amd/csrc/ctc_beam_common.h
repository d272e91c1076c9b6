// What the offline CTC prefix beam search (ctc_beam.hip) and the streaming one (ctc_beam_stream.hip) share outside the
// kernel body, beyond beam_trie.h: the slot count and the context graph with its walk.  The per-frame body itself is
// ctc_beam_frame.inc, its LDS arrays ctc_beam_lds.inc; both kernels include the same text, so their arithmetic cannot
// drift apart.
#ifndef PAFC_CTC_BEAM_COMMON_H
#define PAFC_CTC_BEAM_COMMON_H

#include "beam_trie.h"

namespace pafc {
namespace {

constexpr int NSLOT = BEAM_MAX + BEAM_MAX * BEAM_MAX;  // S slots then E slots

struct Graph {
    int num_nodes;
    const int32_t *child_begin, *child_token, *child_node, *fail;
    const double *token_score, *node_score, *output_score;
};

// every table of a caller's context graph is there
inline bool graph_ok(const pafc_ctc_context_graph *g) {
    return g->child_begin && g->child_token && g->child_node && g->fail && g->token_score && g->node_score && g->output_score;
}

// the kernels' copy of a caller's context graph; no graph: all zero
inline Graph to_graph(const pafc_ctc_context_graph *g) {
    Graph r{};
    if (g) {
        r.num_nodes = g->num_nodes;
        r.child_begin = g->child_begin; r.child_token = g->child_token; r.child_node = g->child_node; r.fail = g->fail;
        r.token_score = g->token_score; r.node_score = g->node_score; r.output_score = g->output_score;
    }
    return r;
}

// the child of `node` for token `tok`, or -1 (children sorted by token)
__device__ __forceinline__ int ctx_child(const Graph &g, int node, int tok) {
    int lo = g.child_begin[node], hi = g.child_begin[node + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int v = g.child_token[mid];
        if (v == tok) return g.child_node[mid];
        if (v < tok) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// ContextGraph.forward_one_step: the bonus for `tok` after `state`, and the next state
__device__ double ctx_step(const Graph &g, int state, int tok, int &next) {
    int n = ctx_child(g, state, tok);
    double sc;
    if (n >= 0) {
        sc = g.token_score[n];
    } else {
        n = g.fail[state];
        for (int guard = 0; guard < g.num_nodes; ++guard) {      // fail arcs strictly shorten the match
            const int c = ctx_child(g, n, tok);
            if (c >= 0) { n = c; break; }
            n = g.fail[n];
            if (n == 0) {
                const int r = ctx_child(g, 0, tok);
                if (r >= 0) n = r;
                break;
            }
        }
        sc = g.node_score[n] - g.node_score[state];
    }
    next = n;
    return sc + g.output_score[n];
}

enum { T_NONE = 0, T_APPEND = 1, T_REPLACE = 2 };   // pending operation on a slot's non-blank frame list

}  // namespace
}  // namespace pafc
#endif
