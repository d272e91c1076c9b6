// CTC prefix beam search on the GPU (C ABI: include/pafc_search.h: pafc_ctc_prefix_beam_search[_ex]).
//
// Reference: ctc_prefix_beam_search, wenet/transformer/search.py:124-248, with its context graph and time stamps: per
// frame the top-`beam` tokens extend / repeat / blank the current prefixes, equal prefixes merge by log-add, the best
// `beam` survive.  There it is a Python loop per utterance, per frame, per candidate with .item() syncs; here one wave
// per utterance walks the frames on the device and only the n-best lists come back.
//
// Prefixes are nodes of a per-utterance trie (parent, token); a frame's candidates are "slots":
//   S_b        the beam member b itself (blank, or its last token again)           -> one slot per member
//   E_{b,r}    member b extended by the r-th best token u                          -> unless that prefix already IS a
//              member Q (parent(Q) = b, token(Q) = u): then the contribution goes to S_Q (the reference's dict key)
// Every slot receives at most three contributions (one blank-ending, one or two non-blank-ending), so each slot GATHERS
// its own instead of the reference's sequential scatter: log-add of two numbers is commutative, a first log-add with
// -inf returns the other argument exactly, hence the values are those of the reference's loop.  Ties of the total score
// are broken like Python's stable sort over the dict's insertion order: the position of the slot's first touch in
// the reference's (token rank, member rank) loop nest.  Arithmetic is float64 like the reference's Python floats; exp
// and log come from the device math library, so scores agree to the last few ulps, token lists exactly.
//
// The kernel is templated on <CTX, TIMES>; <false, false> is pafc_ctc_prefix_beam_search, unchanged.
// TIMES: per slot the viterbi scores v_s / v_ns and two frame lists.  Their updates depend on the order of a slot's
//   contributions (the reference assigns, it does not log-add), so a slot sorts its (at most three) contributions by
//   first-touch key and applies the reference's rules in that order -- including its quirks: the *uu -> *u branch never
//   updates v_ns (the reference assigns a misspelt attribute), and cur_token_prob lives for one frame only.  Frame lists
//   are persistent linked lists (frame, previous node) in the workspace: times_s copies a handle, an append creates
//   (t, handle), "replace the last frame" creates (t, prev(handle)); a slot records the pending operation and only the
//   survivors of a frame create their node, at the same (t, rank) index as the token trie (node 0 = the empty list).
// CTX: per slot the context graph node and the accumulated bonus.  A prefix's context depends only on its tokens (its
//   first contributor sets it: blank and repeat copy the member's, an extension steps the graph), so an S slot copies its
//   member's and an E slot runs forward_one_step (binary search among the node's children, then fail arcs).  The prune
//   ranks on score + bonus; the acoustic score is what the next frame extends.  After the last frame the bonus is
//   replaced by -node_score (the reference's finalize), and the order is not revisited.
#include "pafc_common.h"
#include "../../include/pafc_search.h"

namespace pafc {
namespace {

constexpr int MAXB = 16;                   // beam size and top-k limit
constexpr int NSLOT = MAXB + MAXB * MAXB;  // S slots then E slots
constexpr double NEG_INF = -__builtin_huge_val();

__device__ __forceinline__ double log_add2(double a, double b) {
    if (a == NEG_INF && b == NEG_INF) return NEG_INF;
    const double m = a > b ? a : b;
    return m + log(exp(a - m) + exp(b - m));
}

struct Graph {
    int num_nodes;
    const int32_t *child_begin, *child_token, *child_node, *fail;
    const double *token_score, *node_score, *output_score;
};

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

struct BeamParams {
    int T, K, beam, blank;
    const float *top_logp;     // (B, T, K)
    const int32_t *top_idx;    // (B, T, K)
    const int64_t *lens;       // (B) or null
    int32_t *pool_parent;      // (B, 1 + T * beam)
    int32_t *pool_token;       // (B, 1 + T * beam)
    int32_t *out_tokens;       // (B, beam, T)
    int32_t *out_len;          // (B, beam)   -1 for unused entries
    double *out_score;         // (B, beam)
    int32_t *time_frame;       // (B, 1 + T * beam)  frame lists: node 0 = empty list   [TIMES]
    int32_t *time_prev;        // (B, 1 + T * beam)
    int32_t *out_times;        // (B, beam, T): frames of the viterbi path, then -1     [TIMES]
    Graph g;                   //                                                       [CTX]
};

template <bool CTX, bool TIMES>
__global__ __launch_bounds__(64) void ctc_prefix_beam_kernel(const BeamParams p) {
    __shared__ double c_s[MAXB], c_ns[MAXB], c_sc[MAXB];          // current beam: blank-ending, non-blank-ending, total
    __shared__ int c_node[MAXB], c_last[MAXB], c_parent[MAXB];
    __shared__ double s_s[NSLOT], s_ns[NSLOT], s_tot[NSLOT];
    __shared__ int s_order[NSLOT], s_node[NSLOT], s_tok[NSLOT], s_par[NSLOT];
    __shared__ int tok[MAXB];
    __shared__ double lp[MAXB];
    __shared__ int n_node[MAXB], n_last[MAXB], n_parent[MAXB];              // next beam staging
    __shared__ double n_bs[MAXB], n_bns[MAXB], n_bsc[MAXB];
    __shared__ int s_nb;
    // TIMES: viterbi scores and frame-list handles of the members / slots / next members
    __shared__ double c_vs[MAXB], c_vns[MAXB], s_vs[NSLOT], s_vns[NSLOT], n_vs[MAXB], n_vns[MAXB];
    __shared__ int c_ts[MAXB], c_tns[MAXB], s_ts[NSLOT], s_top[NSLOT], s_tbase[NSLOT], n_ts[MAXB], n_tns[MAXB];
    // CTX: context node and bonus; s_ac = the acoustic score of a slot (s_tot adds the bonus)
    __shared__ int c_ctx[MAXB], s_ctx[NSLOT], n_ctx[MAXB];
    __shared__ double c_cs[MAXB], s_cs[NSLOT], n_cs[MAXB], s_ac[NSLOT];

    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = p.lens ? (int)min((int64_t)p.T, p.lens[b]) : p.T;
    const int K = p.K, beam = p.beam;
    const long pool_stride = 1 + (long)p.T * beam;
    int32_t *pparent = p.pool_parent + b * pool_stride, *ptoken = p.pool_token + b * pool_stride;
    int32_t *tframe = TIMES ? p.time_frame + b * pool_stride : nullptr, *tprev = TIMES ? p.time_prev + b * pool_stride : nullptr;
    constexpr int UNTOUCHED = 0x7fffffff;

    if (lane == 0) {
        c_node[0] = 0; c_last[0] = -1; c_parent[0] = -1; c_s[0] = 0.0; c_ns[0] = NEG_INF; c_sc[0] = 0.0;
        pparent[0] = -1; ptoken[0] = -1;
        s_nb = 1;
        if constexpr (TIMES) { c_vs[0] = 0.0; c_vns[0] = 0.0; c_ts[0] = 0; c_tns[0] = 0; tframe[0] = -1; tprev[0] = 0; }
        if constexpr (CTX) { c_ctx[0] = 0; c_cs[0] = 0.0; }
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int nb = s_nb;
        if (lane < K) {
            tok[lane] = p.top_idx[((long)b * p.T + t) * K + lane];
            lp[lane] = (double)p.top_logp[((long)b * p.T + t) * K + lane];
        }
        __syncthreads();
        // rank of the blank token in the top-k (or -1)
        int rblank = -1;
        for (int r = 0; r < K; ++r) if (tok[r] == p.blank) rblank = r;

        // ---- S slots: lane m < nb gathers what lands on member m itself ---------------------------------------
        if (lane < nb) {
            const int m = lane;
            double s = NEG_INF, ns = NEG_INF;
            int order = UNTOUCHED;
            if (rblank >= 0) { s = c_sc[m] + lp[rblank]; order = min(order, (rblank * nb + m) * 2); }
            int rq = -1;                                            // rank of the member's own last token
            if (c_last[m] >= 0) for (int r = 0; r < K; ++r) if (tok[r] == c_last[m]) rq = r;
            if (rq >= 0 && c_last[m] != p.blank) {
                ns = c_ns[m] + lp[rq];                             // *uu -> *u
                order = min(order, (rq * nb + m) * 2);
                // the same prefix reached by extending its parent, if the parent is in the beam too
                for (int pb = 0; pb < nb; ++pb) {
                    if (c_node[pb] == c_parent[m]) {
                        const bool rep = c_last[pb] == c_last[m];   // parent ends in the same token: only its blank path
                        ns = log_add2(ns, (rep ? c_s[pb] : c_sc[pb]) + lp[rq]);
                        order = min(order, (rq * nb + pb) * 2 + (rep ? 1 : 0));
                    }
                }
            }
            s_s[m] = s; s_ns[m] = ns; s_order[m] = order; s_node[m] = c_node[m]; s_tok[m] = c_last[m]; s_par[m] = c_parent[m];
            if constexpr (TIMES) {
                // the contributions in the reference's loop order: 0 blank of m, 1 *uu -> *u of m, 2 *u-u -> *uu of
                // the parent, 3 extension of the parent
                int ko[3], kk[3], ks[3], nc = 0;
                if (rblank >= 0) { ko[nc] = (rblank * nb + m) * 2; kk[nc] = 0; ks[nc] = m; ++nc; }
                if (rq >= 0 && c_last[m] != p.blank) {
                    ko[nc] = (rq * nb + m) * 2; kk[nc] = 1; ks[nc] = m; ++nc;
                    for (int pb = 0; pb < nb; ++pb) {
                        if (c_node[pb] == c_parent[m]) {
                            const bool rep = c_last[pb] == c_last[m];
                            ko[nc] = (rq * nb + pb) * 2 + (rep ? 1 : 0); kk[nc] = rep ? 2 : 3; ks[nc] = pb; ++nc;
                        }
                    }
                }
                for (int i = 1; i < nc; ++i)
                    for (int j = i; j > 0 && ko[j - 1] > ko[j]; --j) {
                        int x = ko[j]; ko[j] = ko[j - 1]; ko[j - 1] = x;
                        x = kk[j]; kk[j] = kk[j - 1]; kk[j - 1] = x;
                        x = ks[j]; ks[j] = ks[j - 1]; ks[j - 1] = x;
                    }
                double vs = NEG_INF, vns = NEG_INF, ctp = NEG_INF;
                int ts = 0, top = T_NONE, tbase = 0;
                for (int i = 0; i < nc; ++i) {
                    const int q = ks[i];
                    const bool sbest = c_vs[q] > c_vns[q];
                    const double vit = sbest ? c_vs[q] : c_vns[q];
                    const int qtimes = sbest ? c_ts[q] : c_tns[q];
                    if (kk[i] == 0) {
                        vs = vit + lp[rblank]; ts = qtimes;
                    } else if (kk[i] == 1) {
                        const double prob = lp[rq];
                        if (vns < c_vns[q] + prob && ctp < prob) { ctp = prob; top = T_REPLACE; tbase = c_tns[q]; }
                    } else {
                        const double prob = lp[rq];
                        const double x = (kk[i] == 2 ? c_vs[q] : vit) + prob;
                        if (vns < x) { vns = x; ctp = prob; top = T_APPEND; tbase = kk[i] == 2 ? c_ts[q] : qtimes; }
                    }
                }
                s_vs[m] = vs; s_vns[m] = vns; s_ts[m] = ts; s_top[m] = top; s_tbase[m] = tbase;
            }
            if constexpr (CTX) { s_ctx[m] = c_ctx[m]; s_cs[m] = c_cs[m]; }
        } else if (lane < MAXB) {
            s_order[lane] = UNTOUCHED;
        }
        // ---- E slots: (member m, token rank r) -> a new prefix, unless it already is a member ---------------
        for (int e = lane; e < MAXB * MAXB; e += 64) {
            const int m = e / MAXB, r = e % MAXB;
            int order = UNTOUCHED;
            double ns = NEG_INF;
            double vns = NEG_INF, cs = 0.0;
            int top = T_NONE, tbase = 0, cn = 0;
            if (m < nb && r < K && tok[r] != p.blank) {
                bool is_member = false;
                for (int qm = 0; qm < nb; ++qm) is_member |= (c_parent[qm] == c_node[m] && c_last[qm] == tok[r]);
                if (!is_member) {
                    const bool rep = tok[r] == c_last[m];
                    ns = (rep ? c_s[m] : c_sc[m]) + lp[r];
                    order = (r * nb + m) * 2 + (rep ? 1 : 0);
                    if constexpr (TIMES) {        // the slot's only contribution: v_ns and the frame list of the path
                        const bool sbest = c_vs[m] > c_vns[m];
                        const double x = (rep ? c_vs[m] : (sbest ? c_vs[m] : c_vns[m])) + lp[r];
                        vns = NEG_INF; top = T_NONE; tbase = 0;
                        if (NEG_INF < x) { vns = x; top = T_APPEND; tbase = (rep || sbest) ? c_ts[m] : c_tns[m]; }
                    }
                    if constexpr (CTX) { int nx; const double sc = ctx_step(p.g, c_ctx[m], tok[r], nx); cn = nx; cs = c_cs[m] + sc; }
                }
            }
            const int si = MAXB + e;
            if constexpr (TIMES) { s_vs[si] = NEG_INF; s_vns[si] = vns; s_ts[si] = 0; s_top[si] = top; s_tbase[si] = tbase; }
            if constexpr (CTX) { s_ctx[si] = cn; s_cs[si] = cs; }
            s_s[si] = NEG_INF; s_ns[si] = ns; s_order[si] = order; s_node[si] = -1;
            s_tok[si] = (r < K) ? tok[r] : -1; s_par[si] = (m < nb) ? c_node[m] : -1;
        }
        __syncthreads();
        for (int i = lane; i < NSLOT; i += 64) {
            if constexpr (CTX) {                // rank on score() + context_score, keep score() for the next frame
                const double ac = s_order[i] == UNTOUCHED ? NEG_INF : log_add2(s_s[i], s_ns[i]);
                s_ac[i] = ac;
                s_tot[i] = s_order[i] == UNTOUCHED ? NEG_INF : ac + s_cs[i];
            } else {
                s_tot[i] = s_order[i] == UNTOUCHED ? NEG_INF : log_add2(s_s[i], s_ns[i]);
            }
        }
        __syncthreads();
        // ---- rank the touched slots: score descending, first-touch order ascending -----------------------------
        for (int i = lane; i < NSLOT; i += 64) {
            if (s_order[i] == UNTOUCHED) continue;
            int rank = 0;
            const double sc = s_tot[i];
            const int oi = s_order[i];
            for (int j = 0; j < NSLOT; ++j) {
                if (s_order[j] == UNTOUCHED) continue;
                rank += (s_tot[j] > sc || (s_tot[j] == sc && s_order[j] < oi)) ? 1 : 0;
            }
            if (rank < beam) {
                int node = s_node[i];
                if (node < 0) {                                     // a new prefix: its node id is fixed by (t, rank)
                    node = 1 + t * beam + rank;
                    pparent[node] = s_par[i];
                    ptoken[node] = s_tok[i];
                }
                n_node[rank] = node; n_last[rank] = s_tok[i]; n_parent[rank] = s_par[i];
                n_bs[rank] = s_s[i]; n_bns[rank] = s_ns[i]; n_bsc[rank] = CTX ? s_ac[i] : sc;
                if constexpr (TIMES) {
                    int tns = 0;
                    if (s_top[i] != T_NONE) {                      // a survivor materialises its pending frame list
                        tns = 1 + t * beam + rank;
                        tframe[tns] = t;
                        tprev[tns] = s_top[i] == T_APPEND ? s_tbase[i] : tprev[s_tbase[i]];
                    }
                    n_vs[rank] = s_vs[i]; n_vns[rank] = s_vns[i]; n_ts[rank] = s_ts[i]; n_tns[rank] = tns;
                }
                if constexpr (CTX) { n_ctx[rank] = s_ctx[i]; n_cs[rank] = s_cs[i]; }
            }
        }
        __syncthreads();
        if (lane == 0) {
            int cnt = 0;
            for (int i = 0; i < NSLOT; ++i) cnt += s_order[i] != UNTOUCHED;
            s_nb = min(cnt, beam);
        }
        __syncthreads();
        if (lane < s_nb) {
            c_node[lane] = n_node[lane]; c_last[lane] = n_last[lane]; c_parent[lane] = n_parent[lane];
            c_s[lane] = n_bs[lane]; c_ns[lane] = n_bns[lane]; c_sc[lane] = n_bsc[lane];
            if constexpr (TIMES) { c_vs[lane] = n_vs[lane]; c_vns[lane] = n_vns[lane]; c_ts[lane] = n_ts[lane]; c_tns[lane] = n_tns[lane]; }
            if constexpr (CTX) { c_ctx[lane] = n_ctx[lane]; c_cs[lane] = n_cs[lane]; }
        }
        __syncthreads();
    }

    // ---- n-best lists: walk the trie back from each surviving node ------------------------------------------
    const int nb = s_nb;
    if (lane < beam) {
        int32_t *ot = p.out_tokens + ((long)b * beam + lane) * p.T;
        if (lane < nb) {
            int len = 0;
            for (int n = c_node[lane]; n > 0; n = pparent[n]) ++len;
            int pos = len;
            for (int n = c_node[lane]; n > 0; n = pparent[n]) ot[--pos] = ptoken[n];
            p.out_len[b * beam + lane] = len;
            if constexpr (CTX) p.out_score[b * beam + lane] = c_sc[lane] + (-p.g.node_score[c_ctx[lane]]);   // finalize
            else p.out_score[b * beam + lane] = c_sc[lane];
        } else {
            p.out_len[b * beam + lane] = -1;
            p.out_score[b * beam + lane] = NEG_INF;
        }
        if constexpr (TIMES) {
            int32_t *tt = p.out_times + ((long)b * beam + lane) * p.T;
            int len = 0;
            if (lane < nb) {
                const int h = c_vs[lane] > c_vns[lane] ? c_ts[lane] : c_tns[lane];
                for (int n = h; n > 0; n = tprev[n]) ++len;
                int pos = len;
                for (int n = h; n > 0; n = tprev[n]) tt[--pos] = tframe[n];
            }
            for (int i = len; i < p.T; ++i) tt[i] = -1;
        }
    }
}

}  // namespace
}  // namespace pafc

extern "C" size_t pafc_ctc_prefix_beam_workspace_bytes(int B, int T, int beam) {
    if (B <= 0 || T <= 0 || beam <= 0) return 0;
    return (size_t)2 * B * (1 + (size_t)T * beam) * sizeof(int32_t);
}

extern "C" int pafc_ctc_prefix_beam_search(int B, int T, int K, const float *top_logp, const int32_t *top_idx,
                                           const int64_t *lens, int beam, int blank_id, int32_t *out_tokens,
                                           int32_t *out_len, double *out_score, void *workspace, size_t workspace_bytes,
                                           pafc_stream_t stream) {
    if (!top_logp || !top_idx || !out_tokens || !out_len || !out_score || !workspace) return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || T <= 0 || K <= 0 || beam <= 0 || blank_id < 0) return PAFC_ERR_BAD_DIMS;
    if (K > pafc::MAXB || beam > pafc::MAXB) return PAFC_ERR_UNSUPPORTED;
    if (workspace_bytes < pafc_ctc_prefix_beam_workspace_bytes(B, T, beam)) return PAFC_ERR_WORKSPACE;
    pafc::BeamParams p{};
    p.T = T; p.K = K; p.beam = beam; p.blank = blank_id;
    p.top_logp = top_logp; p.top_idx = top_idx; p.lens = lens;
    p.pool_parent = (int32_t *)workspace;
    p.pool_token = p.pool_parent + (size_t)B * (1 + (size_t)T * beam);
    p.out_tokens = out_tokens; p.out_len = out_len; p.out_score = out_score;
    hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<false, false>), dim3(B), dim3(64), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" size_t pafc_ctc_prefix_beam_ex_workspace_bytes(int B, int T, int beam) {
    if (B <= 0 || T <= 0 || beam <= 0) return 0;
    return (size_t)4 * B * (1 + (size_t)T * beam) * sizeof(int32_t);     // token trie + frame lists
}

extern "C" int pafc_ctc_prefix_beam_search_ex(int B, int T, int K, const float *top_logp, const int32_t *top_idx,
                                              const int64_t *lens, int beam, int blank_id,
                                              const pafc_ctc_context_graph *graph, int32_t *out_tokens, int32_t *out_len,
                                              double *out_score, int32_t *out_times, void *workspace,
                                              size_t workspace_bytes, pafc_stream_t stream) {
    if (!top_logp || !top_idx || !out_tokens || !out_len || !out_score || !workspace) return PAFC_ERR_NULL_POINTER;
    if (graph && (!graph->child_begin || !graph->child_token || !graph->child_node || !graph->fail ||
                  !graph->token_score || !graph->node_score || !graph->output_score))
        return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || T <= 0 || K <= 0 || beam <= 0 || blank_id < 0) return PAFC_ERR_BAD_DIMS;
    if (graph && graph->num_nodes < 1) return PAFC_ERR_BAD_DIMS;
    if (K > pafc::MAXB || beam > pafc::MAXB) return PAFC_ERR_UNSUPPORTED;
    if (workspace_bytes < pafc_ctc_prefix_beam_ex_workspace_bytes(B, T, beam)) return PAFC_ERR_WORKSPACE;
    pafc::BeamParams p{};
    const size_t pool = (size_t)B * (1 + (size_t)T * beam);
    p.T = T; p.K = K; p.beam = beam; p.blank = blank_id;
    p.top_logp = top_logp; p.top_idx = top_idx; p.lens = lens;
    p.pool_parent = (int32_t *)workspace;
    p.pool_token = p.pool_parent + pool;
    p.time_frame = p.pool_token + pool;
    p.time_prev = p.time_frame + pool;
    p.out_tokens = out_tokens; p.out_len = out_len; p.out_score = out_score; p.out_times = out_times;
    if (graph) {
        p.g.num_nodes = graph->num_nodes;
        p.g.child_begin = graph->child_begin; p.g.child_token = graph->child_token; p.g.child_node = graph->child_node;
        p.g.fail = graph->fail;
        p.g.token_score = graph->token_score; p.g.node_score = graph->node_score; p.g.output_score = graph->output_score;
    }
    const dim3 grid(B), block(64);
    hipStream_t s = (hipStream_t)stream;
    if (graph && out_times) hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<true, true>), grid, block, 0, s, p);
    else if (graph) hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<true, false>), grid, block, 0, s, p);
    else if (out_times) hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<false, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<false, false>), grid, block, 0, s, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
