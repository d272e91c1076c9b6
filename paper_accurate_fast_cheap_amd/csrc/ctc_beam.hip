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
// The body of the frame loop is ctc_beam_frame.inc and its LDS arrays ctc_beam_lds.inc: the streaming kernel
// (ctc_beam_stream.hip) includes the same text, so a stream of chunks does this kernel's arithmetic.
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
#include "ctc_beam_common.h"

namespace pafc {
namespace {

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
#include "ctc_beam_lds.inc"

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

    constexpr bool STREAM = false;      // (the streaming kernel also carries the members' token counts)
    for (int t = 0; t < T; ++t) {
        const int tin = t;
#include "ctc_beam_frame.inc"
    }

    // ---- n-best lists: walk the trie back from each surviving node ------------------------------------------
    const int nb = s_nb;
    if (lane < beam) {
        int32_t *ot = p.out_tokens + ((long)b * beam + lane) * p.T;
        if (lane < nb) {
            p.out_len[b * beam + lane] = trie_list_back(c_node[lane], pparent, ptoken, ot, p.T);
            if constexpr (CTX) p.out_score[b * beam + lane] = c_sc[lane] + (-p.g.node_score[c_ctx[lane]]);   // finalize
            else p.out_score[b * beam + lane] = c_sc[lane];
        } else {
            p.out_len[b * beam + lane] = -1;
            p.out_score[b * beam + lane] = NEG_INF;
        }
        if constexpr (TIMES) {
            int32_t *tt = p.out_times + ((long)b * beam + lane) * p.T;
            int len = 0;
            if (lane < nb) len = trie_list_back(c_vs[lane] > c_vns[lane] ? c_ts[lane] : c_tns[lane], tprev, tframe, tt, p.T);
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
    if (K > pafc::BEAM_MAX || beam > pafc::BEAM_MAX) return PAFC_ERR_UNSUPPORTED;
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
    if (graph && !pafc::graph_ok(graph)) return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || T <= 0 || K <= 0 || beam <= 0 || blank_id < 0) return PAFC_ERR_BAD_DIMS;
    if (graph && graph->num_nodes < 1) return PAFC_ERR_BAD_DIMS;
    if (K > pafc::BEAM_MAX || beam > pafc::BEAM_MAX) return PAFC_ERR_UNSUPPORTED;
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
    p.g = pafc::to_graph(graph);
    const dim3 grid(B), block(64);
    hipStream_t s = (hipStream_t)stream;
    if (graph && out_times) hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<true, true>), grid, block, 0, s, p);
    else if (graph) hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<true, false>), grid, block, 0, s, p);
    else if (out_times) hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<false, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((pafc::ctc_prefix_beam_kernel<false, false>), grid, block, 0, s, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
