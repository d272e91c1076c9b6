// CTC prefix beam search chunk by chunk (C ABI: include/pafc_search.h: pafc_ctc_beam_stream_*).
//
// The offline kernel (ctc_beam.hip) initialises its beam at frame 0, keeps it in LDS and writes n-best lists after the
// last frame.  Here the beam lives in the workspace between launches: a feed loads a row's beam into LDS, walks the
// chunk's frames with the offline kernel's per-frame body (the same text: ctc_beam_frame.inc) and stores the beam back.
// Loads and stores of float64 and int32 are exact, so after any cut of T frames into chunks the beam holds the bits
// the offline kernel holds after T frames.
//
// Workspace: B RowState records (padded to 256 bytes), then per row the pools of the offline kernel -- trie parent,
// trie token and, with times, frame-list frame and previous node -- of 1 + max_total_frames * beam int32 each.  A node
// created at absolute frame t by the survivor of rank r is 1 + t * beam + r in both numberings, as offline; node 0 is
// the empty prefix / the empty list.  A feed that would take a row past max_total_frames consumes nothing and raises
// the row's overflow flag (kept until the row is reset), so no index beyond the pool is ever formed.
//
// drain reads the state and writes the n-best lists as if the stream ended here: trie_drain (beam_trie.h), which says
// what `committed` and `from` mean; the finalize bonus goes to the returned score only.  It needs each member's token
// count; the feed carries it (c_len).
#include "ctc_beam_common.h"

namespace pafc {
namespace {

constexpr int32_t STATE_MAGIC = 0x43544253;      // a row that was reset

struct RowState {
    int64_t base;                                 // frames consumed since the reset
    int32_t nb, overflow, magic, beam;
    double s[BEAM_MAX], ns[BEAM_MAX], sc[BEAM_MAX], vs[BEAM_MAX], vns[BEAM_MAX], cs[BEAM_MAX];
    int32_t node[BEAM_MAX], last[BEAM_MAX], parent[BEAM_MAX], ts[BEAM_MAX], tns[BEAM_MAX], ctx[BEAM_MAX], len[BEAM_MAX];
};

struct Layout {
    size_t pool, state_bytes, total;              // nodes per row; bytes
};

__host__ __device__ inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }

inline Layout layout(int B, int max_total, int beam, int with_times) {
    Layout l;
    l.pool = 1 + (size_t)max_total * beam;
    l.state_bytes = align256((size_t)B * sizeof(RowState));
    l.total = l.state_bytes + (size_t)(with_times ? 4 : 2) * B * l.pool * sizeof(int32_t);
    return l;
}

struct StreamParams {
    int T, K, beam, blank, max_total;             // T = Tmax: frames per row of top_logp / top_idx
    const float *top_logp;                        // (B, Tmax, K)
    const int32_t *top_idx;                       // (B, Tmax, K)
    const int64_t *nframes;                       // (B)
    RowState *state;                              // (B)
    int32_t *pool_parent, *pool_token, *time_frame, *time_prev;   // (B, 1 + max_total * beam) each
    Graph g;
};

__global__ void ctc_beam_stream_reset_kernel(int B, int beam, long pool, int with_times, const int32_t *row_mask,
                                             RowState *state, int32_t *pool_parent, int32_t *pool_token,
                                             int32_t *time_frame, int32_t *time_prev) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (row_mask && row_mask[b] == 0)) return;
    RowState &r = state[b];
    r.base = 0; r.nb = 1; r.overflow = 0; r.magic = STATE_MAGIC; r.beam = beam;
    r.node[0] = 0; r.last[0] = -1; r.parent[0] = -1; r.s[0] = 0.0; r.ns[0] = NEG_INF; r.sc[0] = 0.0;
    r.vs[0] = 0.0; r.vns[0] = 0.0; r.ts[0] = 0; r.tns[0] = 0; r.ctx[0] = 0; r.cs[0] = 0.0; r.len[0] = 0;
    pool_parent[b * pool] = -1; pool_token[b * pool] = -1;
    if (with_times) { time_frame[b * pool] = -1; time_prev[b * pool] = 0; }
}

template <bool CTX, bool TIMES>
__global__ __launch_bounds__(64) void ctc_beam_stream_feed_kernel(const StreamParams p) {
#include "ctc_beam_lds.inc"

    const int b = blockIdx.x, lane = threadIdx.x;
    RowState &r = p.state[b];
    const int n = clamp_frames(p.nframes[b], p.T);
    if (n == 0) return;                                           // the row sits this feed out
    const int K = p.K, beam = p.beam;
    const int64_t base = r.base;
    if (r.magic != STATE_MAGIC || r.beam != beam || r.overflow != 0 || base < 0 || base + n > p.max_total) {
        if (lane == 0) r.overflow = (r.magic != STATE_MAGIC || r.beam != beam) ? 2 : 1;     // 2: the row was never reset
        return;
    }
    const long pool_stride = 1 + (long)p.max_total * beam;
    int32_t *pparent = p.pool_parent + b * pool_stride, *ptoken = p.pool_token + b * pool_stride;
    int32_t *tframe = TIMES ? p.time_frame + b * pool_stride : nullptr, *tprev = TIMES ? p.time_prev + b * pool_stride : nullptr;
    constexpr int UNTOUCHED = 0x7fffffff;
    constexpr bool STREAM = true;

    if (lane == 0) s_nb = min(max(r.nb, 1), beam);
    __syncthreads();
    if (lane < s_nb) {
        c_node[lane] = r.node[lane]; c_last[lane] = r.last[lane]; c_parent[lane] = r.parent[lane];
        c_s[lane] = r.s[lane]; c_ns[lane] = r.ns[lane]; c_sc[lane] = r.sc[lane]; c_len[lane] = r.len[lane];
        if constexpr (TIMES) { c_vs[lane] = r.vs[lane]; c_vns[lane] = r.vns[lane]; c_ts[lane] = r.ts[lane]; c_tns[lane] = r.tns[lane]; }
        if constexpr (CTX) { c_ctx[lane] = r.ctx[lane]; c_cs[lane] = r.cs[lane]; }
    }
    __syncthreads();

    for (int tin = 0; tin < n; ++tin) {
        const int t = (int)base + tin;
#include "ctc_beam_frame.inc"
    }

    if (lane < s_nb) {
        r.node[lane] = c_node[lane]; r.last[lane] = c_last[lane]; r.parent[lane] = c_parent[lane];
        r.s[lane] = c_s[lane]; r.ns[lane] = c_ns[lane]; r.sc[lane] = c_sc[lane]; r.len[lane] = c_len[lane];
        if constexpr (TIMES) { r.vs[lane] = c_vs[lane]; r.vns[lane] = c_vns[lane]; r.ts[lane] = c_ts[lane]; r.tns[lane] = c_tns[lane]; }
        if constexpr (CTX) { r.ctx[lane] = c_ctx[lane]; r.cs[lane] = c_cs[lane]; }
    }
    if (lane == 0) { r.nb = s_nb; r.base = base + n; }
}

struct DrainParams {
    int beam, max_total, ld, ld_times;
    const RowState *state;
    const int32_t *pool_parent, *pool_token, *time_frame, *time_prev;
    const int32_t *from;                          // (B) or null
    int32_t *out_tokens;                          // (B, beam, ld)
    int32_t *out_len;                             // (B, beam)
    double *out_score;                            // (B, beam)
    int32_t *out_count, *out_committed, *out_overflow;   // (B)
    int32_t *out_times, *out_ntimes;              // (B, beam, ld_times), (B, beam), or null
    const double *node_score;                     // the context graph's, or null
};

__global__ __launch_bounds__(64) void ctc_beam_stream_drain_kernel(const DrainParams p) {
    const int b = blockIdx.x, lane = threadIdx.x, beam = p.beam;
    const RowState &r = p.state[b];
    const bool valid = r.magic == STATE_MAGIC && r.beam == beam;
    const int nb = valid ? min(max(r.nb, 1), beam) : 0;
    const long pool_stride = 1 + (long)p.max_total * beam;
    const int32_t *pparent = p.pool_parent + b * pool_stride, *ptoken = p.pool_token + b * pool_stride;
    const bool active = lane < nb;
    const long o = (long)b * beam + lane;
    const int node = active ? r.node[lane] : 0, len = active ? r.len[lane] : 0;

    const int committed = trie_drain(active, node, len, nb, pparent, ptoken, p.from ? p.from[b] : 0, p.ld,
                                     active ? p.out_tokens + o * p.ld : nullptr);
    if (lane == 0) {
        p.out_count[b] = nb;
        p.out_committed[b] = committed;
        p.out_overflow[b] = valid ? r.overflow : 2;
    }
    if (lane < beam) {                                            // per member: total token count, score, frame list
        if (active) {
            p.out_len[o] = len;
            p.out_score[o] = p.node_score ? r.sc[lane] + (-p.node_score[r.ctx[lane]]) : r.sc[lane];     // finalize, on a copy
        } else {
            p.out_len[o] = -1;
            p.out_score[o] = NEG_INF;
        }
        if (p.out_ntimes) {
            int cnt = 0;
            if (active)
                cnt = trie_list_back(r.vs[lane] > r.vns[lane] ? r.ts[lane] : r.tns[lane], p.time_prev + b * pool_stride,
                                     p.time_frame + b * pool_stride, p.out_times + o * p.ld_times, p.ld_times);
            p.out_ntimes[o] = cnt;
        }
    }
}

}  // namespace
}  // namespace pafc

extern "C" size_t pafc_ctc_beam_stream_workspace_bytes(int B, int max_total_frames, int beam, int with_times) {
    if (pafc::beam_dims_check(B, max_total_frames, beam)) return 0;
    return pafc::layout(B, max_total_frames, beam, with_times).total;
}

namespace {
// the four pools behind the states
void pools(void *workspace, const pafc::Layout &l, int B, int with_times, int32_t *&parent, int32_t *&token, int32_t *&frame,
           int32_t *&prev) {
    parent = (int32_t *)((char *)workspace + l.state_bytes);
    token = parent + (size_t)B * l.pool;
    frame = with_times ? token + (size_t)B * l.pool : nullptr;
    prev = with_times ? frame + (size_t)B * l.pool : nullptr;
}
}  // namespace

extern "C" int pafc_ctc_beam_stream_reset(int B, int max_total_frames, int beam, int with_times, const int32_t *row_mask,
                                          void *workspace, size_t workspace_bytes, pafc_stream_t stream) {
    if (!workspace) return PAFC_ERR_NULL_POINTER;
    if (const int e = pafc::beam_dims_check(B, max_total_frames, beam)) return e;
    const pafc::Layout l = pafc::layout(B, max_total_frames, beam, with_times);
    if (workspace_bytes < l.total) return PAFC_ERR_WORKSPACE;
    int32_t *parent, *token, *frame, *prev;
    pools(workspace, l, B, with_times, parent, token, frame, prev);
    hipLaunchKernelGGL(pafc::ctc_beam_stream_reset_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, beam,
                       (long)l.pool, with_times, row_mask, (pafc::RowState *)workspace, parent, token, frame, prev);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_ctc_beam_stream_feed(int B, int Tmax, int K, const float *top_logp, const int32_t *top_idx,
                                         const int64_t *nframes, int max_total_frames, int beam, int blank_id,
                                         const pafc_ctc_context_graph *graph, int with_times, void *workspace,
                                         size_t workspace_bytes, pafc_stream_t stream) {
    if (!top_logp || !top_idx || !nframes || !workspace) return PAFC_ERR_NULL_POINTER;
    if (graph && !pafc::graph_ok(graph)) return PAFC_ERR_NULL_POINTER;
    if (Tmax <= 0 || K <= 0 || blank_id < 0) return PAFC_ERR_BAD_DIMS;
    if (B <= 0 || max_total_frames <= 0 || beam <= 0) return PAFC_ERR_BAD_DIMS;
    if (graph && graph->num_nodes < 1) return PAFC_ERR_BAD_DIMS;
    if (K > pafc::BEAM_MAX) return PAFC_ERR_UNSUPPORTED;
    if (const int e = pafc::beam_dims_check(B, max_total_frames, beam)) return e;
    const pafc::Layout l = pafc::layout(B, max_total_frames, beam, with_times);
    if (workspace_bytes < l.total) return PAFC_ERR_WORKSPACE;
    pafc::StreamParams p{};
    p.T = Tmax; p.K = K; p.beam = beam; p.blank = blank_id; p.max_total = max_total_frames;
    p.top_logp = top_logp; p.top_idx = top_idx; p.nframes = nframes;
    p.state = (pafc::RowState *)workspace;
    pools(workspace, l, B, with_times, p.pool_parent, p.pool_token, p.time_frame, p.time_prev);
    p.g = pafc::to_graph(graph);
    const dim3 grid(B), block(64);
    hipStream_t s = (hipStream_t)stream;
    if (graph && with_times) hipLaunchKernelGGL((pafc::ctc_beam_stream_feed_kernel<true, true>), grid, block, 0, s, p);
    else if (graph) hipLaunchKernelGGL((pafc::ctc_beam_stream_feed_kernel<true, false>), grid, block, 0, s, p);
    else if (with_times) hipLaunchKernelGGL((pafc::ctc_beam_stream_feed_kernel<false, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((pafc::ctc_beam_stream_feed_kernel<false, false>), grid, block, 0, s, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_ctc_beam_stream_drain(int B, int max_total_frames, int beam, const pafc_ctc_context_graph *graph,
                                          int with_times, const void *workspace, size_t workspace_bytes, const int32_t *from,
                                          int ld, int32_t *out_tokens, int32_t *out_len, double *out_score, int32_t *out_count,
                                          int32_t *out_committed, int32_t *out_overflow, int ld_times, int32_t *out_times,
                                          int32_t *out_ntimes, pafc_stream_t stream) {
    if (!workspace || !out_len || !out_score || !out_count || !out_committed || !out_overflow) return PAFC_ERR_NULL_POINTER;
    if (ld > 0 && !out_tokens) return PAFC_ERR_NULL_POINTER;
    if (ld_times > 0 && (!out_times || !out_ntimes)) return PAFC_ERR_NULL_POINTER;
    if (graph && !pafc::graph_ok(graph)) return PAFC_ERR_NULL_POINTER;
    if (ld < 0 || ld_times < 0) return PAFC_ERR_BAD_DIMS;
    if (graph && graph->num_nodes < 1) return PAFC_ERR_BAD_DIMS;
    if (const int e = pafc::beam_dims_check(B, max_total_frames, beam)) return e;
    if (out_ntimes && !with_times) return PAFC_ERR_UNSUPPORTED;           // the workspace holds no frame lists
    const pafc::Layout l = pafc::layout(B, max_total_frames, beam, with_times);
    if (workspace_bytes < l.total) return PAFC_ERR_WORKSPACE;
    pafc::DrainParams p{};
    p.beam = beam; p.max_total = max_total_frames; p.ld = ld; p.ld_times = ld_times;
    p.state = (const pafc::RowState *)workspace;
    int32_t *parent, *token, *frame, *prev;
    pools(const_cast<void *>(workspace), l, B, with_times, parent, token, frame, prev);
    p.pool_parent = parent; p.pool_token = token; p.time_frame = frame; p.time_prev = prev;
    p.from = from;
    p.out_tokens = out_tokens; p.out_len = out_len; p.out_score = out_score;
    p.out_count = out_count; p.out_committed = out_committed; p.out_overflow = out_overflow;
    p.out_times = out_times; p.out_ntimes = out_ntimes;
    p.node_score = graph ? graph->node_score : nullptr;
    hipLaunchKernelGGL(pafc::ctc_beam_stream_drain_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
