// CTC-fused RNN-T prefix beam search chunk by chunk (C ABI: include/pafc_search.h: pafc_rnnt_beam_stream_*), and the
// in-place selection of the survivors' LSTM state (pafc_rnnt_beam_select_state).
//
// The offline search (rnnt_beam.hip) sizes its trie by the utterance's T, numbers nodes by utterance frame and starts
// every row at once.  Here the workspace begins with the same beam state, laid out for T = max_total_frames, followed per
// row by the frames consumed since the reset, the frames taken in the current chunk, an overflow flag, a mark that the row
// was reset, and per member its token count.  A step of chunk frame j runs, for every row with j < taken, the offline
// kernel's per-frame text (rnnt_beam_frame.inc) at the ABSOLUTE frame consumed[b]: a node created there by the survivor of
// rank r is 1 + consumed[b] * beam + r, as offline.  Loads and stores of float64 and int32 are exact, so after any cut of
// a row's frames into chunks the beam holds the bits the offline kernel holds after as many frames.  A feed that would
// take a row past max_total_frames takes nothing and raises the row's flag (kept until the reset), so no index beyond the
// pool is ever formed.
//
// drain reads the state and writes the n-best lists as if the stream ended here: trie_drain (beam_trie.h), which says what
// `committed` and `from` mean.  It needs each member's token count; the step carries it.
#include "rnnt_beam_common.h"

namespace pafc {
namespace {

constexpr int32_t RSTREAM_MAGIC = 0x524e5442;     // a row that was reset

struct RnntStreamRows {
    int32_t *consumed, *taken, *overflow, *magic;  // (B)
    int32_t *len;                                  // (B, beam) token count of each member
};

__host__ __device__ __forceinline__ size_t rows_offset(int B, int T, int beam) {
    return (rnnt_state_bytes(B, T, beam) + 7) / 8 * 8;
}

__host__ __device__ __forceinline__ RnntStreamRows carve_rows(void *ws, int B, int T, int beam) {
    RnntStreamRows x;
    int32_t *p = (int32_t *)((char *)ws + rows_offset(B, T, beam));
    x.consumed = p; p += B;
    x.taken = p; p += B;
    x.overflow = p; p += B;
    x.magic = p; p += B;
    x.len = p;
    return x;
}

inline size_t stream_bytes(int B, int T, int beam) {
    return rows_offset(B, T, beam) + sizeof(int32_t) * (4 * (size_t)B + (size_t)B * beam);
}

__global__ void rnnt_beam_stream_reset_kernel(void *ws, int B, int T, int beam, int blank, const int32_t *row_mask,
                                              int64_t *next_idx, int64_t *last_tok) {
    const RnntState s = carve(ws, B, T, beam);
    const RnntStreamRows x = carve_rows(ws, B, T, beam);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * beam) return;
    const int b = i / beam, m = i % beam;
    if (row_mask != nullptr && row_mask[b] == 0) return;
    s.node[i] = 0; s.parent[i] = -1; s.last[i] = blank;
    s.score[i] = m == 0 ? 0.0 : NEG_INF;
    x.len[i] = 0;
    next_idx[i] = i;
    last_tok[i] = blank;
    if (m == 0) {
        s.nb[b] = 1;
        s.pool_parent[(size_t)b * (1 + (size_t)T * beam)] = -1;
        s.pool_token[(size_t)b * (1 + (size_t)T * beam)] = blank;
        x.consumed[b] = 0; x.taken[b] = 0; x.overflow[b] = 0; x.magic[b] = RSTREAM_MAGIC;
    }
}

__global__ void rnnt_beam_stream_feed_kernel(void *ws, int B, int Tmax, int T, int beam, const int64_t *nframes) {
    const RnntStreamRows x = carve_rows(ws, B, T, beam);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n = clamp_frames(nframes[b], Tmax);
    int take = n;
    if (x.magic[b] != RSTREAM_MAGIC) {                      // never reset: nothing of this row can be trusted
        x.overflow[b] = 2;
        take = 0;
    } else if (n > 0 && (x.overflow[b] != 0 || x.consumed[b] < 0 || (int64_t)x.consumed[b] + n > T)) {
        x.overflow[b] = x.overflow[b] == 2 ? 2 : 1;
        take = 0;
    }
    x.taken[b] = take;
}

__global__ __launch_bounds__(64) void rnnt_beam_stream_step_kernel(void *ws, int B, int T, int beam, int blank, int j_host,
                                                                   const int64_t *j_dev, const float *top_val,
                                                                   const int64_t *top_idx, int64_t *next_idx,
                                                                   int64_t *last_tok) {
    // the chunk frame comes from device memory when the frame body is replayed from a captured graph
    const int64_t j = j_dev != nullptr ? *j_dev : (int64_t)j_host;
    __shared__ int m_len[BEAM_MAX];

    const RnntState s = carve(ws, B, T, beam);
    const RnntStreamRows x = carve_rows(ws, B, T, beam);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int base = b * beam;
    const int t = x.consumed[b];                           // the absolute frame: it numbers the new nodes
    if (x.magic[b] != RSTREAM_MAGIC || j < 0 || j >= x.taken[b] || t < 0 || t >= T) {
        if (lane < beam) next_idx[base + lane] = base + lane;     // no frame for this row: every slot keeps its state
        return;
    }
    if (lane < beam) m_len[lane] = x.len[base + lane];     // (read by others behind the barriers of the walk)
#include "rnnt_beam_frame.inc"
    if (lane < cnt) x.len[base + a_rank[lane]] = m_len[a_src[lane]] + a_new[lane];
    else if (lane < beam) x.len[base + lane] = 0;
    if (lane == 0) x.consumed[b] = t + 1;
}

struct RnntDrainParams {
    int B, T, beam, ld;
    void *ws;
    const int32_t *from;                          // (B) or null
    int32_t *out_tokens;                          // (B, beam, ld)
    int32_t *out_len;                             // (B, beam)
    double *out_score;                            // (B, beam)
    int32_t *out_count, *out_committed, *out_overflow;   // (B)
};

__global__ __launch_bounds__(64) void rnnt_beam_stream_drain_kernel(const RnntDrainParams p) {
    const int b = blockIdx.x, lane = threadIdx.x, beam = p.beam;
    const RnntState s = carve(p.ws, p.B, p.T, beam);
    const RnntStreamRows x = carve_rows(p.ws, p.B, p.T, beam);
    const bool valid = x.magic[b] == RSTREAM_MAGIC;
    const int nb = valid ? min(max(s.nb[b], 1), beam) : 0;
    const size_t pstride = 1 + (size_t)p.T * beam;
    const int32_t *pparent = s.pool_parent + b * pstride, *ptoken = s.pool_token + b * pstride;
    const bool active = lane < nb;
    const long o = (long)b * beam + lane;
    const int node = active ? s.node[o] : 0, len = active ? x.len[o] : 0;

    const int committed = trie_drain(active, node, len, nb, pparent, ptoken, p.from ? p.from[b] : 0, p.ld,
                                     active ? p.out_tokens + o * p.ld : nullptr);
    if (lane == 0) {
        p.out_count[b] = nb;
        p.out_committed[b] = committed;
        p.out_overflow[b] = valid ? x.overflow[b] : 2;
    }
    if (lane < beam) {                                            // per member: total token count and score
        p.out_len[o] = active ? len : -1;
        p.out_score[o] = active ? s.score[o] : NEG_INF;
    }
}

// h[l, i, :] = (next_idx[i] < n ? h : h_new)[l, next_idx[i] mod n, :] for both LSTM tensors, in place.  Block (b, y) owns
// utterance b; a thread owns one V-wide column of one layer of one tensor for ALL the utterance's slots: it loads the `beam`
// source vectors into registers, then stores them.  Sources are slots of the same utterance, so nobody else writes what a
// thread reads, and no barrier or LDS staging is needed.

template <typename V>
__global__ __launch_bounds__(256) void rnnt_beam_select_state_kernel(int L, int B, int beam, int rowv, V *h, V *c, const V *hn,
                                                                     const V *cn, const int64_t *next_idx) {
    const int b = blockIdx.x;
    const long n = (long)B * beam;
    const int per = L * rowv, items = 2 * per;
    for (int it = blockIdx.y * blockDim.x + threadIdx.x; it < items; it += gridDim.y * blockDim.x) {
        const int which = it / per, rem = it - which * per, l = rem / rowv, col = rem - l * rowv;
        V *dst = which ? c : h;
        const V *fresh = which ? cn : hn;
        V vals[BEAM_MAX];
#pragma unroll
        for (int i = 0; i < BEAM_MAX; ++i) {
            if (i < beam) {
                const long slot = (long)b * beam + i;
                long v = next_idx[slot];
                if (v < 0 || v >= 2 * n) v = slot;                // not an index of [old | new]: the slot keeps its state
                const V *from = v < n ? dst : fresh;
                const long r = v < n ? v : v - n;
                vals[i] = from[((long)l * n + r) * rowv + col];
            }
        }
#pragma unroll
        for (int i = 0; i < BEAM_MAX; ++i)
            if (i < beam) dst[((long)l * n + (long)b * beam + i) * rowv + col] = vals[i];
    }
}

template <typename V>
void launch_select(int L, int B, int beam, long row_bytes, void *h, void *c, const void *hn, const void *cn,
                   const int64_t *next_idx, hipStream_t stream) {
    const int rowv = (int)(row_bytes / (long)sizeof(V));
    const int items = 2 * L * rowv;
    const int gy = min(max((items + 255) / 256, 1), 8);
    hipLaunchKernelGGL((rnnt_beam_select_state_kernel<V>), dim3(B, gy), dim3(256), 0, stream, L, B, beam, rowv, (V *)h, (V *)c,
                       (const V *)hn, (const V *)cn, next_idx);
}

int stream_check(int B, int T, int beam, const void *ws, size_t ws_bytes) {
    if (!ws) return PAFC_ERR_NULL_POINTER;
    if (const int rc = beam_dims_check(B, T, beam)) return rc;
    if (ws_bytes < stream_bytes(B, T, beam)) return PAFC_ERR_WORKSPACE;
    return PAFC_OK;
}

}  // namespace
}  // namespace pafc

extern "C" size_t pafc_rnnt_beam_stream_workspace_bytes(int B, int max_total_frames, int beam) {
    if (pafc::beam_dims_check(B, max_total_frames, beam)) return 0;
    return pafc::stream_bytes(B, max_total_frames, beam);
}

extern "C" int pafc_rnnt_beam_stream_reset(int B, int max_total_frames, int beam, int blank_id, const int32_t *row_mask,
                                           void *workspace, size_t workspace_bytes, int64_t *next_idx, int64_t *last_tok,
                                           pafc_stream_t stream) {
    if (const int rc = pafc::stream_check(B, max_total_frames, beam, workspace, workspace_bytes)) return rc;
    if (!next_idx || !last_tok) return PAFC_ERR_NULL_POINTER;
    hipLaunchKernelGGL(pafc::rnnt_beam_stream_reset_kernel, dim3((B * beam + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       workspace, B, max_total_frames, beam, blank_id, row_mask, next_idx, last_tok);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_rnnt_beam_stream_feed(int B, int Tmax, int max_total_frames, int beam, const int64_t *nframes,
                                          void *workspace, size_t workspace_bytes, pafc_stream_t stream) {
    if (const int rc = pafc::stream_check(B, max_total_frames, beam, workspace, workspace_bytes)) return rc;
    if (!nframes) return PAFC_ERR_NULL_POINTER;
    if (Tmax <= 0) return PAFC_ERR_BAD_DIMS;
    hipLaunchKernelGGL(pafc::rnnt_beam_stream_feed_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, workspace, B,
                       Tmax, max_total_frames, beam, nframes);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_rnnt_beam_stream_step(int B, int Tmax, int max_total_frames, int beam, int blank_id, int j,
                                          const int64_t *j_dev, const float *top_val, const int64_t *top_idx, void *workspace,
                                          size_t workspace_bytes, int64_t *next_idx, int64_t *last_tok, pafc_stream_t stream) {
    if (const int rc = pafc::stream_check(B, max_total_frames, beam, workspace, workspace_bytes)) return rc;
    if (!top_val || !top_idx || !next_idx || !last_tok) return PAFC_ERR_NULL_POINTER;
    if (Tmax <= 0 || (!j_dev && (j < 0 || j >= Tmax))) return PAFC_ERR_BAD_DIMS;
    hipLaunchKernelGGL(pafc::rnnt_beam_stream_step_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, workspace, B,
                       max_total_frames, beam, blank_id, j, j_dev, top_val, top_idx, next_idx, last_tok);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_rnnt_beam_stream_drain(int B, int max_total_frames, int beam, const void *workspace, size_t workspace_bytes,
                                           const int32_t *from, int ld, int32_t *out_tokens, int32_t *out_len,
                                           double *out_score, int32_t *out_count, int32_t *out_committed,
                                           int32_t *out_overflow, pafc_stream_t stream) {
    if (const int rc = pafc::stream_check(B, max_total_frames, beam, workspace, workspace_bytes)) return rc;
    if (!out_len || !out_score || !out_count || !out_committed || !out_overflow) return PAFC_ERR_NULL_POINTER;
    if (ld > 0 && !out_tokens) return PAFC_ERR_NULL_POINTER;
    if (ld < 0) return PAFC_ERR_BAD_DIMS;
    pafc::RnntDrainParams p{};
    p.B = B; p.T = max_total_frames; p.beam = beam; p.ld = ld;
    p.ws = const_cast<void *>(workspace);
    p.from = from;
    p.out_tokens = out_tokens; p.out_len = out_len; p.out_score = out_score;
    p.out_count = out_count; p.out_committed = out_committed; p.out_overflow = out_overflow;
    hipLaunchKernelGGL(pafc::rnnt_beam_stream_drain_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_rnnt_beam_select_state(int dtype, int num_layers, int B, int beam, int hidden, void *h, void *c,
                                           const void *h_new, const void *c_new, const int64_t *next_idx, pafc_stream_t stream) {
    if (!h || !c || !h_new || !c_new || !next_idx) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (num_layers <= 0 || B <= 0 || beam <= 0 || hidden <= 0) return PAFC_ERR_BAD_DIMS;
    if (beam > pafc::BEAM_MAX) return PAFC_ERR_UNSUPPORTED;
    const long row_bytes = (long)hidden * (dtype == PAFC_F32 ? 4 : 2);
    if ((long)num_layers * row_bytes >= 0x3fffffffL) return PAFC_ERR_UNSUPPORTED;
    // the widest vector that divides a row and every base address
    const uintptr_t bits = (uintptr_t)h | (uintptr_t)c | (uintptr_t)h_new | (uintptr_t)c_new | (uintptr_t)row_bytes;
    hipStream_t s = (hipStream_t)stream;
    if (bits % 16 == 0) pafc::launch_select<pafc::u32x4>(num_layers, B, beam, row_bytes, h, c, h_new, c_new, next_idx, s);
    else if (bits % 8 == 0) pafc::launch_select<pafc::u32x2>(num_layers, B, beam, row_bytes, h, c, h_new, c_new, next_idx, s);
    else if (bits % 4 == 0) pafc::launch_select<uint32_t>(num_layers, B, beam, row_bytes, h, c, h_new, c_new, next_idx, s);
    else if (bits % 2 == 0) pafc::launch_select<uint16_t>(num_layers, B, beam, row_bytes, h, c, h_new, c_new, next_idx, s);
    else return PAFC_ERR_ALIGNMENT;
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
