// Bookkeeping of the CTC-fused RNN-T prefix beam search on the GPU (C ABI: include/pafc_search.h: pafc_rnnt_beam_*).
//
// Reference: PrefixBeamSearch.prefix_beam_search_decode_batch, wenet/transducer/search/prefix_beam_search.py:428-574.  Per
// frame and utterance the reference sorts the beam x beam candidates (beam score + fused log-prob of the top tokens),
// walks them best first, merges candidates that spell the same hypothesis with log_add, stops as soon as `beam`
// distinct hypotheses are collected, sorts those and keeps them -- reading every candidate with .item().  Here the
// predictor / joint / fusion / top-k stay batched framework ops on fixed (B x beam) slots and this kernel does the walk
// on the device: no host synchronisation between frames.  It also emits, per slot, which LSTM state the survivor
// carries (old state of its parent beam for a blank, new state for an emitted token) and the token to feed next.
//
// Hypotheses are nodes of a per-utterance trie (as in ctc_beam.hip): a blank keeps the parent's node, a token either
// lands on a beam member that already spells parent + token or becomes a new node.  Scores are float64 like the
// reference's Python floats; each candidate's score is float32(beam score) + float32 log-prob added in float32, the
// rounding point of the reference (`torch.tensor(scores) + top_k_logp`).
#include "rnnt_beam_common.h"

namespace pafc {
namespace {

__global__ void rnnt_beam_init_kernel(void *ws, int B, int T, int beam, int blank, int64_t *next_idx, int64_t *last_tok) {
    const RnntState s = carve(ws, B, T, beam);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * beam) return;
    const int b = i / beam, m = i % beam;
    s.node[i] = 0; s.parent[i] = -1; s.last[i] = blank;
    s.score[i] = m == 0 ? 0.0 : NEG_INF;
    next_idx[i] = i;
    last_tok[i] = blank;
    if (m == 0) {
        s.nb[b] = 1;
        s.pool_parent[(size_t)b * (1 + (size_t)T * beam)] = -1;
        s.pool_token[(size_t)b * (1 + (size_t)T * beam)] = blank;
    }
}

__global__ __launch_bounds__(64) void rnnt_beam_step_kernel(void *ws, int B, int T, int beam, int blank, int t_host,
                                                            const int64_t *t_dev, const int64_t *lens,
                                                            const float *top_val, const int64_t *top_idx,
                                                            int64_t *next_idx, int64_t *last_tok) {
    // the frame index comes from device memory when the frame body is replayed from a captured graph
    const int t = t_dev != nullptr ? (int)*t_dev : t_host;

    const RnntState s = carve(ws, B, T, beam);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int base = b * beam;
    if (t >= T || (lens != nullptr && t >= lens[b])) {   // finished utterance: every slot keeps its state and its beam
        if (lane < beam) next_idx[base + lane] = base + lane;
        return;
    }
#include "rnnt_beam_frame.inc"
}

__global__ __launch_bounds__(64) void rnnt_beam_finish_kernel(void *ws, int B, int T, int beam, int32_t *out_tokens,
                                                              int32_t *out_len, double *out_score) {
    const RnntState s = carve(ws, B, T, beam);
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane >= beam) return;
    const size_t pstride = 1 + (size_t)T * beam;
    const int32_t *pp = s.pool_parent + b * pstride, *pt = s.pool_token + b * pstride;
    int32_t *ot = out_tokens + ((size_t)b * beam + lane) * T;
    if (lane < s.nb[b]) {
        out_len[b * beam + lane] = trie_list_back(s.node[b * beam + lane], pp, pt, ot, T);
        out_score[b * beam + lane] = s.score[b * beam + lane];
    } else {
        out_len[b * beam + lane] = -1;
        out_score[b * beam + lane] = NEG_INF;
    }
}

}  // namespace
}  // namespace pafc

extern "C" size_t pafc_rnnt_beam_workspace_bytes(int B, int T, int beam) {
    if (B <= 0 || T <= 0 || beam <= 0) return 0;
    return pafc::rnnt_state_bytes(B, T, beam);
}

static int rnnt_check(int B, int T, int beam, const void *ws, size_t ws_bytes) {
    if (!ws) return PAFC_ERR_NULL_POINTER;
    if (const int rc = pafc::beam_dims_check(B, T, beam)) return rc;
    if (ws_bytes < pafc_rnnt_beam_workspace_bytes(B, T, beam)) return PAFC_ERR_WORKSPACE;
    return PAFC_OK;
}

extern "C" int pafc_rnnt_beam_init(int B, int T, int beam, int blank_id, void *workspace, size_t workspace_bytes,
                                   int64_t *next_idx, int64_t *last_tok, pafc_stream_t stream) {
    const int rc = rnnt_check(B, T, beam, workspace, workspace_bytes);
    if (rc) return rc;
    if (!next_idx || !last_tok) return PAFC_ERR_NULL_POINTER;
    hipLaunchKernelGGL(pafc::rnnt_beam_init_kernel, dim3((B * beam + 255) / 256), dim3(256), 0, (hipStream_t)stream, workspace,
                       B, T, beam, blank_id, next_idx, last_tok);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_rnnt_beam_step(int B, int T, int beam, int blank_id, int t, const int64_t *t_dev, const int64_t *lens,
                                   const float *top_val, const int64_t *top_idx, void *workspace, size_t workspace_bytes,
                                   int64_t *next_idx, int64_t *last_tok, pafc_stream_t stream) {
    const int rc = rnnt_check(B, T, beam, workspace, workspace_bytes);
    if (rc) return rc;
    if (!top_val || !top_idx || !next_idx || !last_tok) return PAFC_ERR_NULL_POINTER;
    if (!t_dev && (t < 0 || t >= T)) return PAFC_ERR_BAD_DIMS;
    hipLaunchKernelGGL(pafc::rnnt_beam_step_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, workspace, B, T, beam, blank_id, t,
                       t_dev, lens, top_val, top_idx, next_idx, last_tok);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_rnnt_beam_finish(int B, int T, int beam, void *workspace, size_t workspace_bytes, int32_t *out_tokens,
                                     int32_t *out_len, double *out_score, pafc_stream_t stream) {
    const int rc = rnnt_check(B, T, beam, workspace, workspace_bytes);
    if (rc) return rc;
    if (!out_tokens || !out_len || !out_score) return PAFC_ERR_NULL_POINTER;
    hipLaunchKernelGGL(pafc::rnnt_beam_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, workspace, B, T, beam, out_tokens,
                       out_len, out_score);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
