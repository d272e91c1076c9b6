/*
 * pafc_attn_search.h -- C ABI of the autoregressive beam search of the attention decoder (reference:
 * attention_beam_search, wenet/transformer/search.py:251-360).
 *
 * The reference re-projects K and V of the whole prefix in every layer and step, reorders every cache by index_select after
 * every step and forms the (B*N, V) log-softmax to keep N numbers of each row.  Here the R = B*N running rows (utterance b
 * owns the beam slots b*N .. b*N + N - 1) keep, per layer, a key/value cache whose rows are written once and never moved:
 *   cache: (P, R, 2*H*dk) elements, the row of beam slot r at position p being p*R + r: [k | v], head h the column slice
 *          [h*dk, (h+1)*dk) of each half;
 *   anc:   (2, R, P) int32, anc[p & 1][r][j] the beam slot within r's utterance (0 .. N-1) whose cache row holds r's ancestor
 *          at position j < p, p the position being decoded (double-buffered: a step reads one half and writes the other);
 *   pos, done: one int32 each in device memory: the position being decoded, and whether every row has ended.
 * Two kernels do what the GEMMs do not: single-query self-attention through the ancestor table, and the two top-N
 * selections of a step straight from the logits.  A step whose `done` is set, or whose `pos` has reached the cap, changes
 * nothing, so the host may issue steps in blocks and look at (done, pos) once per block.
 * Conventions as in pafc_attention.h.
 */
#ifndef PAFC_ATTN_SEARCH_H
#define PAFC_ATTN_SEARCH_H

#include "pafc_attention.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Single-query self-attention of the R new rows at position p = *pos, one launch for all rows and heads.  For row r, head h:
 *   cache[p*R + r] = [k | v] of the row, copied from qkv (every head of row r is stored by the launch);
 *   out[r, h*dk : (h+1)*dk] = softmax_j(q[r, h] . k_j[h] / sqrt(dk)) v_j[h]  over j in [0, p],
 *   key j < p being the cache row j*R + (r / N)*N + anc[p & 1][r][j], key p the row's own k and v.
 * dtype: PAFC_F32 or PAFC_BF16, the type of qkv, cache and out; products and the online softmax are float32, so the length
 *   is bounded by P only.
 * qkv: (R, ldqkv) the stacked projection of the new rows, q | k | v at the columns 0, H*dk, 2*H*dk; out: (R, ldo).
 *   ldqkv >= 3*H*dk, ldo >= H*dk, both multiples of 16 bytes; qkv, cache, out 16-byte aligned.
 * pos, done: device memory.  With *pos outside [0, P) or *done != 0 the launch writes nothing at all.  An entry of anc
 *   outside [0, N) is clamped into it: nothing is read outside the cache.
 * R = B*N must be a multiple of N; 1 <= N <= 16.  dk != 64: PAFC_ERR_UNSUPPORTED.  No workspace. */
int pafc_mha_step(int dtype, int R, int N, int H, int dk, int P, const void *qkv, long ldqkv, void *cache, const int32_t *anc,
                  const int32_t *pos, const int32_t *done, void *out, long ldo, pafc_stream_t stream);

/* Bytes of pafc_attn_beam_select's workspace (the N candidates of every row, their log-probabilities as doubles):
 * B * N * N * 12; 0 for bad arguments. */
size_t pafc_attn_beam_select_workspace_bytes(int B, int N);

/* One step's selection from the (R, ldl) logits of output_layer, R = B*N, at p = *pos (two launches).
 * Per row r: lse = logsumexp(logits[r, :]), accumulated in double, and the N largest logits, the lowest index winning a
 *   tie; candidate k of the row is (token_k, logits[r, token_k] - lse).  A row with ended[r] != 0 has the single candidate
 *   (eos, 0) and N - 1 candidates (eos, -inf): mask_finished_scores / mask_finished_preds.  The (R, V) log-softmax is
 *   never formed.
 * Per utterance b: the N best of its N*N candidates c = i*N + k (i the parent's slot) by score[b*N + i] + logp (the double
 *   sum rounded to float32 once), the lowest c winning a tie (-inf candidates after every finite one).  Slot s of the
 *   utterance, row r = b*N + s, gets the s-th best: score[r] the sum, token[r], ended[r] = (token == eos), the trace row p:
 *   trace_parent[p*R + r] = i, trace_token[p*R + r], trace_score[p*R + r], and
 *   anc[(p + 1) & 1][r] = anc[p & 1][b*N + i][0 .. p-1] followed by i at position p.
 * Then done = (every row ended) and pos = p + 1.
 * Frozen: with *done != 0 or *pos >= cap nothing is written.  1 <= cap < P; anc is (2, R, P), the traces (P, R).
 * logits: PAFC_F32 or PAFC_BF16, row pitch ldl >= V elements.  score, trace_score: float32; every other table int32; all in
 *   device memory.  1 <= N <= 16 and V >= N, else PAFC_ERR_UNSUPPORTED; 0 <= eos < V.
 * workspace: pafc_attn_beam_select_workspace_bytes(B, N) bytes, 8-byte aligned. */
int pafc_attn_beam_select(int dtype, int B, int N, int V, int P, int cap, int eos, const void *logits, long ldl, float *score,
                          int32_t *ended, int32_t *token, int32_t *anc, int32_t *trace_parent, int32_t *trace_token,
                          float *trace_score, int32_t *pos, int32_t *done, void *workspace, size_t workspace_bytes,
                          pafc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PAFC_ATTN_SEARCH_H */
