/*
 * pafc_attention.h -- C ABI of the attention decoder's second pass (attention rescoring: wenet/transformer/search.py:364-448,
 * asr_model.py:876-986 of the reference).
 *
 * The reference repeats the encoder output once per hypothesis, pads every hypothesis to the longest and forms the
 * (beam, L, V) log-softmax to read L + 1 numbers of each.  Here all hypotheses of all utterances are packed as rows without
 * padding (hypothesis i owns L_i + 1 rows), an utterance's memory is projected once, and two kernels do what the GEMMs do
 * not: multi-head attention over row groups, and log p(target) per row straight from the logits.
 * Conventions as in pafc_wkv6.h.
 */
#ifndef PAFC_ATTENTION_H
#define PAFC_ATTENTION_H

#include "pafc_wkv6.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Multi-head scaled-dot-product attention over G row groups, one launch for all groups and heads:
 *   out[r, h*dk : (h+1)*dk] = softmax_j(q[r, h] . k[kv_off[g] + j, h] / sqrt(dk)) v[kv_off[g] + j, h]
 * for the query rows r in [q_off[g], q_off[g + 1]) of group g and the keys j in [0, kv_len[g]); head h is the column slice
 * [h*dk, (h+1)*dk) of a row of q / k / v / out.
 * dtype: PAFC_F32 (QK^T and PV on the fp32 matrix cores: exact products, fp32 accumulation) or PAFC_BF16 (bf16 matrix
 *   cores, fp32 accumulation, the probabilities rounded to bf16 for PV); the softmax is online over key tiles in fp32, so
 *   kv_len is bounded by memory alone.
 * q: rows of ldq elements; k, v: rows of ldkv elements (two pointers into one stacked [K | V] projection, or two buffers);
 *   out: rows of ldo elements.  ldq, ldkv, ldo >= H*dk and multiples of 16 bytes; q, k, v, out 16-byte aligned.
 * q_off: (G + 1) int32, non-decreasing; kv_off, kv_len: (G) int32 -- all three in device memory.
 * causal = 1: query i of its group (row q_off[g] + i) sees the keys [0, min(i + 1, kv_len[g])): self-attention over packed
 *   rows with kv_off = q_off and kv_len = the group's rows.  causal = 0: every query of the group sees all kv_len[g] keys.
 * A group with kv_len[g] = 0 gets zeros; a group without query rows is skipped.
 * dk != 64: PAFC_ERR_UNSUPPORTED.  No workspace. */
int pafc_mha_rows(int dtype, int G, int H, int dk, const void *q, long ldq, const void *k, const void *v, long ldkv,
                  const int32_t *q_off, const int32_t *kv_off, const int32_t *kv_len, int causal, void *out, long ldo,
                  pafc_stream_t stream);

/* out[r] = logits[r, target[r]] - logsumexp(logits[r, :]): the log-probability of one token per row without the (rows, V)
 * log-softmax.  logits: (rows, V) PAFC_F32 or PAFC_BF16 with row pitch ldl >= V elements, read once; target: (rows) int32 in
 * device memory (a target outside [0, V) gives NaN, nothing is read out of bounds); out: (rows) float32.  A NaN anywhere in
 * a row gives NaN for that row, as log_softmax does; -inf logits are ordinary (a row of nothing but -inf gives NaN). */
int pafc_logp_gather_rows(int dtype, long rows, int V, const void *logits, long ldl, const int32_t *target, float *out,
                          pafc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PAFC_ATTENTION_H */
