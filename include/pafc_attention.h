/*
 * pafc_attention.h -- C ABI of the attention decoder over packed rows: its second pass (attention rescoring:
 * wenet/transformer/search.py:364-448, asr_model.py:876-986 of the reference) and, further down, the training half (the
 * attention loss, asr_model.py:251-292: attention with statistics, its backward, the label-smoothing loss from the logits).
 *
 * The reference repeats the encoder output once per hypothesis, pads every hypothesis to the longest and forms the
 * (beam, L, V) log-softmax to read L + 1 numbers of each.  Here all hypotheses of all utterances are packed as rows without
 * padding (hypothesis i owns L_i + 1 rows), an utterance's memory is projected once, and two kernels do what the GEMMs do
 * not: multi-head attention over row groups, and log p(target) per row straight from the logits.
 * pafc_mha_band is the encoder-side attention of the Conformer baseline (limited context, positional term).
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

/* Limited-context self-attention with the positional term of the Conformer baseline (limited_rel_selfattn with
 * global_tokens = 0: wenet/transformer/attention.py:406-645 of the reference), one launch for every batch row, head and query:
 *   out[b*T + i, h*dk : (h+1)*dk] = sum_j softmax_j(s_ij) v[b*T + j, h]   over the keys j with |j - i| <= w, 0 <= j < t_pad,
 *   s_ij = ((q[b*T + i, h] + u[h]) . k[b*T + j, h] + (q[b*T + i, h] + v_bias[h]) . p[j, h]) / sqrt(dk)    for j < T;
 * p[j] is the KEY's position row (no relative shift) and is shared by the batch.  The keys T <= j < t_pad are the zero padding
 * of the reference's blocked layout and are NOT masked: score 0, value 0, so each adds exp(0 - max) to its queries'
 * denominators and nothing to their numerators.  They are arithmetic here: no operand has a row T or later.  Any
 * t_pad >= T is taken (the reference's is T rounded up to a multiple of 2w); with w >= t_pad every query sees every key: full
 * attention with the positional term.  There is no length mask (the reference applies none): a batch row's padded frames
 * take part as keys with whatever they hold and get output rows.
 * dtype: PAFC_F32 (both products on the fp32 matrix cores: exact products, fp32 accumulation) or PAFC_BF16 (bf16 matrix
 *   cores, fp32 accumulation, q + u and q + v rounded to bf16 once, the probabilities rounded to bf16 for PV); the softmax is
 *   online over key tiles in fp32.
 * q: rows of ldq elements; k, v: rows of ldkv elements (three pointers into one stacked [Q | K | V] projection with
 *   ldq = ldkv, or separate buffers); p: (T) rows of ldp elements; out: rows of ldo elements; all B*T rows except p.
 *   Every pitch >= H*dk and a multiple of 16 bytes.  pos_bias_u, pos_bias_v: (H, dk) contiguous, in `dtype`.
 *   q, k, v, p, pos_bias_u, pos_bias_v, out 16-byte aligned.  Row offsets are 64-bit.
 * B, H in [1, 65535], 1 <= T <= t_pad <= 2^30, w >= 0 (w = 0: a query sees itself, and the padding keys none).
 * dk != 64: PAFC_ERR_UNSUPPORTED.  No workspace; two runs on the same input give the same bits. */
int pafc_mha_band(int dtype, int B, int T, int H, int dk, int w, int t_pad, const void *q, long ldq, const void *k,
                  const void *v, long ldkv, const void *p, long ldp, const void *pos_bias_u, const void *pos_bias_v,
                  void *out, long ldo, pafc_stream_t stream);

/* ---- the training half: the attention decoder's loss on packed rows (one group per utterance, [sos] + y) ---- */

/* pafc_mha_rows that also writes lse[r, h] = m + log(l), the log of the softmax's denominator of query row r and head h, as
 * float32 (rows, H) (row pitch H): what the backward needs to form P again.  out holds the bits pafc_mha_rows writes.  Rows of a
 * group with kv_len[g] = 0 get lse = -inf; rows outside every group are not written. */
int pafc_mha_rows_lse(int dtype, int G, int H, int dk, const void *q, long ldq, const void *k, const void *v, long ldkv,
                      const int32_t *q_off, const int32_t *kv_off, const int32_t *kv_len, int causal, void *out, long ldo,
                      float *lse, pafc_stream_t stream);

/* Bytes of pafc_mha_rows_bwd's workspace (delta, one float32 per query row and head): rows * H * 4; 0 for bad arguments. */
size_t pafc_mha_rows_bwd_workspace_bytes(long rows, int H);

/* The backward of pafc_mha_rows: from q, k, v, the forward's out and lse and the upstream gradient dout, with
 *   P = exp(S / sqrt(dk) - lse), delta_i = sum_d dout_id out_id, dS = P o (dout V^T - delta)
 * per group and head,
 *   dq = dS K / sqrt(dk),  dk = dS^T Q / sqrt(dk),  dv = P^T dout.
 * dtype as in the forward: PAFC_F32 takes every product exactly on the fp32 matrix cores, PAFC_BF16 runs on the bf16 matrix
 *   cores with fp32 accumulation, P and dS rounded to bf16 for the products that consume them.
 * rows: the query rows q / out / dout / dq / lse hold (q_off[G] <= rows); it sizes the workspace.
 * out / dout / dq: rows of ldo / lddo / lddq elements; dk_out, dv_out: rows of lddkv elements (two pointers into one stacked
 *   buffer, or two buffers).  Every pitch >= H*dk and a multiple of 16 bytes, every operand 16-byte aligned; nothing past a
 *   group's end is read.
 * PRECONDITION: the key ranges [kv_off[g], kv_off[g] + kv_len[g]) of two groups that both have query rows do not overlap.  A
 *   row of dk / dv then has one owner and no atomics are needed: two runs on the same input give the same bits.  Overlapping
 *   ranges give wrong values in the shared rows, never an access outside the buffers.
 * Written: dq for the query rows of every group (zeros where kv_len[g] = 0), dk / dv for the key rows of every group that has
 *   query rows.  Rows outside every group's range are NOT written by the kernels: the caller zeroes dq / dk / dv first where
 *   it needs zeros there (hip_ops.mha_rows_bwd does).
 * workspace: pafc_mha_rows_bwd_workspace_bytes(rows, H) bytes, 4-byte aligned.
 * dk != 64: PAFC_ERR_UNSUPPORTED. */
int pafc_mha_rows_bwd(int dtype, int G, int H, int dk, long rows, const void *q, long ldq, const void *k, const void *v,
                      long ldkv, const void *out, long ldo, const void *dout, long lddo, const float *lse,
                      const int32_t *q_off, const int32_t *kv_off, const int32_t *kv_len, int causal, void *dq, long lddq,
                      void *dk_out, void *dv_out, long lddkv, void *workspace, size_t workspace_bytes, pafc_stream_t stream);

/* Label-smoothing loss per row in one pass over the logits (reference: wenet/transformer/label_smoothing_loss.py, the KL sum
 * against the smoothed one-hot distribution, without the (rows, V) log-softmax):
 *   loss[r] = C - conf * logp_y - s * (sum_v x_v - V * lse[r] - logp_y),   logp_y = x_y - lse[r],  y = target[r],
 *   s = smoothing / (V - 1), conf = 1 - smoothing, C = conf log conf + (V - 1) s log s with 0 log 0 = 0;
 *   lse[r] = logsumexp(x_r);  correct[r] = (argmax_v x_rv == y), the lowest index winning a tie.
 * logits: (rows, V) PAFC_F32 or PAFC_BF16 with row pitch ldl >= V; target: (rows) int32; loss, lse: (rows) float32; correct:
 * (rows) int32 -- all in device memory.  target -1 is the ignore id: loss 0, correct 0.  Any other target outside [0, V) gives
 * loss NaN and correct 0 for that row; nothing is read out of bounds.  V >= 2, 0 <= smoothing <= 1. */
int pafc_lsm_loss_rows(int dtype, long rows, int V, const void *logits, long ldl, const int32_t *target, float smoothing,
                       float *loss, float *lse, int32_t *correct, pafc_stream_t stream);

/* dlogits[r, v] = g * (exp(x_rv - lse[r]) - t_v) in the logits' dtype, t_v = conf at the target and s elsewhere: the gradient
 * of sum_r loss[r] scaled by g, ONE float32 read from device memory (the upstream gradient times 1 / denominator).  Ignored rows
 * (target -1) get zeros, a row whose target is otherwise outside [0, V) gets NaN, and the columns [V, ldd) of every row get
 * zeros (the padding that makes the dX GEMM's K a multiple of 64).  dlogits may be the logits themselves (then ldd = ldl). */
int pafc_lsm_loss_rows_bwd(int dtype, long rows, int V, const void *logits, long ldl, const int32_t *target, float smoothing,
                           const float *lse, const float *g, void *dlogits, long ldd, pafc_stream_t stream);

/* ---- the training half of the Conformer baseline's slot: pafc_mha_band with statistics, and its backward ---- */

/* pafc_mha_band that also writes lse[b*T + i, h] = m' + log(l'), the log of the softmax's denominator of query i and head h
 * INCLUDING the padding keys' term n0_i e^0 (n0_i = max(0, min(t_pad - 1, i + w) - T + 1)), as float32 (B*T, H) with row pitch
 * H: what the backward needs to form P again.  out holds the bits pafc_mha_band writes.  lse 4-byte aligned. */
int pafc_mha_band_lse(int dtype, int B, int T, int H, int dk, int w, int t_pad, const void *q, long ldq, const void *k,
                      const void *v, long ldkv, const void *p, long ldp, const void *pos_bias_u, const void *pos_bias_v,
                      void *out, long ldo, float *lse, pafc_stream_t stream);

/* Bytes of pafc_mha_band_bwd's workspace: the position-row gradient of every batch row (B, T, H*64) and the column sums of
 * dqu | dqv of every query tile of 16 (B * ceil(T / 16), H, 128) in float32, and delta (B*T, H) in float64; 0 for bad
 * arguments. */
size_t pafc_mha_band_bwd_workspace_bytes(int B, int T, int H);

/* The backward of pafc_mha_band: from its operands, the out and lse of pafc_mha_band_lse and the upstream gradient dout.  Per
 * batch row and head, with qu_i = q_i + u, qv_i = q_i + v_bias, P_ij = exp(s_ij - lse_i) for the real keys of the band,
 * delta_i = sum_d dout_id out_id and dS_ij = P_ij (dout_i . v_j - delta_i):
 *   dqu_i = sum_j dS_ij k_j / sqrt(dk),  dqv_i = sum_j dS_ij p_j / sqrt(dk),  dq_i = dqu_i + dqv_i,
 *   dk_j = sum_i dS_ij qu_i / sqrt(dk),  dv_j = sum_i P_ij dout_i,
 *   dp_j = sum_b sum_i dS_ij qv_i / sqrt(dk)   (the position rows are shared by the batch),
 *   du = sum_{b,i} dqu_i,  dvb = sum_{b,i} dqv_i.
 * The padding keys have a constant score and a zero value: they enter through lse alone and receive no gradient.
 * dtype as in the forward: PAFC_F32 takes every product exactly on the fp32 matrix cores; PAFC_BF16 runs on the bf16 matrix
 *   cores with fp32 accumulation, P and dS rounded to bf16 for the products that consume them, and uses the forward's
 *   rounded q + u and q + v (that rounding is treated as the identity).
 * out / dout / dq: B*T rows of ldo / lddo / lddq elements; dk_out, dv_out: B*T rows of lddkv elements (pointers into one
 *   stacked buffer, or separate ones); dp: T rows of lddp elements; all in `dtype`.  du, dvb: (H, dk) contiguous FLOAT32, the
 *   sums over every row of the batch.  Every pitch >= H*dk and a multiple of 16 bytes; every operand, dq, dk_out, dv_out, dp
 *   and the workspace 16-byte aligned; lse, du, dvb 4-byte aligned.  Nothing past row T - 1 of any operand is read.
 * Every row of every output is written: the caller zeroes nothing.  No atomics: every sum has a fixed order, two runs on the
 *   same input give the same bits, and dq / dk / dv of a batch row do not depend on the other rows.
 * workspace: pafc_mha_band_bwd_workspace_bytes(B, T, H) bytes.  Limits on B, T, H, w, t_pad as in pafc_mha_band, and
 *   T * H / 16 + 2 H < 2^31 (the blocks of the reduce launch): PAFC_ERR_BAD_DIMS otherwise.
 * dk != 64: PAFC_ERR_UNSUPPORTED. */
int pafc_mha_band_bwd(int dtype, int B, int T, int H, int dk, int w, int t_pad, const void *q, long ldq, const void *k,
                      const void *v, long ldkv, const void *p, long ldp, const void *pos_bias_u, const void *pos_bias_v,
                      const void *out, long ldo, const void *dout, long lddo, const float *lse, void *dq, long lddq,
                      void *dk_out, void *dv_out, long lddkv, void *dp, long lddp, float *du, float *dvb, void *workspace,
                      size_t workspace_bytes, pafc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PAFC_ATTENTION_H */
