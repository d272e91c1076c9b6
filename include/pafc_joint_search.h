/*
 * pafc_joint_search.h -- C ABI of joint CTC/attention decoding, the time-synchronous beam search (reference:
 * BeamSearchTimeSync, wenet/espnet/beam_search_timesync.py; joint_decoding, wenet/transformer/search.py:450-496).
 *
 * The reference runs one Python loop per utterance and frame over dictionaries keyed by the prefix.  Here B utterances run in
 * lockstep with everything on the device.  R = B*N beam rows; utterance b owns the slots b*N .. b*N + N - 1, of which the first
 * nlive[b] hold a prefix.  Per utterance a trie of every prefix ever formed: a pool of M = 1 + T*N*C nodes (C = pre_beam_size;
 * an executed frame forms at most N*C prefixes; node 0 is [sos]) and an open-addressing hash (parent node, token) -> node of
 * HS slots, HS a power of two >= 2*M.  The self-attention key/value cache and the pool of decoded hidden rows have (T + 1)*R
 * rows: row f*R + r is written at most once, by slot r in decode round f (round 0 decodes [sos], round e follows the e-th
 * executed frame), and never moved; a prefix is decoded at most once per utterance and keeps its row when it leaves the beam.
 * Conventions as in pafc_attention.h.
 */
#ifndef PAFC_JOINT_SEARCH_H
#define PAFC_JOINT_SEARCH_H

#include "pafc_attention.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Single-query self-attention of R rows that stand at DIFFERENT positions: pafc_mha_step (pafc_attn_search.h) with a per-row
 * length and a per-row table of cache rows.  Row r of length L = length[r] (clamped into [1, W + 1]):
 *   if need[r] != 0 and 0 <= new_row[r] < rows: cache[new_row[r]] = [k | v] of the row, copied from qkv;
 *   out[r, h*dk : (h+1)*dk] = softmax_j(q[r, h] . k_j[h] / sqrt(dk)) v_j[h]  over j in [0, L - 1],
 *   key j < L - 1 being the cache row path[r*ldpath + j] (clamped into [0, rows)), key L - 1 the row's own k and v.
 * A row with need[r] == 0 writes nothing to the cache; its out row is computed all the same, from whatever its table names
 *   (the row rides along: its output is defined, finite for finite operands, and meant to be discarded).
 * dtype: PAFC_F32 or PAFC_BF16, the type of qkv, cache and out; products and the online softmax are float32.
 * qkv: (R, ldqkv), q | k | v at the columns 0, H*dk, 2*H*dk; cache: (rows, 2*H*dk); out: (R, ldo).  ldqkv >= 3*H*dk,
 *   ldo >= H*dk, both multiples of 16 bytes; qkv, cache, out 16-byte aligned.
 * path: (R, ldpath) int32, ldpath >= W, W the number of table entries a row can hold; length, new_row, need: (R) int32.
 *   All in device memory.  dk != 64: PAFC_ERR_UNSUPPORTED.  rows <= 2^31 - 1.  No workspace. */
int pafc_mha_step_paths(int dtype, int R, int H, int dk, int rows, int W, const void *qkv, long ldqkv, void *cache,
                        const int32_t *path, long ldpath, const int32_t *length, const int32_t *new_row, const int32_t *need,
                        void *out, long ldo, pafc_stream_t stream);

/* The candidates of every frame, one launch before the loop.  ctc: (B, T, V) CTC log-probabilities, PAFC_F32 or PAFC_BF16
 * (dtype), contiguous; lens: (B) int32 on the device.  For every frame t < lens[b]:
 *   cand_tok[b, t, 0..C-1] the C tokens with the largest values, the lowest index winning a tie, in ascending token order;
 *   cand_p[b, t, :] their values as float32; p_blank[b, t] = ctc[b, t, blank];
 *   skip[b, t] = (the arg-max is blank, lowest index winning a tie, and its value >= log_threshold).
 * Frames at or beyond lens[b] are left untouched.  1 <= C <= 24 and C <= V, else PAFC_ERR_UNSUPPORTED. */
int pafc_joint_candidates(int dtype, int B, int T, int V, int C, int blank, float log_threshold, const void *ctc,
                          const int32_t *lens, int32_t *cand_tok, float *cand_p, float *p_blank, int32_t *skip,
                          pafc_stream_t stream);

/* The device state of one call.  Every pointer is device memory that the caller allocates and initialises (the Python
 * wrapper hip_ops.JointSearchState is the reference for the initial values); nothing here is read by the host during the loop. */
typedef struct pafc_joint_state {
    int B, N, C, T, M, HS;
    /* the trie, (B, M) each: node 0 = [sos] */
    int32_t *parent, *token, *length;  /* length counts sos */
    int32_t *start, *end, *snap_end;   /* first frame; the live end frame; the PARENT's live end frame when the node was formed */
    float *ctc_conf, *snap_ctc_conf;   /* max of p_ctc[token] over the node's sightings; the parent's, when the node was formed */
    double *att_conf, *att_sum, *lse;  /* log p_dec(token | parent); its sum along the prefix; logsumexp of the node's logits row (NaN: not taken yet) */
    int32_t *row;                      /* the cache row where the node was decoded, or -1 */
    double *p_nb, *p_b;                /* (2, B, M): the CTC table of the executed frames of even / odd index */
    int32_t *stamp;                    /* (2, B, M): the index of the executed frame that wrote the entry (-1: never) */
    unsigned long long *hash_key;      /* (B, HS): parent << 32 | token, all ones = empty */
    int32_t *hash_node;                /* (B, HS) */
    /* per utterance, (B) */
    int32_t *n_nodes, *executed, *nlive, *evals;
    /* per slot, (R) */
    int32_t *node, *need, *in_token, *in_pos, *in_len, *new_row, *row_of_slot, *store_row;
    double *score;
    int32_t *path;                     /* (R, T + 1): the cache rows of the slot's ancestors by position */
    /* the frames' candidates (pafc_joint_candidates) */
    const int32_t *cand_tok;
    const float *cand_p, *p_blank;
    const int32_t *skip;
    /* the trace, (T, R): the slot's node (-1: empty) and joint score after frame t; trace_exec (T, B): was it executed */
    int32_t *trace_node;
    double *trace_score;
    int32_t *trace_exec;
} pafc_joint_state;

/* One frame t of the search for all utterances (one launch, one block per utterance).  A frame with t >= lens[b] or
 * skip[b, t] leaves utterance b untouched except need = 0 for its slots (and its trace row).  Otherwise, e being the index of
 * this executed frame (1, 2, ...): the beam's prefixes are expanded by the frame's candidates with find-or-insert in the
 * trie; the float64 CTC recursion writes the table of parity e & 1 from the one of parity (e - 1) & 1, with the reference's
 * rules for repeated tokens and for prefixes "considered before"; start / end frames and confidences follow the reference's
 * sequence of updates, a new node taking a snapshot of its parent's live (end, ctc_conf); every scored prefix h gets
 *   joint(h) = ctc_w * logadd(p_nb, p_b) + dec_w * att_sum(h) + bonus * (length(h) - 1)       (no attention term for [sos])
 * with att_sum(child) = att_sum(parent) + (logits[slot of parent, token] - lse), lse the row's logsumexp in double; the N best
 * (ties: the prefix that the reference's loop would have listed first) become the new beam: node, score, in_token, in_pos,
 * in_len, path (the parent slot's path, extended by the parent's cache row), row_of_slot, and for a prefix that was never
 * decoded (and only if dec_w > 0 and a later frame of the utterance exists) need = 1, new_row = store_row = e*R + r, which
 * becomes the node's row.  Slots beyond the scored prefixes are empty (node -1).  store_row of a row without need is
 * (T + 1)*R, the caller's dump row.  Deterministic: no result depends on the order in which lanes arrive.
 * logits: (R, ldl) in logits_dtype (PAFC_F32 / PAFC_BF16), row r the output_layer row of slot r's prefix; may be NULL when
 * dec_w == 0.  lens: (B) int32 device.  weights: three doubles in HOST memory, read before the launch: ctc_w, dec_w, bonus.
 * 1 <= N <= 16, 1 <= C <= 24. */
int pafc_joint_frame(const pafc_joint_state *state, int t, int logits_dtype, int V, const void *logits, long ldl,
                     const int32_t *lens, const double *weights, int blank, pafc_stream_t stream);

/* After the last frame: the beams' hypotheses in compact form, one launch.  Per slot r (W = T + 1 columns per row):
 * out_len[r] the prefix's length without sos (-1: empty slot); out_tok / out_start / out_end (R, W) int32, out_ctc_conf
 * (R, W) float32 and out_att_conf (R, W) float64: per token its id, start frame, reported end frame and confidences -- the
 * last token's live values, every other token's as snapshotted by the next node on the path. */
int pafc_joint_collect(const pafc_joint_state *state, int32_t *out_len, int32_t *out_tok, int32_t *out_start, int32_t *out_end,
                       float *out_ctc_conf, double *out_att_conf, pafc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PAFC_JOINT_SEARCH_H */
