/*
 * pafc_search.h -- C ABI of the GPU-resident part of the decode step.
 *
 * CTC greedy search of the reference (wenet/transformer/search.py:106-121 + remove_duplicates_and_blank,
 * wenet/utils/ctc_utils.py:22-32): argmax over the vocabulary per frame, frames beyond the utterance length count as
 * blank, runs of equal ids collapse to one, blanks are dropped.  There: topk on the device, a (B, T) copy to the
 * host and a Python loop per frame.  Here: two kernels; only the collapsed token lists leave the device.
 * Conventions as in pafc_wkv6.h.
 */
#ifndef PAFC_SEARCH_H
#define PAFC_SEARCH_H

#include "pafc_wkv6.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scores: (B, T, V) contiguous, PAFC_F32 or PAFC_BF16 -- log-probabilities or logits (same argmax).
 * lens: (B) int64 valid frames per utterance, or NULL (all T frames valid).
 * best: (B, T) int32 scratch that receives the per-frame argmax (ties: lowest index, like torch.topk / argmax;
 *       padded frames: blank_id).
 * tokens: (B, T) int32, row b holds ntok[b] collapsed token ids; ntok: (B) int32.
 * frames: (B, T) int32 or NULL: frame index of the FIRST frame of each emitted token (for time stamps). */
int pafc_ctc_greedy(int dtype, int B, int T, int V, const void *scores, const int64_t *lens, int blank_id,
                    int32_t *best, int32_t *tokens, int32_t *ntok, int32_t *frames, pafc_stream_t stream);

/* Row-wise log-softmax over the vocabulary: out[r][v] = x[r][v] - max_v x[r] - log sum_v exp(x[r][v] - max), fp32
 * arithmetic, one rounding to the element type (CTC.log_softmax, wenet/transformer/ctc.py:106-114, behind
 * ASRModel.ctc_logprobs, asr_model.py:324-335).  x, out: (rows, V) contiguous, may alias.  One pass over HBM: a wave
 * keeps its row in registers (V <= 8192 elements in bf16, 4096 in fp32; longer rows are re-read from cache). */
int pafc_log_softmax_rows(int dtype, long rows, int V, const void *x, void *out, pafc_stream_t stream);

/* CTC prefix beam search (ctc_prefix_beam_search, wenet/transformer/search.py:124-248, without context graph and time
 * stamps -- see pafc_ctc_prefix_beam_search_ex for both), one wave per utterance, frames walked on the device.
 * top_logp / top_idx: (B, T, K) the K best log-probabilities and token ids per frame, best first (torch.topk of the CTC
 *   log-probs, as the reference takes them per frame); K <= 16, beam <= 16.  lens: (B) int64 valid frames, or NULL.
 * out_tokens: (B, beam, T) int32, entry (b, n) holds out_len[b][n] ids of the n-th best prefix (best first);
 * out_len: (B, beam) int32, -1 for unused entries (fewer prefixes than beam); out_score: (B, beam) float64 total
 * log-probabilities (arithmetic in float64 like the reference's Python floats).
 * workspace: pafc_ctc_prefix_beam_workspace_bytes(B, T, beam) bytes (the per-utterance prefix tries). */
size_t pafc_ctc_prefix_beam_workspace_bytes(int B, int T, int beam);
int pafc_ctc_prefix_beam_search(int B, int T, int K, const float *top_logp, const int32_t *top_idx, const int64_t *lens,
                                int beam, int blank_id, int32_t *out_tokens, int32_t *out_len, double *out_score,
                                void *workspace, size_t workspace_bytes, pafc_stream_t stream);

/* The same search with the reference's context biasing and token time stamps (the whole of search.py:124-248).
 * graph: NULL (no biasing) or a host struct of device tables of a ContextGraph (utils/context_graph.py:
 *   ContextGraph.device_tables), node 0 the root: child_begin (num_nodes + 1) and child_token / child_node (one entry per
 *   arc) int32, each node's children sorted by token; fail (num_nodes) int32; token_score / node_score / output_score
 *   (num_nodes) float64.  The prune ranks on score + context bonus; out_score is score + the finalize() bonus
 *   (-node_score of the survivor's state) -- the order is not revisited after finalize, as in the reference.
 * out_times: NULL, or (B, beam, T) int32: entry (b, n) holds the frame of every token of the n-th prefix's viterbi path
 *   (the reference's DecodeResult.times / nbest_times), then -1 up to T.  The list may be shorter than the token list
 *   where the reference's is.
 * With graph == NULL and out_times == NULL the results equal pafc_ctc_prefix_beam_search's bit for bit.
 * workspace: pafc_ctc_prefix_beam_ex_workspace_bytes(B, T, beam) bytes (prefix tries and frame lists). */
typedef struct pafc_ctc_context_graph {
    int num_nodes;
    const int32_t *child_begin, *child_token, *child_node, *fail;
    const double *token_score, *node_score, *output_score;
} pafc_ctc_context_graph;

size_t pafc_ctc_prefix_beam_ex_workspace_bytes(int B, int T, int beam);
int pafc_ctc_prefix_beam_search_ex(int B, int T, int K, const float *top_logp, const int32_t *top_idx,
                                   const int64_t *lens, int beam, int blank_id, const pafc_ctc_context_graph *graph,
                                   int32_t *out_tokens, int32_t *out_len, double *out_score, int32_t *out_times,
                                   void *workspace, size_t workspace_bytes, pafc_stream_t stream);

/* CTC prefix beam search chunk by chunk (pafc_ctc_beam_stream_*): the search of pafc_ctc_prefix_beam_search_ex with the
 * beam carried from one chunk to the next in `workspace`.  After any cut of a row's frames into feeds, the n-best token
 * lists, frame lists and float64 scores are those of the offline search of the concatenated frames, bit for bit: a feed
 * loads the beam, runs the offline kernel's per-frame arithmetic and stores the beam back.  Nothing reads the host or
 * allocates, so a feed can be captured in a graph.  beam <= 16, K <= 16, max_total_frames * beam < 2^31 - 1.
 * max_total_frames: the most frames a row may consume between two resets; it sizes the row's node pools, which keep the
 *   offline numbering by absolute frame (node 1 + t * beam + rank).  Memory per stream: 1240 bytes of beam state plus
 *   (1 + max_total_frames * beam) nodes of 8 bytes, or 16 bytes with_times (beam 8, 4000 frames = 160 s: 500 kB).  The
 *   pools are not compacted: reset a row at an endpoint.
 * with_times: the workspace also holds the frame lists (DecodeResult.times); the same value in every call on a workspace.
 * reset: rows with row_mask[b] != 0 (device int32 (B), or NULL = every row) start again from the empty prefix at absolute
 *   frame 0, overflow flag cleared.  Call it on every row before the first feed.
 * feed: row b consumes its first clamp(nframes[b], 0, Tmax) frames of top_logp / top_idx ((B, Tmax, K), as in
 *   pafc_ctc_prefix_beam_search; nframes: device int64 (B)).  A row with 0 frames is untouched.  A feed that would take a
 *   row past max_total_frames consumes nothing for that row and sets its overflow flag, which stays until the reset (2: the
 *   row was never reset).  graph: NULL or the context graph, the same for every feed of a stream.
 * drain: the n-best of every row as if its stream ended here; the carried state is not changed.  from: device int32 (B)
 *   or NULL (= 0): tokens [from[b], from[b] + ld) of each list go to out_tokens (B, beam, ld); pass the committed count of
 *   an earlier drain, and the walk and the copy are bounded by the tail that is not final yet.  out_len (B, beam): the
 *   TOTAL token count of each entry, -1 for unused entries; out_score (B, beam) float64, with a graph score + the
 *   finalize() bonus of the entry's state; out_count (B): entries in use; out_committed (B): the length of the longest
 *   common prefix of the row's token lists -- every later hypothesis extends one of them, so these tokens are final
 *   (looked for at or above from[b]: a `from` beyond it is the caller's error); out_overflow (B): the row's flag.
 *   out_ntimes (B, beam) / out_times (B, beam, ld_times), or NULL (need with_times): the length of each entry's frame
 *   list and its first ld_times frames (ld_times 0: lengths only).  Frame lists are per entry and final only at the end. */
size_t pafc_ctc_beam_stream_workspace_bytes(int B, int max_total_frames, int beam, int with_times);
int pafc_ctc_beam_stream_reset(int B, int max_total_frames, int beam, int with_times, const int32_t *row_mask,
                               void *workspace, size_t workspace_bytes, pafc_stream_t stream);
int pafc_ctc_beam_stream_feed(int B, int Tmax, int K, const float *top_logp, const int32_t *top_idx, const int64_t *nframes,
                              int max_total_frames, int beam, int blank_id, const pafc_ctc_context_graph *graph,
                              int with_times, void *workspace, size_t workspace_bytes, pafc_stream_t stream);
int pafc_ctc_beam_stream_drain(int B, int max_total_frames, int beam, const pafc_ctc_context_graph *graph, int with_times,
                               const void *workspace, size_t workspace_bytes, const int32_t *from, int ld,
                               int32_t *out_tokens, int32_t *out_len, double *out_score, int32_t *out_count,
                               int32_t *out_committed, int32_t *out_overflow, int ld_times, int32_t *out_times,
                               int32_t *out_ntimes, pafc_stream_t stream);

/* CTC greedy search chunk by chunk: pafc_ctc_greedy over the first clamp(nframes[b], 0, Tmax) frames of scores
 * (B, Tmax, V), with two values carried per row in `workspace` (pafc_ctc_greedy_stream_workspace_bytes(B) = 16 B bytes):
 * the previous frame's argmax, so a run of equal ids that crosses a chunk boundary collapses once, and the frames consumed
 * so far, so `frames` ((B, Tmax) int64, or NULL) are absolute.  Frames beyond nframes[b] are ignored (not blank).  tokens /
 * ntok: the tokens this chunk adds.  reset: rows with row_mask[b] != 0 (NULL = all) start a new stream. */
size_t pafc_ctc_greedy_stream_workspace_bytes(int B);
int pafc_ctc_greedy_stream_reset(int B, const int32_t *row_mask, void *workspace, size_t workspace_bytes, pafc_stream_t stream);
int pafc_ctc_greedy_stream(int dtype, int B, int Tmax, int V, const void *scores, const int64_t *nframes, int blank_id,
                           void *workspace, size_t workspace_bytes, int32_t *best, int32_t *tokens, int32_t *ntok,
                           int64_t *frames, pafc_stream_t stream);

/* CTC forced alignment (force_align, wenet/utils/ctc_utils.py:105-161, for B utterances at once): the best path of the
 * log-probabilities lp through the extended labels l' = (blank, y_1, blank, ..., y_L, blank), S = 2 L + 1 states, and the
 * frames of its tokens.  One block per utterance, one launch; nothing reads the host, allocates or synchronises.
 * Recursion, all in fp32, each value one add: alpha_t(s) = max(cands) + lp[t, l'_s], the candidates in this order
 *   alpha_{t-1}(s); alpha_{t-1}(s-1) if s >= 1; alpha_{t-1}(s-2) if s >= 2, l'_s != blank and l'_s != l'_{s-2};
 * a later candidate wins only when strictly greater (torch.argmax).  alpha_0(0) = lp[0, blank], alpha_0(1) = lp[0, y_1], the
 * rest -inf.  The path ends in state S-1 unless alpha(S-2) > alpha(S-1).  -inf entries are data; NaN input is undefined.
 * State 0 has itself as its only predecessor (the reference indexes state -1 there, the LAST state: DESIGN.md).
 * lp: (B, T, V) of PAFC_F32 or PAFC_BF16 in rows of ldl >= V elements.  hlens (B) int32 frames; ys (B, ldy) int64 labels,
 * ylens (B) int32 label counts.  ldy is also the most labels an utterance may have (Lmax): it sizes the workspace and
 * the kernel's LDS, two frames of alpha with two guard entries each: 2 x (64 ceil((2 ldy + 1) / 64) + 2) x 4 bytes of the
 * CU's 160 KiB.  The cap is ldy <= 8191 (S <= 16383: 128 KiB of LDS, 16 states per thread of a 1024-thread block -- more
 * per thread spills registers before the LDS is full), else PAFC_ERR_UNSUPPORTED; V < 2^30.  ys may be NULL when ldy == 0,
 * first / last when ld_times == 0.
 * align (B, T) int32: the token of every frame, -1 from hlens[b] on.  first / last (B, ld_times >= ldy) int32: the first and
 * the last frame of label i's state 2 i + 1 (first = gen_ctc_peak_time of the alignment), -1 from ylens[b] on.
 * score (B) fp32: the end state's alpha.  ok (B) int32: 1, or 0 for a row that cannot be aligned -- hlens[b] outside [1, T],
 * ylens[b] outside [0, ldy], a label that is the blank or outside [0, V), more labels plus adjacent equal labels than frames,
 * a final score of -inf -- which gets score -inf and -1 in all of align, first and last.  L = 0: every frame blank.
 * Frames beyond hlens[b] and labels beyond ylens[b] are never read.
 * workspace: pafc_ctc_align_workspace_bytes(B, T, ldy) = B T ceil((2 ldy + 1) / 64) 16 + 32 B bytes (0 when B, T <= 0 or
 *   Lmax < 0), 16-byte aligned: the back-pointers (0, 1 or 2: 2 bits each, two 64-bit planes per 64 states and frame) and, per
 *   utterance, three 64-bit wall-clock stamps (start, recursion done, backtrace done).  The stamps are a diagnostic for
 *   tools/bench_ctc_align.py, not a stable contract: only the size of the workspace is, what the kernel leaves in it is not. */
size_t pafc_ctc_align_workspace_bytes(int B, int T, int Lmax);
int pafc_ctc_align(int dtype, int B, int T, int V, const void *lp, long ldl, const int32_t *hlens, const int64_t *ys, int ldy,
                   const int32_t *ylens, int blank, void *workspace, size_t workspace_bytes, int32_t *align, int32_t *first,
                   int32_t *last, int ld_times, float *score, int32_t *ok, pafc_stream_t stream);

/* CTC-fused RNN-T prefix beam search (PrefixBeamSearch.prefix_beam_search_decode_batch,
 * wenet/transducer/search/prefix_beam_search.py:428-574): the per-frame candidate walk on the device.  The caller keeps
 * B x beam fixed slots; per frame it runs predictor step + joint + log-softmax + fusion + top-`beam` for all slots with
 * framework ops and hands the (B, beam, beam) values / token ids to pafc_rnnt_beam_step, which updates the beams in
 * `workspace` and returns, per slot, where the survivor's LSTM state comes from -- next_idx[slot] indexes the
 * concatenation [old states (B*beam) | new states (B*beam)] -- and the token to feed the predictor next (last_tok).
 * No host synchronisation between frames.  beam <= 16.  lens: (B) int64 valid frames or NULL.  t_dev (device int64, or
 * NULL): when given, the frame index is read from it instead of `t`, so the whole frame body can be captured once in a
 * hipGraph and replayed (the caller increments it); frames t >= T are no-ops.
 * pafc_rnnt_beam_finish writes the n-best lists like pafc_ctc_prefix_beam_search (the leading blank is not included). */
size_t pafc_rnnt_beam_workspace_bytes(int B, int T, int beam);
int pafc_rnnt_beam_init(int B, int T, int beam, int blank_id, void *workspace, size_t workspace_bytes, int64_t *next_idx,
                        int64_t *last_tok, pafc_stream_t stream);
int pafc_rnnt_beam_step(int B, int T, int beam, int blank_id, int t, const int64_t *t_dev, const int64_t *lens,
                        const float *top_val, const int64_t *top_idx, void *workspace, size_t workspace_bytes,
                        int64_t *next_idx, int64_t *last_tok, pafc_stream_t stream);
int pafc_rnnt_beam_finish(int B, int T, int beam, void *workspace, size_t workspace_bytes, int32_t *out_tokens,
                          int32_t *out_len, double *out_score, pafc_stream_t stream);

/* The same search chunk by chunk (pafc_rnnt_beam_stream_*), the beams carried from one chunk to the next in `workspace`.
 * The caller keeps B x beam slots as above and fixed (B, Tmax, ...) staging buffers of the current chunk; per chunk it calls
 * feed once and then, for j = 0 .. Tmax - 1 (or up to the longest row), its frame body on frame j of the staging buffers
 * followed by step.  The step kernel includes the per-frame text of pafc_rnnt_beam_step (csrc/rnnt_beam_frame.inc), so after
 * any cut of a row's frames into chunks the n-best token lists, float64 scores and every frame's next_idx / last_tok are
 * those of the offline search of the concatenated frames, bit for bit, given the same top_val / top_idx.  Nothing reads the
 * host or allocates: a feed and its steps can be captured in a graph.
 * max_total_frames: the most frames a row may consume between two resets; it sizes the row's trie pools of
 *   1 + max_total_frames * beam nodes of 8 bytes, numbered by absolute frame (node 1 + t_abs * beam + rank).  The workspace
 *   holds the beam state of pafc_rnnt_beam_* for T = max_total_frames and, per row, the frames consumed since the reset, the
 *   frames taken in the current chunk, an overflow flag and each member's token count.  beam <= 16 and max_total_frames *
 *   beam < 2^31 - 1, else PAFC_ERR_UNSUPPORTED (workspace_bytes: 0).
 * reset: rows with row_mask[b] != 0 (device int32 (B), or NULL = every row) restart: one live beam of score 0 at the root
 *   node, last_tok = blank and the identity next_idx for the row's slots, consumed frames 0, overflow flag cleared.  Other
 *   rows are untouched.  Call it on every row before the first feed.  (The LSTM state of the slots is the caller's.)
 * feed: begins a chunk: row b takes clamp(nframes[b], 0, Tmax) frames (nframes: device int64 (B)).  A feed that would take a
 *   row past max_total_frames takes nothing for that row and sets its overflow flag, which stays until the reset (2: the row
 *   was never reset).
 * step: frame j of the chunk, j read from *j_dev (device int64) when that is given.  A row with j >= its taken count is a
 *   no-op with the identity next_idx, as a finished utterance is offline; a live row runs the walk at absolute frame
 *   consumed[b], then consumed[b] advances.  top_val float32 / top_idx int64: (B, beam, beam).
 * drain: the n-best of every row as if its stream ended here; the state is not changed.  The contract of
 *   pafc_ctc_beam_stream_drain: from (device int32 (B), or NULL = 0): tokens [from[b], from[b] + ld) of each list go to
 *   out_tokens (B, beam, ld); out_len (B, beam): TOTAL token counts, -1 for unused entries; out_score (B, beam) float64;
 *   out_count (B): entries in use; out_committed (B): the length of the longest common prefix of the row's live hypotheses --
 *   every later hypothesis is a live one, or a live one plus a token, so these tokens are final (looked for at or above
 *   from[b]); out_overflow (B): the row's flag.  The walk and the copy are bounded by the uncommitted tail. */
size_t pafc_rnnt_beam_stream_workspace_bytes(int B, int max_total_frames, int beam);
int pafc_rnnt_beam_stream_reset(int B, int max_total_frames, int beam, int blank_id, const int32_t *row_mask, void *workspace,
                                size_t workspace_bytes, int64_t *next_idx, int64_t *last_tok, pafc_stream_t stream);
int pafc_rnnt_beam_stream_feed(int B, int Tmax, int max_total_frames, int beam, const int64_t *nframes, void *workspace,
                               size_t workspace_bytes, pafc_stream_t stream);
int pafc_rnnt_beam_stream_step(int B, int Tmax, int max_total_frames, int beam, int blank_id, int j, const int64_t *j_dev,
                               const float *top_val, const int64_t *top_idx, void *workspace, size_t workspace_bytes,
                               int64_t *next_idx, int64_t *last_tok, pafc_stream_t stream);
int pafc_rnnt_beam_stream_drain(int B, int max_total_frames, int beam, const void *workspace, size_t workspace_bytes,
                                const int32_t *from, int ld, int32_t *out_tokens, int32_t *out_len, double *out_score,
                                int32_t *out_count, int32_t *out_committed, int32_t *out_overflow, pafc_stream_t stream);

/* The LSTM state of the survivors, in one launch and in place: for h and for c, both (num_layers, n = B * beam, hidden)
 * contiguous of `dtype`, h[l, i, :] = (next_idx[i] < n ? h : h_new)[l, next_idx[i] mod n, :] -- what
 * torch.cat([h, h_new], 1).index_select(1, next_idx) copied back into h computes, bit for bit.  A slot only ever references
 * slots of its own utterance (next_idx of pafc_rnnt_beam_step / _stream_step), and a thread owns the same columns of all the
 * utterance's slots: it reads every row it needs before it writes any.  An index outside [0, 2 n) keeps the slot as it is. */
int pafc_rnnt_beam_select_state(int dtype, int num_layers, int B, int beam, int hidden, void *h, void *c, const void *h_new,
                                const void *c_new, const int64_t *next_idx, pafc_stream_t stream);

/* RNN-T greedy search (basic_greedy_search, wenet/transducer/search/greedy_search.py) for B utterances at once, in lockstep:
 * each pafc_rnnt_greedy_step advances every running utterance by one decision -- the LSTM predictor (only for rows whose
 * last decision was not blank), projection, pred_ffn, the joint reduced to per-slice softmax statistics, argmax (lowest index
 * on ties) and the state machine: a non-blank is emitted with its frame and commits the pending LSTM state; a blank, or the
 * n_steps-th symbol of a frame, moves to the next frame; a blank also keeps the predictor's output for the next decision.
 * All state lives in `workspace`; a step reads nothing from the host, allocates nothing and copies nothing, so it can be
 * captured in a graph.  The path score of a row is the sum of log p(decision) over all its decisions (blanks included),
 * accumulated in float64.
 * net: the weights, every one of them contiguous in nn.Module layout and of net->dtype (PAFC_F32: exact fp32 products and
 * fp32 accumulation; PAFC_BF16: bf16 operands, fp32 accumulation, the LSTM state, pred_out, P, E + P and tanh rounded to
 * bf16).  Dimensions multiples of 4, join_dim <= 2048, embed_rows >= vocab, 16-byte aligned weights; b_ih / b_hh may be
 * NULL (no bias) and so may proj_b, pred_ffn_b, out_b.  The pointer arrays w_ih .. b_hh are host memory.
 * E: (B, T, join_dim) of net->dtype, enc_ffn(encoder_out).  lens: (B) int64 device frames per utterance (clamped to [0, T]).
 * B <= 256, T * n_steps < 2^31.  running (device int32, or NULL): receives the number of rows still running after the step.
 * pafc_rnnt_greedy_finish writes, for row b, ntok[b] and the first min(ntok[b], ld) tokens and their frame indices into row
 * b of tokens / frames ((B, ld) int32; frames may be NULL), score[b] (or NULL) and the running count. */
typedef struct pafc_rnnt_greedy_net {
    int dtype;
    int num_layers, embed_dim, hidden, pred_dim, join_dim, vocab, embed_rows;
    const void *embed;                         /* (embed_rows, embed_dim) */
    const void *const *w_ih;                   /* num_layers x (4 hidden, embed_dim for layer 0 else hidden): gates i, f, g, o */
    const void *const *w_hh;                   /* num_layers x (4 hidden, hidden) */
    const void *const *b_ih, *const *b_hh;     /* num_layers x (4 hidden), or NULL */
    const void *proj_w, *proj_b;               /* (pred_dim, hidden), (pred_dim) */
    const void *pred_ffn_w, *pred_ffn_b;       /* (join_dim, pred_dim), (join_dim) */
    const void *out_w, *out_b;                 /* (vocab, join_dim), (vocab) */
} pafc_rnnt_greedy_net;

size_t pafc_rnnt_greedy_workspace_bytes(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps);
int pafc_rnnt_greedy_init(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps, int blank_id, const int64_t *lens,
                          void *workspace, size_t workspace_bytes, pafc_stream_t stream);
int pafc_rnnt_greedy_step(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps, int blank_id, const void *E, void *workspace,
                          size_t workspace_bytes, int32_t *running, pafc_stream_t stream);
int pafc_rnnt_greedy_finish(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps, const void *workspace, size_t workspace_bytes,
                            int ld, int32_t *tokens, int32_t *frames, int32_t *ntok, double *score, int32_t *running,
                            pafc_stream_t stream);

/* The frame body of the CTC-fused RNN-T prefix beam search as kernels (csrc/rnnt_beam_body.hip): for the n = B * beam slots,
 * what the framework ops in front of pafc_rnnt_beam_step / _stream_step compute -- predictor step, joint, log-softmax, fusion
 * with the CTC row and top-`beam` -- in num_layers + 4 launches, the big products on the matrix cores.  Per slot s of
 * utterance b = s / beam, at frame f = clamp(t_dev ? *t_dev : t, 0, T - 1):
 *   x = embed[last_tok[s]]; the LSTM layers (gates i, f, g, o) from (h, c)[:, s] into (h_new, c_new)[:, s]; projection;
 *   P = pred_ffn(.); z = out_w tanh(E[b, f] + P) + out_b; lse = logsumexp(z);
 *   score_v = log(w_rnnt exp(z_v - lse) + w_ctc exp(ctc[b, f, v])) in fp32;
 *   top_val / top_idx[s, :] = the `beam` largest scores, descending, ties to the lowest token id.
 * net: pafc_rnnt_greedy_net above, with its rounding points (PAFC_F32: exact fp32 products, fp32 accumulation; PAFC_BF16:
 * bf16 operands, fp32 accumulation, LSTM state, pred_out, P, E + P and tanh rounded to bf16; z and the scores stay fp32).
 * E: (B, T, join_dim) of net->dtype, enc_ffn(encoder_out).  ctc: (B, T, ldc >= vocab) log-probabilities of ctc_dtype (PAFC_F32
 * or PAFC_BF16), read in place.  h, c, h_new, c_new: (num_layers, n, hidden) of net->dtype, 16-byte aligned, h_new / c_new
 * distinct from h / c.  last_tok: (n) int64 (clamped to the embedding's rows).  top_val float32 / top_idx int64: (B, beam, beam),
 * as pafc_rnnt_beam_step takes them.  Rows whose utterance has ended are computed like any other: the walk ignores them.
 * beam <= 16, vocab >= beam, B * beam <= 4096, else PAFC_ERR_UNSUPPORTED (workspace_bytes: 0).  workspace: 256-byte aligned,
 * pafc_rnnt_beam_body_workspace_bytes(net, B, beam) bytes: pred_out, the joint's input and the n x vocab fp32 logits.
 * Nothing reads the host or allocates, no atomics: a frame can be captured in a graph and two calls give the same bits. */
size_t pafc_rnnt_beam_body_workspace_bytes(const pafc_rnnt_greedy_net *net, int B, int beam);
int pafc_rnnt_beam_body(const pafc_rnnt_greedy_net *net, int B, int T, int beam, int t, const int64_t *t_dev, const void *E,
                        int ctc_dtype, const void *ctc, long ldc, float w_rnnt, float w_ctc, const int64_t *last_tok,
                        const void *h, const void *c, void *h_new, void *c_new, float *top_val, int64_t *top_idx, void *workspace,
                        size_t workspace_bytes, pafc_stream_t stream);
/* *t_dev += 1 (device int64), for the end of a captured frame: body, step, select_state, advance. */
int pafc_rnnt_beam_body_advance(int64_t *t_dev, pafc_stream_t stream);

/* RNN-T greedy search chunk by chunk, with the decoder state carried from one chunk to the next (pafc_rnnt_greedy_stream_*).
 * The stream workspace begins with the pafc_rnnt_greedy_* layout for (B, T = Tmax), followed by an int64 frame base per row,
 * so pafc_rnnt_greedy_step(net, B, Tmax, n_steps, blank_id, E, workspace, ...) advances it, E being a fixed (B, Tmax, join_dim)
 * buffer that holds enc_ffn of the current chunk.  A row leaves a chunk at a frame boundary, holding the state the
 * whole-utterance decode holds there, so the decisions over a stream of chunks are those of the decode of the concatenated
 * frames, given the same E rows.
 * reset: restarts the rows with row_mask[b] != 0 (device int32 (B), or NULL = every row): zero committed LSTM state,
 *   predictor input blank, frame base 0, no frames, score 0.  Other rows are untouched.  Call it on every row before the
 *   first feed.
 * feed: begins a chunk: per row the frame base advances by the previous chunk's frame count, the row gets
 *   clamp(nframes[b], 0, Tmax) frames of E (nframes: device int64 (B)), and its per-chunk token count is zeroed; the LSTM
 *   state, predictor input and output, symbols of the current frame and score carry over.  A row with no frames keeps its
 *   state.  running (device int32, or NULL) receives the number of rows with frames.  Then pafc_rnnt_greedy_step until no
 *   row is running.
 * drain: per row the tokens emitted since the last feed (ntok[b], first min(ntok[b], ld) of them into row b of tokens
 *   (B, ld) int32), their absolute frame indices (frame base + frame in the chunk, (B, ld) int64, may be NULL) and the
 *   path score since the row's reset (float64 (B), may be NULL).
 * Nothing reads the host or allocates: a feed and its steps can be captured in a graph.  B <= 256, Tmax * n_steps < 2^31,
 * 256-byte aligned workspace. */
size_t pafc_rnnt_greedy_stream_workspace_bytes(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps);
int pafc_rnnt_greedy_stream_reset(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps, int blank_id, const int32_t *row_mask,
                                  void *workspace, size_t workspace_bytes, pafc_stream_t stream);
int pafc_rnnt_greedy_stream_feed(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps, int blank_id, const int64_t *nframes,
                                 void *workspace, size_t workspace_bytes, int32_t *running, pafc_stream_t stream);
int pafc_rnnt_greedy_stream_drain(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps, const void *workspace,
                                  size_t workspace_bytes, int ld, int32_t *tokens, int64_t *frames, int32_t *ntok, double *score,
                                  int32_t *running, pafc_stream_t stream);

/* Full-sum transducer score log p(y | x) of n-best lists (the second pass of transducer_attention_rescoring,
 * wenet/transducer/transducer.py:185-210, without its beam-fold repeat of the encoder output): the hypotheses of one utterance
 * are scored over the trie of their prefixes.  A lattice column ("arc") of utterance b is (node, label) for every child edge of
 * a trie node, or (node, none) for a node without children; K_b arcs.  Rows are (b, t, k): r = off_b + t K_b + k, off_b the rows
 * of the group's earlier utterances.  h_r = bf16(tanh(E[enc_b, t] + Pnode[prow_k])) (add and tanh in fp32, one rounding),
 * z_r = W h_r + bias accumulated in fp32, never rounded, never stored; per row lse, z[blank] and z[label_k] -- the rounding points
 * and the kernels (join, stats epilogue, lse) of pafc_rnnt_joint_loss_forward.  Then one block per hypothesis runs that forward's
 * alpha recurrence (fp32, "log 0" = -1e30, lse2(alpha(t-1, u) + lp_blank, alpha(t, u-1) + lp_label)) with lp_blank / lp_label of
 * (t, u) read from column col[n][u], and score[n] = alpha(T_b - 1, U_n) + lp_blank(T_b - 1, U_n): bit for bit -nll of
 * pafc_rnnt_joint_loss_forward fed that hypothesis alone (its encoder rows, its own predictor rows, its labels).  U_n > T_b is fine.
 * E: (Benc, T, J) bf16 in rows of lde, utterances strideE apart, passed once per utterance.  Pnode: (prows, J) bf16 in rows of
 * ldp: pred_ffn of the predictor's output after each prefix.  W (V, J), bias (V) or NULL: bf16.  hlens: (Benc) device int32 frames, or
 * NULL when the caller built the tables from lengths it holds on the host (then T_b is taken as it is).
 * The tables: one int32 array, given twice -- tab_host for validation and sizing, tab_dev (the same values on the device) for the
 * kernels, as pafc_fbank_stream_rows takes its rows -- laid out as
 *   utt_enc (nutt): the row of E / hlens of utterance b (several utterances may share one: every hypothesis its own utterance
 *     scores without sharing);  utt_T (nutt): its frames T_b;  arc_off, hyp_off (nutt + 1 each): its first arc / hypothesis;
 *   arc_prow, arc_label (narc each): the row of Pnode of the arc's node, and its label or -1;
 *   hyp_utt, hyp_len (nhyp each): utterance and U_n;  col_off (nhyp + 1);  col (ncol): col_off[n] + u holds the column, in
 *     [0, K_b), of position u <= U_n -- for u < U_n the arc (y[:u], y[u]), for u = U_n any arc of node y[:U_n].
 * One call scores the utterances [utt0, utt1) and writes score[hyp_off[utt0] .. hyp_off[utt1]) of score (nhyp) fp32; the caller
 * bounds the workspace by cutting the batch into such groups.  Before anything is launched the group's tables are checked on the
 * host copy: offsets monotonic and inside the arrays, utt_enc in [0, Benc), T_b in [1, T], prow in [0, prows), labels in [-1, V),
 * columns in [0, K_b) and labelled where u < U_n, else PAFC_ERR_BAD_DIMS.  A hypothesis whose utterance has hlens[enc_b] != T_b on
 * the device (a length outside E, or not the one the tables were built from) gets NaN.  Limits of the training forward: J % 64 == 0, V % 8 == 0, U_n + 1 <= 2559, nutt <= 65535, else
 * PAFC_ERR_UNSUPPORTED; lde, strideE, ldp multiples of 8, E / Pnode / W 16-byte and the workspace 256-byte aligned, else
 * PAFC_ERR_ALIGNMENT.  workspace: pafc_rnnt_score_workspace_bytes(utt1 - utt0, J, V, rows of the group) bytes
 * (rows x (2 J + 8 ceil(V / 128) + 16) and the offsets).  No float atomics, nothing reads the host or allocates after the checks:
 * two calls give the same bits. */
size_t pafc_rnnt_score_workspace_bytes(int nutt, int J, int V, long rows);
int pafc_rnnt_score(int Benc, int T, int J, int V, const void *E, long lde, long strideE, const void *Pnode, long ldp, long prows,
                    const void *W, const void *bias, const int32_t *hlens, int nutt, int nhyp, int narc, int ncol,
                    const int32_t *tab_host, const int32_t *tab_dev, int utt0, int utt1, int blank, float *score, void *workspace,
                    size_t workspace_bytes, pafc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
