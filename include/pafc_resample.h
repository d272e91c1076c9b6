/*
 * pafc_resample.h -- C ABI of the sample-rate converter in front of the fbank on gfx950.
 *
 * Replaces the reference's `resample` processor, wenet/dataset/processor.py:294-313, which calls a third-party CPU routine,
 *   torchaudio.transforms.Resample(orig_freq, new_freq)      (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).
 * With g = gcd(f_in, f_out), orig = f_in / g, new_ = f_out / g, base = min(orig, new_) * 0.99 and W = ceil(6 orig / base)
 * the filter has new_ phases of 2 W + orig taps k[i][j], and with x zero outside [0, S)
 *   y[m new_ + i] = sum_j k[i][j] x[m orig - W + j],   0 <= m new_ + i < N = pafc_resample_num_out(S, orig, new_).
 * Every tap whose argument the definition clamps is exactly zero, so the caller hands over a COMPACT table (device
 * pointers; the library holds no state): first (new_) int32, the first kept tap of a phase, and coef (new_, span) float32,
 * the taps first[i] .. first[i] + span - 1 of phase i, with 0 <= first[i] <= 2 W + orig - span (a value outside is clamped
 * in the kernel).  An output is ONE fma chain over the span kept taps in ascending order, from 0.0f, in every entry point
 * below: a batch, a stream cut into any packets and a slot pool give the same bits per output sample.
 *
 * Limits (PAFC_ERR_UNSUPPORTED outside them, nothing is launched): orig + 2 W <= PAFC_RESAMPLE_MAX_CARRY, and the two
 * buffers a block stages in LDS, min(new_, 1024) phases of the table and the input span of 1024 outputs, <= 64 KiB each.
 *
 * pafc_resample_batch: B rows of waves (B, ld_wave >= max_samples) in ONE launch, grid (ceil(N_max / 1024), B),
 *   N_max = pafc_resample_num_out(max_samples, orig, new_).  lengths: device int64 (B) sample counts, clamped to
 *   [0, max_samples] in the kernel, or NULL (every row max_samples).  out: (B, ld_out >= N_max) float32: row b's first N_b
 *   samples, zeros in [N_b, N_max).  out_lengths: device int64 (B) that receives N_b, or NULL.  No host synchronisation.
 *
 * pafc_resample_stream_plan: a stream's device state is a carry of c <= orig + 2 W input samples that starts as W zeros
 *   (the left padding).  With n new samples, A = c + n: frames = A >= 2 W + orig ? (A - 2 W - orig) / orig + 1 : 0 whole
 *   frames of new_ outputs are released (*n_out = frames * new_) and *c_next = A - frames * orig samples are carried on.
 *
 * pafc_resample_rows: R ragged rows over a pool of S carries (S, ld_carry >= orig + 2 W), in one launch pair.  Row i's
 *   descriptor is five int32 {slot, c, n, n_out, c_next}: its samples are z = carry[slot, 0:c] followed by chunk[i, 0:n]
 *   (chunk: (R, ld_chunk >= n_max)), zero behind that; out[i, o] = sum_t coef[o % new_][t] z[(o / new_) orig + first + t]
 *   for 0 <= o < n_out (out: (R, ld_out >= every n_out)); a second small kernel on the same stream then moves the last
 *   c_next <= c + n samples of z to the front of carry[slot].  n_out is the plan's value for a packet inside a stream, and
 *   N - (outputs so far) with c_next = 0 for the last packet, whose trailing outputs see zeros behind the last sample.
 *   Lock-step streams are the case slot = row.  The table is passed twice: rows is the HOST copy, which is validated and
 *   sizes the grid, rows_dev the device copy the kernels read (uploaded by the caller on `stream`).  The slots of a call
 *   are distinct; a row with n == 0 and n_out == 0 does nothing; the carries of slots not named are not touched; a call
 *   in which no row has an output launches only the carry update, one in which no row does anything launches nothing.
 *   Both launches can be captured.
 */
#ifndef PAFC_RESAMPLE_H
#define PAFC_RESAMPLE_H

#include "pafc_wkv6.h"

#define PAFC_RESAMPLE_MAX_CARRY 4096

#ifdef __cplusplus
extern "C" {
#endif

long pafc_resample_num_out(long n_in, int orig, int new_);
int pafc_resample_stream_plan(int orig, int new_, int W, int c, long n, long *n_out, int *c_next);
int pafc_resample_batch(const float *waves, long ld_wave, const long *lengths, int B, long max_samples, int orig, int new_,
                        int W, const int *first, const float *coef, int span, float *out, long ld_out, long *out_lengths,
                        pafc_stream_t stream);
int pafc_resample_rows(float *carry, long ld_carry, int S, const int *rows, const int *rows_dev, int R, const float *chunk,
                       long ld_chunk, long n_max, int orig, int new_, int W, const int *first, const float *coef, int span,
                       float *out, long ld_out, pafc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PAFC_RESAMPLE_H */
