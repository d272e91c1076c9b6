/*
 * pafc_fbank.h -- C ABI of the Kaldi-compatible 80-bin log-mel filterbank on gfx950.
 *
 * Replaces the reference's call into a third-party CPU routine,
 *   torchaudio.compliance.kaldi.fbank(waveform, num_mel_bins=80, frame_length=25, frame_shift=10,
 *                                     dither=0|1, energy_floor=0.0, sample_frequency=16000)
 * at wenet/dataset/processor.py:363-369, wenet/bin/encoder-rtf.py:575-583, wenet/bin/recognize_wav2.py:510-518
 * (all other arguments at torchaudio's defaults: snip_edges, remove_dc_offset, preemphasis 0.97, povey window,
 * round_to_power_of_two -> 512-point FFT, power spectrum, low_freq 20 Hz, high_freq Nyquist, log with float-eps
 * floor).  Frame geometry is fixed to that configuration: 400-sample window, 160-sample shift.
 *
 * The constant tables are supplied by the caller (device pointers), so the library holds no state:
 *   window      (400)          povey window
 *   dft_table   (400, cols)    cols = pafc_fbank_tables_cols(); column 2k = cos(2 pi k n / 512),
 *                              column 2k+1 = -sin(2 pi k n / 512) for k = 0..256, remaining columns zero
 *   mel_weights (num_mel_bins, 257), mel_lo / mel_hi (num_mel_bins): filter b is non-zero on bins [lo, hi)
 * wave: (num_samples) float32 in int16 range; noise: (frames, 400) standard normal or NULL (dither off);
 * out: (frames, num_mel_bins) float32, frames = pafc_fbank_num_frames(num_samples) = 1 + (S - 400) / 160.
 *
 * Every frame is computed from its own 400 samples alone, so the batched and the streaming entry points below give, frame by
 * frame, the bits pafc_fbank_f32 gives for the same samples.
 *
 * pafc_fbank_batch: B waveforms as the rows of waves (B, ld_wave >= max_samples) in ONE launch, grid (ceil(T_max / 64), B).
 *   lengths: device int64 (B) sample counts, clamped to [0, max_samples] in the kernel, or NULL (every row max_samples).
 *   out: (B, T_max, num_mel_bins), T_max = pafc_fbank_num_frames(max_samples), PAFC_F32 or PAFC_BF16 (round-to-nearest-even of
 *   the fp32 value); frames of a row at or past its own frame count are written as ZERO.  out_frames: device int32 (B) that
 *   receives every row's frame count, or NULL.  noise: (B, T_max, 400) or NULL.  No host synchronisation.
 *
 * pafc_fbank_stream: B lock-step streams.  Row b's samples are carry[b, 0:c] followed by chunk[b, 0:n] (carry: (B, 560)
 *   float32, 0 <= c < 560; chunk: (B, ld_chunk >= n)).  frames = pafc_fbank_num_frames(c + n) frames per row are written at
 *   out + row * out_row_stride + (first_frame + f) * num_mel_bins (strides in elements of out_dtype), and a second small kernel
 *   on the same stream then moves the last c_next = c + n - 160 * frames samples to the front of carry[b], in place.
 *   frames == 0 launches only that update, n == 0 launches nothing; both launches can be captured.  pafc_fbank_stream_plan is
 *   the arithmetic (frames, c_next) on the host, c_next < 560 always.  dither != 0 is PAFC_ERR_UNSUPPORTED here.
 *
 * pafc_fbank_stream_rows: R ragged rows that belong to arbitrary slots of a pool of S independent streams, in one launch
 *   pair, grid (tiles of the row with the most frames, R).  carry: (S, 560) float32; chunk: (R, ld_chunk >= n_max); row i's
 *   descriptor is four int32 {slot, c, n, first_frame}: its samples are carry[slot, 0:c] followed by chunk[i, 0:n]
 *   (0 <= c < 560, 0 <= n <= n_max), and its frame f is written at out[slot, (first_frame + f) mod ring_frames, :]
 *   (out: (S, ring_frames, num_mel_bins) contiguous, PAFC_F32 or PAFC_BF16; first_frame: the absolute index of the row's first
 *   new frame).  The table is passed twice: rows is the HOST copy, which is validated and sizes the grid, rows_dev the
 *   device copy the kernels read (uploaded by the caller on `stream`), so nothing is ever read back.  The slots of a call are
 *   distinct, and a row completes at most ring_frames frames (the caller cuts a longer packet).  The second kernel moves the
 *   last c + n - 160 * frames samples of every row with n > 0 to the front of carry[slot].  Rows with n == 0 do nothing; a
 *   call in which no row completes a frame launches only the carry update; a call without a new sample launches nothing.
 *   The carries and rings of slots not named are not touched.  dither != 0 is PAFC_ERR_UNSUPPORTED.
 */
#ifndef PAFC_FBANK_H
#define PAFC_FBANK_H

#include "pafc_wkv6.h"

#ifdef __cplusplus
extern "C" {
#endif

long pafc_fbank_num_frames(long num_samples);
int pafc_fbank_tables_cols(void);
int pafc_fbank_f32(const float *wave, long num_samples, const float *window, const float *dft_table,
                   const float *mel_weights, const int *mel_lo, const int *mel_hi, int num_mel_bins,
                   const float *noise, float dither, float preemph, float *out, pafc_stream_t stream);
int pafc_fbank_batch(const float *waves, long ld_wave, const long *lengths, int B, long max_samples, const float *window,
                     const float *dft_table, const float *mel_weights, const int *mel_lo, const int *mel_hi, int num_mel_bins,
                     const float *noise, float dither, float preemph, void *out, int out_dtype, int *out_frames,
                     pafc_stream_t stream);
int pafc_fbank_stream_plan(int c, long n, long *frames, int *c_next);
int pafc_fbank_stream(float *carry, int c, const float *chunk, long ld_chunk, long n, int B, const float *window,
                      const float *dft_table, const float *mel_weights, const int *mel_lo, const int *mel_hi, int num_mel_bins,
                      float dither, float preemph, void *out, int out_dtype, long out_row_stride, long first_frame,
                      pafc_stream_t stream);
int pafc_fbank_stream_rows(float *carry, int S, const int *rows, const int *rows_dev, int R, const float *chunk, long ld_chunk,
                           long n_max, const float *window, const float *dft_table, const float *mel_weights, const int *mel_lo,
                           const int *mel_hi, int num_mel_bins, float dither, float preemph, void *out, int out_dtype,
                           int ring_frames, pafc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PAFC_FBANK_H */
