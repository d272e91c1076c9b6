// Host-only arithmetic and argument checks of the fbank entry points (include/pafc_fbank.h): plain C++ without a HIP
// header, so that fbank.hip and a stand-alone host program (tools/fbank_host_check.cpp, built with sanitizers) share one
// statement of them.
#pragma once
#include "../../include/pafc_fbank.h"

namespace pafc {
namespace fbank_host {

constexpr int WIN = 400, SHIFT = 160;
constexpr int CARRY = WIN + SHIFT;   // row length of a stream's carry: it never holds more than WIN + SHIFT - 1 samples
constexpr int MAXMEL = 128;
constexpr long MAXROWS = 65535;      // grid y

constexpr long num_frames(long num_samples) { return num_samples < WIN ? 0 : 1 + (num_samples - WIN) / SHIFT; }

// c carried samples + n new ones -> frames completed, samples carried on (the tail no frame has left behind yet)
inline int stream_plan(int c, long n, long *frames, int *c_next) {
    if (c < 0 || c >= CARRY || n < 0) return PAFC_ERR_BAD_DIMS;
    const long f = num_frames(c + n);
    if (f > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    if (frames) *frames = f;
    if (c_next) *c_next = (int)(c + n - SHIFT * f);
    return PAFC_OK;
}

inline bool tables_null(const void *window, const void *dft, const void *melw, const void *lo, const void *hi) {
    return !window || !dft || !melw || !lo || !hi;
}

// -> PAFC_OK and *t_max, or the error
inline int batch_check(const void *waves, long ld_wave, int B, long max_samples, bool tables_are_null, int nmel, const void *out,
                       int out_dtype, long *t_max) {
    if (!waves || tables_are_null || !out) return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || B > MAXROWS || nmel <= 0 || nmel > MAXMEL || ld_wave < max_samples) return PAFC_ERR_BAD_DIMS;
    const long m = num_frames(max_samples);
    if (m <= 0 || m > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    if (out_dtype != PAFC_F32 && out_dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    *t_max = m;
    return PAFC_OK;
}

// -> PAFC_OK and the plan, or the error
inline int stream_check(const void *carry, int c, const void *chunk, long ld_chunk, long n, int B, bool tables_are_null, int nmel,
                        float dither, const void *out, int out_dtype, long out_row_stride, long first_frame, long *frames,
                        int *c_next) {
    if (!carry || tables_are_null) return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || B > MAXROWS || nmel <= 0 || nmel > MAXMEL) return PAFC_ERR_BAD_DIMS;
    const int rc = stream_plan(c, n, frames, c_next);
    if (rc != PAFC_OK) return rc;
    if (dither != 0.f) return PAFC_ERR_UNSUPPORTED;
    if (out_dtype != PAFC_F32 && out_dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (n == 0) return PAFC_OK;
    if (!chunk) return PAFC_ERR_NULL_POINTER;
    if (ld_chunk < n) return PAFC_ERR_BAD_DIMS;
    if (*frames > 0) {
        if (!out) return PAFC_ERR_NULL_POINTER;
        if (first_frame < 0 || first_frame > 0x7fffffffL || out_row_stride < (first_frame + *frames) * nmel) return PAFC_ERR_BAD_DIMS;
    }
    return PAFC_OK;
}

// Ragged rows of a slot pool: rows is the HOST copy of the (R, 4) int32 descriptor table {slot, c, n, first_frame}.
// -> PAFC_OK, *max_frames (the most frames a row completes) and *any_new (some row has n > 0), or the error
inline int stream_rows_check(const void *carry, int S, const int *rows, const void *rows_dev, int R, const void *chunk,
                             long ld_chunk, long n_max, bool tables_are_null, int nmel, float dither, const void *out,
                             int out_dtype, int ring_frames, long *max_frames, bool *any_new) {
    if (!carry || !rows || !rows_dev || tables_are_null) return PAFC_ERR_NULL_POINTER;
    if (S <= 0 || S > MAXROWS || R <= 0 || R > S || nmel <= 0 || nmel > MAXMEL || n_max < 0 || ring_frames <= 0)
        return PAFC_ERR_BAD_DIMS;
    if (dither != 0.f) return PAFC_ERR_UNSUPPORTED;
    if (out_dtype != PAFC_F32 && out_dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    long most = 0;
    bool fresh = false;
    for (int i = 0; i < R; ++i) {
        const int slot = rows[4 * i], c = rows[4 * i + 1], n = rows[4 * i + 2], first = rows[4 * i + 3];
        if (slot < 0 || slot >= S || n > n_max || first < 0) return PAFC_ERR_BAD_DIMS;
        for (int j = 0; j < i; ++j)                    // two rows of one slot would race on its carry and its ring
            if (rows[4 * j] == slot) return PAFC_ERR_BAD_DIMS;
        long f = 0;
        const int rc = stream_plan(c, n, &f, nullptr);
        if (rc != PAFC_OK) return rc;
        if (n == 0) continue;
        if (f > ring_frames || first + f > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
        fresh = true;
        most = f > most ? f : most;
    }
    if (fresh && (!chunk || ld_chunk < n_max)) return chunk ? PAFC_ERR_BAD_DIMS : PAFC_ERR_NULL_POINTER;
    if (most > 0 && !out) return PAFC_ERR_NULL_POINTER;
    *max_frames = most;
    *any_new = fresh;
    return PAFC_OK;
}

}  // namespace fbank_host
}  // namespace pafc
