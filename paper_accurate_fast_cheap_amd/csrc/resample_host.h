// Host-only arithmetic and argument checks of the resampler's entry points (include/pafc_resample.h): plain C++ without a
// HIP header, as fbank_host.h is for the fbank.  The kernels use the same num_out / table_rows / table_ld / input_span, so
// the grid, the LDS size and the indices inside a block come from one statement.
#pragma once
#include "../../include/pafc_resample.h"

namespace pafc {
namespace resample_host {

constexpr int TILE = 1024;             // outputs per block
constexpr long MAXROWS = 65535;        // grid y
constexpr long LDS_CAP = 64 * 1024;    // bytes, for each of the two staged buffers
constexpr int DESC = 5;                // int32 per row descriptor {slot, c, n, n_out, c_next}

constexpr long num_out(long n_in, long orig, long nw) { return n_in <= 0 ? 0 : (nw * n_in + orig - 1) / orig; }

// phases of the table a block stages, and the row stride (odd: lanes on consecutive phases hit different banks)
constexpr int table_rows(int nw) { return nw < TILE ? nw : TILE; }
constexpr int table_ld(int span) { return span | 1; }
// the most input samples the outputs of one block span: its first output is any phase, its last TILE - 1 further on
constexpr long input_span(long orig, long nw, long W) { return ((nw + TILE - 2) / nw) * orig + 2 * W + orig; }

inline long lds_bytes(int orig, int nw, int W, int span) {
    return 4 * ((long)table_rows(nw) * table_ld(span) + table_rows(nw) + input_span(orig, nw, W));
}

// the conversion itself: PAFC_OK, or what is wrong with it
inline int ratio_check(int orig, int nw, int W, int span) {
    if (orig <= 0 || nw <= 0 || W <= 0 || span <= 0) return PAFC_ERR_BAD_DIMS;
    if (W > PAFC_RESAMPLE_MAX_CARRY || orig > PAFC_RESAMPLE_MAX_CARRY) return PAFC_ERR_UNSUPPORTED;
    if (span > 2 * W + orig) return PAFC_ERR_BAD_DIMS;
    if (orig + 2 * W > PAFC_RESAMPLE_MAX_CARRY) return PAFC_ERR_UNSUPPORTED;
    if (4L * table_rows(nw) * table_ld(span) > LDS_CAP || 4 * input_span(orig, nw, W) > LDS_CAP) return PAFC_ERR_UNSUPPORTED;
    return PAFC_OK;
}

inline int stream_plan(int orig, int nw, int W, int c, long n, long *n_out, int *c_next) {
    if (orig <= 0 || nw <= 0 || W <= 0) return PAFC_ERR_BAD_DIMS;
    if (W > PAFC_RESAMPLE_MAX_CARRY || orig > PAFC_RESAMPLE_MAX_CARRY) return PAFC_ERR_UNSUPPORTED;
    const long win = 2L * W + orig;
    if (c < 0 || c > win || n < 0 || n > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    const long A = c + n;
    const long F = A >= win ? (A - win) / orig + 1 : 0;
    if (F * nw > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    if (n_out) *n_out = F * nw;
    if (c_next) *c_next = (int)(A - F * orig);
    return PAFC_OK;
}

// -> PAFC_OK and *n_max_out, or the error
inline int batch_check(const void *waves, long ld_wave, int B, long max_samples, int orig, int nw, int W, const void *first,
                       const void *coef, int span, const void *out, long ld_out, long *n_max_out) {
    if (!waves || !first || !coef || !out) return PAFC_ERR_NULL_POINTER;
    const int rc = ratio_check(orig, nw, W, span);
    if (rc != PAFC_OK) return rc;
    if (B <= 0 || B > MAXROWS || max_samples <= 0 || ld_wave < max_samples) return PAFC_ERR_BAD_DIMS;
    if (max_samples > 0x7fffffffffffL / nw) return PAFC_ERR_BAD_DIMS;
    const long N = num_out(max_samples, orig, nw);
    if (ld_out < N || (N + TILE - 1) / TILE > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    *n_max_out = N;
    return PAFC_OK;
}

// rows: the HOST copy of the (R, 5) descriptor table.  -> PAFC_OK, *most_out (the most outputs of a row) and *any (some
// row brings a sample or has an output), or the error
inline int rows_check(const void *carry, long ld_carry, int S, const int *rows, const void *rows_dev, int R, const void *chunk,
                      long ld_chunk, long n_max, int orig, int nw, int W, const void *first, const void *coef, int span,
                      const void *out, long ld_out, long *most_out, bool *any) {
    if (!carry || !rows || !rows_dev || !first || !coef) return PAFC_ERR_NULL_POINTER;
    const int rc = ratio_check(orig, nw, W, span);
    if (rc != PAFC_OK) return rc;
    const long win = 2L * W + orig;
    if (S <= 0 || S > MAXROWS || R <= 0 || R > S || n_max < 0 || n_max > 0x7fffffffL || ld_carry < win) return PAFC_ERR_BAD_DIMS;
    long most = 0;
    bool fresh = false, some = false;
    for (int i = 0; i < R; ++i) {
        const int *d = rows + DESC * i;
        const int slot = d[0], c = d[1], n = d[2], n_out = d[3], c_next = d[4];
        if (slot < 0 || slot >= S || c < 0 || c > win || n < 0 || n > n_max || n_out < 0 || c_next < 0 || c_next > win ||
            c_next > (long)c + n)
            return PAFC_ERR_BAD_DIMS;
        for (int j = 0; j < i; ++j)                    // two rows of one slot would race on its carry
            if (rows[DESC * j] == slot) return PAFC_ERR_BAD_DIMS;
        if (n == 0 && n_out == 0) continue;
        some = true;
        fresh = fresh || n > 0;
        most = n_out > most ? n_out : most;
    }
    if (fresh && (!chunk || ld_chunk < n_max)) return chunk ? PAFC_ERR_BAD_DIMS : PAFC_ERR_NULL_POINTER;
    if (most > 0 && (!out || ld_out < most)) return out ? PAFC_ERR_BAD_DIMS : PAFC_ERR_NULL_POINTER;
    *most_out = most;
    *any = some;
    return PAFC_OK;
}

}  // namespace resample_host
}  // namespace pafc
