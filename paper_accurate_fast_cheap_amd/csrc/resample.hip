// Sample-rate conversion in front of the fbank on gfx950 (C ABI: include/pafc_resample.h).
//
// Replaces torchaudio.transforms.Resample as the reference's `resample` processor calls it (wenet/dataset/processor.py:294-313):
// a polyphase FIR of new_ phases, output m new_ + i = sum_j k[i][j] x[m orig - W + j].  The work is ~2 * 6 * max(1, orig / new_)
// FMAs per output on inputs that neighbouring outputs share almost entirely, so the kernel is bound by memory and launches.
//
// One 256-thread block = 1024 consecutive outputs of one row.  It stages (1) the phases its outputs use of the compact table
// (first[], coef[][span]; row stride span | 1, so that lanes on consecutive phases read different banks) and (2) the input span
// of its outputs, with coalesced loads through a fetch functor that answers zero outside the row's samples, in LDS; then every
// thread computes four outputs, 256 apart, so that the stores of a wave are contiguous.
//
// An output is resample_dot: ONE fma chain over the span kept taps, ascending, from 0.0f.  The three kernels differ in where a
// sample lies (a row of a batch shifted by the left padding W; a carry followed by a chunk) and in nothing else, so a batch, a
// stream cut into any packets and a slot pool give the same bits per output.
#include "pafc_common.h"
#include "resample_host.h"

namespace pafc {
namespace {

using resample_host::TILE;
using resample_host::DESC;
constexpr int NT = 256;

struct ResampleTable {
    int orig, nw, W, span;
    const int *first;       // (nw)
    const float *coef;      // (nw, span)
};

__device__ __forceinline__ float resample_dot(const float *k, const float *z, const int span) {
    float acc = 0.0f;
    for (int t = 0; t < span; ++t) acc = fmaf(k[t], z[t], acc);
    return acc;
}

// Outputs [o0, o0 + TILE) of a row of which [0, n_live) exist.  z(q): sample q of the row's padded signal, in which the
// window of output frame m starts at q = m orig; asked for any q >= 0, answers zero where the row has no sample.
// emit(o, value) is called for o0 <= o < min(o0 + TILE, n_live).  Called by whole blocks with o0 < n_live.
template <class Fetch, class Emit>
__device__ __forceinline__ void resample_tile(const ResampleTable &t, const long o0, const long n_live, Fetch z, Emit emit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int krows = resample_host::table_rows(t.nw), ldk = resample_host::table_ld(t.span);
    float *Ks = lds;                                   // [krows][ldk]
    int *Fs = (int *)(lds + (long)krows * ldk);        // [krows]
    float *Zs = lds + (long)krows * ldk + krows;       // the input span
    const int taps = 2 * t.W + t.orig;
    const long last = (o0 + TILE < n_live ? o0 + TILE : n_live) - 1;
    const long m0 = o0 / t.nw, m1 = last / t.nw;
    const int i0 = (int)(o0 - m0 * t.nw);
    const int zlen = (int)(m1 - m0) * t.orig + taps;   // <= resample_host::input_span
    const long q0 = m0 * t.orig;

    for (int u = tid; u < zlen; u += NT) Zs[u] = z(q0 + u);
    // LDS row r holds phase (i0 + r) mod nw: output o0 + l uses row l mod nw
    for (int r = tid; r < krows; r += NT) {
        int i = i0 + r;
        i -= i >= t.nw ? t.nw : 0;
        const int f = t.first[i];
        Fs[r] = f < 0 ? 0 : (f > taps - t.span ? taps - t.span : f);
    }
    for (int u = tid; u < krows * t.span; u += NT) {
        const int r = u / t.span, c = u - r * t.span;
        int i = i0 + r;
        i -= i >= t.nw ? t.nw : 0;
        Ks[r * ldk + c] = t.coef[(long)i * t.span + c];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < TILE / NT; ++e) {
        const int l = tid + NT * e;
        const long o = o0 + l;
        if (o <= last) {
            const int r = l % t.nw;
            const int m = (i0 + l) / t.nw;             // frames past m0
            emit(o, resample_dot(Ks + r * ldk, Zs + m * t.orig + Fs[r], t.span));
        }
    }
}

// Rows of a batch: grid (tiles, B).  Row b's samples are wave[b, 0:len]; its padded signal has W zeros in front.
__global__ __launch_bounds__(NT) void resample_batch_kernel(const ResampleTable t, const float *waves, const long ld_wave,
                                                            const long *lens, const long max_samples, const long n_max_out,
                                                            float *out, const long ld_out, long *out_lens) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const long o0 = (long)blockIdx.x * TILE;
    long len = max_samples;
    if (lens) {
        const long v = lens[b];
        len = v < 0 ? 0 : (v > max_samples ? max_samples : v);
    }
    const long N = resample_host::num_out(len, t.orig, t.nw);           // <= n_max_out
    if (o0 == 0 && tid == 0 && out_lens) out_lens[b] = N;
    float *dst = out + (long)b * ld_out;
    const long end = o0 + TILE < n_max_out ? o0 + TILE : n_max_out;
    if (o0 < N) {                                                       // block-uniform
        const float *row = waves + (long)b * ld_wave;
        const long W = t.W;
        resample_tile(t, o0, N, [&](long q) { const long p = q - W; return p >= 0 && p < len ? row[p] : 0.0f; },
                      [&](long o, float v) { dst[o] = v; });
    }
    for (long o = (o0 > N ? o0 : N) + tid; o < end; o += NT) dst[o] = 0.0f;   // behind the row's own N
}

// Ragged rows of a slot pool: grid (tiles of the row with the most outputs, R).  Row i's descriptor is rows[5 i ..] =
// {slot, c, n, n_out, c_next}; its padded signal is carry[slot, 0:c] ++ chunk[i, 0:n] ++ zeros.
__global__ __launch_bounds__(NT) void resample_rows_kernel(const ResampleTable t, const float *carry, const long ld_carry,
                                                           const int *rows, const float *chunk, const long ld_chunk, float *out,
                                                           const long ld_out) {
    const int *d = rows + DESC * blockIdx.y;
    const int slot = d[0], c = d[1], n = d[2], n_out = d[3];
    const long o0 = (long)blockIdx.x * TILE;
    if (o0 >= n_out) return;                                            // block-uniform, before any barrier
    const float *car = carry + (long)slot * ld_carry;
    const float *row = chunk + (long)blockIdx.y * ld_chunk;
    float *dst = out + (long)blockIdx.y * ld_out;
    resample_tile(t, o0, n_out, [&](long q) { return q < c ? car[q] : (q - c < n ? row[q - c] : 0.0f); },
                  [&](long o, float v) { dst[o] = v; });
}

// carry[slot, 0:c_next] <- the last c_next samples of (carry[slot, 0:c] ++ chunk[i, 0:n]) per row of the table.  Source and
// destination overlap: one block per row reads its <= PAFC_RESAMPLE_MAX_CARRY samples into LDS, barriers, then writes.
__global__ __launch_bounds__(NT) void resample_carry_kernel(float *carry, const long ld_carry, const int *rows, const float *chunk,
                                                            const long ld_chunk) {
    __shared__ float keep[PAFC_RESAMPLE_MAX_CARRY];
    const int *d = rows + DESC * blockIdx.x;
    const int slot = d[0], c = d[1], n = d[2], n_out = d[3];
    int c_next = d[4];
    if (n == 0 && n_out == 0) return;                                   // block-uniform
    c_next = c_next > PAFC_RESAMPLE_MAX_CARRY ? PAFC_RESAMPLE_MAX_CARRY : c_next;
    float *car = carry + (long)slot * ld_carry;
    const float *row = chunk + (long)blockIdx.x * ld_chunk;
    const long from = (long)c + n - c_next;                             // >= 0 (checked on the host)
    for (int j = threadIdx.x; j < c_next; j += NT) {
        const long s = from + j;
        keep[j] = s < c ? car[s] : row[s - c];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < c_next; j += NT) car[j] = keep[j];
}

template <class K>
bool allow_lds(K kernel) {
    // > 64 KiB of dynamic LDS needs the attribute; it is per device and idempotent, so set it on every call
    return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
}

}  // namespace
}  // namespace pafc

extern "C" {

long pafc_resample_num_out(long n_in, int orig, int new_) {
    if (orig <= 0 || new_ <= 0 || n_in > 0x7fffffffffffL / new_) return 0;
    return pafc::resample_host::num_out(n_in, orig, new_);
}

int pafc_resample_stream_plan(int orig, int new_, int W, int c, long n, long *n_out, int *c_next) {
    return pafc::resample_host::stream_plan(orig, new_, W, c, n, n_out, c_next);
}

int pafc_resample_batch(const float *waves, long ld_wave, const long *lengths, int B, long max_samples, int orig, int new_,
                        int W, const int *first, const float *coef, int span, float *out, long ld_out, long *out_lengths,
                        pafc_stream_t stream) {
    long N = 0;
    const int rc = pafc::resample_host::batch_check(waves, ld_wave, B, max_samples, orig, new_, W, first, coef, span, out,
                                                    ld_out, &N);
    if (rc != PAFC_OK) return rc;
    if (!pafc::allow_lds(pafc::resample_batch_kernel)) return PAFC_ERR_LAUNCH;
    const pafc::ResampleTable t{orig, new_, W, span, first, coef};
    const unsigned tiles = (unsigned)((N + pafc::TILE - 1) / pafc::TILE);
    hipLaunchKernelGGL(pafc::resample_batch_kernel, dim3(tiles, (unsigned)B), dim3(pafc::NT),
                       (size_t)pafc::resample_host::lds_bytes(orig, new_, W, span), (hipStream_t)stream, t, waves, ld_wave, lengths,
                       max_samples, N, out, ld_out, out_lengths);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_resample_rows(float *carry, long ld_carry, int S, const int *rows, const int *rows_dev, int R, const float *chunk,
                       long ld_chunk, long n_max, int orig, int new_, int W, const int *first, const float *coef, int span,
                       float *out, long ld_out, pafc_stream_t stream) {
    long most = 0;
    bool any = false;
    const int rc = pafc::resample_host::rows_check(carry, ld_carry, S, rows, rows_dev, R, chunk, ld_chunk, n_max, orig, new_, W,
                                                   first, coef, span, out, ld_out, &most, &any);
    if (rc != PAFC_OK || !any) return rc;
    if (most > 0) {
        if (!pafc::allow_lds(pafc::resample_rows_kernel)) return PAFC_ERR_LAUNCH;
        const pafc::ResampleTable t{orig, new_, W, span, first, coef};
        const unsigned tiles = (unsigned)((most + pafc::TILE - 1) / pafc::TILE);
        hipLaunchKernelGGL(pafc::resample_rows_kernel, dim3(tiles, (unsigned)R), dim3(pafc::NT),
                           (size_t)pafc::resample_host::lds_bytes(orig, new_, W, span), (hipStream_t)stream, t, carry, ld_carry,
                           rows_dev, chunk, ld_chunk, out, ld_out);
        if (hipGetLastError() != hipSuccess) return PAFC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(pafc::resample_carry_kernel, dim3((unsigned)R), dim3(pafc::NT), 0, (hipStream_t)stream, carry, ld_carry,
                       rows_dev, chunk, ld_chunk);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

}  // extern "C"
