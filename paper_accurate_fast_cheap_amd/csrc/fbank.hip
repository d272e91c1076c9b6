// Kaldi-compatible log-mel filterbank on gfx950 (C ABI: include/pafc_fbank.h).
//
// Replaces torchaudio.compliance.kaldi.fbank as the reference calls it (wenet/dataset/processor.py:363-369,
// wenet/bin/encoder-rtf.py:575-583): 25 ms / 10 ms frames at 16 kHz (400 / 160 samples), snip_edges, optional
// dither, DC removal, pre-emphasis 0.97, povey window, 512-point power spectrum, triangular mel filters, log.
//
// One 256-thread block = 64 frames.  (1) each wave conditions 16 frames (mean, pre-emphasis, window) straight
// from the waveform -- frames overlap by 60 %, so the block touches 10.5 k samples once -- into an LDS tile
// A[64][400] (row stride 401 words: conflict-free column reads).  (2) the 512-point real DFT of all 64 frames is
// one fp32 GEMM A[64x400] x W[400x514] on the matrix cores with v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains;
// the zero-padded tail 400..511 contributes nothing, so K = 400).  W interleaves cos / -sin per bin, which puts
// the real and imaginary part of a bin on adjacent lanes of the accumulator.  (3) |X|^2 = re^2 + im^2 by one
// lane exchange, written to LDS P[64][257].  (4) 80 mel sums over each filter's support, log(max(., eps)),
// staged and stored as 64 contiguous rows.  fp32 throughout (bf16 operands would put ~0.4 % noise on the power
// spectrum).  The DFT is 206 k MAC per frame = 74 GFLOP for 30 minutes of audio.
//
// The four stages are one device function, fbank_tile, over a sample-fetch functor (where frame f's sample n lies) and an
// emit functor (where the tile's rows go).  Every frame depends on its own 400 samples only -- one wave_sum per frame, one A
// row per MFMA output row --, so each instantiation gives the same bits per frame: pafc_fbank_f32 (one waveform),
// pafc_fbank_batch (grid.y = row of a ragged batch; rows past a row's frame count are written as zero) and
// pafc_fbank_stream (a row's samples are its carried tail followed by the new chunk; a second small kernel moves the carry)
// and pafc_fbank_stream_rows (the same per row of a slot pool: every row has its own carry length, sample count and place in
// its slot's ring of frames, read from a descriptor table in device memory).
#include "pafc_common.h"
#include "fbank_host.h"

namespace pafc {
namespace {

using fbank_host::WIN;
using fbank_host::SHIFT;
using fbank_host::CARRY;
using fbank_host::MAXMEL;
constexpr int NBIN = 257;
constexpr int NTILE = 17, NCOL = NTILE * 32;  // 544 >= 2 * 257
constexpr int FPB = 64;                       // frames per block
constexpr int LDA = WIN + 1;                  // LDS row stride (words)
constexpr int LDP = NBIN;                     // 257: odd, conflict-free

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct FbankParams {
    const float *wave;      // (S)
    long S;
    int m;                  // frames
    const float *window;    // (400)
    const float *tw;        // (400, 544): col 2k = cos(2 pi k n / 512), col 2k+1 = -sin(.), zero padded
    const float *melw;      // (nmel, 257)
    const int *mel_lo;      // (nmel) first bin with non-zero weight
    const int *mel_hi;      // (nmel) one past the last
    int nmel;
    const float *noise;     // (m, 400) or null
    float dither;
    float preemph;
    float *out;             // (m, nmel)
};

// One tile of 64 frames [m0, m0 + 64) of a row with p.m frames (p.noise: that row's; p.wave and p.out are not used here).
// fetch(160 f)[n]: sample n of the row's frame f, asked for live frames only (f < p.m, n < 400); emit(O, ldo, tid): called by
// all 256 threads after the last barrier with the staged tile O[64][ldo].
template <class Fetch, class Emit>
__device__ __forceinline__ void fbank_tile(const FbankParams &p, const int m0, Fetch fetch, Emit emit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *A = lds;                            // [64][401]
    float *P = lds;                            // [64][257], aliases A after the GEMM
    float *O = lds + FPB * LDP + 64;           // [64][nmel] staging, behind P
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    // ---- (1) frame conditioning ----------------------------------------------------------------------
    for (int ff = 0; ff < 16; ++ff) {
        const int f = wv * 16 + ff;
        const int fr = m0 + f;
        float x[7], xp[7];
        float sum = 0.f;
        const bool live = fr < p.m;
        const auto src = fetch((long)fr * SHIFT);
        const float *nz = p.noise ? p.noise + (long)fr * WIN : nullptr;
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const int n = lane + 64 * q;
            x[q] = 0.f; xp[q] = 0.f;
            if (live && n < WIN) {
                x[q] = src[n];
                const int np = n > 0 ? n - 1 : 0;   // replicate-padded predecessor
                xp[q] = src[np];
                if (nz) { x[q] += nz[n] * p.dither; xp[q] += nz[np] * p.dither; }
                sum += x[q];
            }
        }
        const float mean = wave_sum(sum) * (1.f / WIN);
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const int n = lane + 64 * q;
            if (n < WIN) {
                const float y = (x[q] - mean) - p.preemph * (xp[q] - mean);
                A[f * LDA + n] = live ? y * p.window[n] : 0.f;
            }
        }
    }
    __syncthreads();

    // ---- (2) DFT as an fp32 MFMA GEMM: [64 x 400] x [400 x 544] -----------------------------------
    f32x16 acc[2][5];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int ci = 0; ci < 5; ++ci)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][ci][r] = 0.f;
    const int lr = lane & 31, lk = lane >> 5;
    const float *twl = p.tw + lr;
#pragma unroll 2
    for (int k0 = 0; k0 < WIN; k0 += 2) {
        const int kk = k0 + lk;
        const float a0 = A[lr * LDA + kk];
        const float a1 = A[(32 + lr) * LDA + kk];
        const float *twr = twl + (long)kk * NCOL;
#pragma unroll
        for (int ci = 0; ci < 5; ++ci) {
            const int ct = wv + 4 * ci;          // wave-uniform
            if (ct < NTILE) {
                const float b = twr[ct * 32];
                acc[0][ci] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][ci], 0, 0, 0);
                acc[1][ci] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][ci], 0, 0, 0);
            }
        }
    }
    __syncthreads();   // every wave is done with A before P overwrites it

    // ---- (3) power spectrum: C/D layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ---
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int ci = 0; ci < 5; ++ci) {
            const int ct = wv + 4 * ci;
            if (ct < NTILE) {
                const int bin = (ct * 32 + lr) >> 1;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float sq = acc[mt][ci][r] * acc[mt][ci][r];
                    sq += __shfl_xor(sq, 1, 64);     // re^2 + im^2 (adjacent columns = adjacent lanes)
                    const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                    if (!(lr & 1) && bin < NBIN) P[row * LDP + bin] = sq;
                }
            }
        }
    __syncthreads();

    // ---- (4) mel energies + log: lane = frame, wave = a quarter of the filters ------------------------
    const int per = (p.nmel + 3) / 4;
    const int ldo = p.nmel | 1;                  // odd row stride: conflict-free lane-per-frame writes
    const float eps = 1.1920928955078125e-07f;   // float32 machine epsilon, as torchaudio's floor
    for (int bi = 0; bi < per; ++bi) {
        const int b = wv * per + bi;             // wave-uniform
        if (b < p.nmel) {
            const int lo = p.mel_lo[b], hi = p.mel_hi[b];
            const float *wrow = p.melw + (long)b * NBIN;
            float e = 0.f;
            for (int k = lo; k < hi; ++k) e = fmaf(P[lane * LDP + k], wrow[k], e);
            O[lane * ldo + b] = logf(fmaxf(e, eps));
        }
    }
    __syncthreads();
    emit(O, ldo, tid);
}

__global__ __launch_bounds__(256) void fbank_kernel(const FbankParams p) {
    const int m0 = blockIdx.x * FPB;
    fbank_tile(p, m0, [&](long s0) { return p.wave + s0; }, [&](const float *O, int ldo, int tid) {
        const int nvalid = min(FPB, p.m - m0);
        float *dst = p.out + (long)m0 * p.nmel;
        for (int i = tid; i < nvalid * p.nmel; i += 256) dst[i] = O[(i / p.nmel) * ldo + (i % p.nmel)];
    });
}

// Rows of a batch or of B lock-step streams: grid (tiles, rows).
struct RowsParams {
    const float *carry;       // stream: (rows, CARRY), the first c samples of a row; batch: unused
    int c;
    long ld_wave;             // row stride of p.wave (the batch's waveforms / the stream's chunk)
    const long *lens;         // batch: (rows) sample counts or null; stream: null
    long max_samples;         // batch: the row length the grid was sized for; stream: c + n
    int t_rows;               // rows [0, t_rows) of a batch row's output are written (zero past its frame count)
    void *out;                // row b, frame f at out + b * out_row_stride + out_offset + f * nmel  (elements)
    long out_row_stride, out_offset;
    int *out_lens;            // (rows) frame counts or null
};

// sample s0 + n of (carry[0:c] ++ chunk)
struct CarryThenChunk {
    const float *carry, *chunk;
    long c, s0;
    __device__ __forceinline__ float operator[](int n) const { return s0 + n < c ? carry[s0 + n] : chunk[s0 + n - c]; }
};

template <typename ET, bool STREAM>
__global__ __launch_bounds__(256) void fbank_rows_kernel(const FbankParams p, const RowsParams r) {
    const int b = blockIdx.y, m0 = blockIdx.x * FPB, tid = threadIdx.x;
    long len = r.max_samples;
    if (r.lens) {
        const long v = r.lens[b];
        len = v < 0 ? 0 : (v > r.max_samples ? r.max_samples : v);
    }
    const int m = (int)fbank_host::num_frames(len);             // <= t_rows
    if (m0 == 0 && tid == 0 && r.out_lens) r.out_lens[b] = m;
    ET *dst = (ET *)r.out + (long)b * r.out_row_stride + r.out_offset + (long)m0 * p.nmel;
    const int nrows = min(FPB, r.t_rows - m0);
    if (m0 >= m) {                                              // block-uniform, before any barrier: a tile of padding
        for (int i = tid; i < nrows * p.nmel; i += 256) Elem<ET>::store(dst + i, 0.f);
        return;
    }
    FbankParams q = p;
    q.m = m;
    q.noise = p.noise ? p.noise + (long)b * r.t_rows * WIN : nullptr;
    const float *row = p.wave + (long)b * r.ld_wave;
    const float *car = STREAM ? r.carry + (long)b * CARRY : nullptr;
    const int c = STREAM ? r.c : 0;
    auto emit = [&](const float *O, int ldo, int) {
        const int nvalid = min(FPB, m - m0);
        for (int i = tid; i < nrows * q.nmel; i += 256) {
            const int f = i / q.nmel;
            Elem<ET>::store(dst + i, f < nvalid ? O[f * ldo + (i % q.nmel)] : 0.f);   // padding is zero, not log(eps)
        }
    };
    if (STREAM)
        fbank_tile(q, m0, [&](long s0) { return CarryThenChunk{car, row, c, s0}; }, emit);
    else
        fbank_tile(q, m0, [&](long s0) { return row + s0; }, emit);
}

// carry[b, 0:c_next] <- the last c_next samples of (carry[b, 0:c] ++ chunk[b, 0:n]).  Source and destination overlap when
// n < c: one block per row reads its <= CARRY - 1 samples into registers, barriers, then writes.
__global__ __launch_bounds__(256) void fbank_carry_kernel(float *carry, int c, const float *chunk, long ld_chunk, long n,
                                                          int c_next) {
    float *car = carry + (long)blockIdx.x * CARRY;
    const float *row = chunk + (long)blockIdx.x * ld_chunk;
    const long first = c + n - c_next;
    float v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = threadIdx.x + 256 * q;
        v[q] = 0.f;
        if (j < c_next) {
            const long s = first + j;
            v[q] = s < c ? car[s] : row[s - c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = threadIdx.x + 256 * q;
        if (j < c_next) car[j] = v[q];
    }
}

// Ragged rows of a slot pool: grid (tiles of the row with the most frames, R).  Row b's descriptor is rows[4 b ..] =
// {slot, c, n, first_frame}; its frame f goes to out[slot, (first_frame + f) mod ring_frames, :].
struct SlotRowsParams {
    const float *carry;       // (S, CARRY)
    const int *rows;          // (R, 4) device
    long ld_chunk;
    void *out;                // (S, ring_frames, nmel)
    int ring_frames;
};

template <typename ET>
__global__ __launch_bounds__(256) void fbank_slot_rows_kernel(const FbankParams p, const SlotRowsParams r) {
    const int b = blockIdx.y, m0 = blockIdx.x * FPB, tid = threadIdx.x;
    const int *d = r.rows + 4 * b;
    const int slot = d[0], c = d[1], n = d[2], first = d[3];
    const int m = n > 0 ? (int)fbank_host::num_frames((long)c + n) : 0;
    if (m0 >= m) return;                                        // block-uniform, before any barrier
    FbankParams q = p;
    q.m = m;
    const float *row = p.wave + (long)b * r.ld_chunk;
    const float *car = r.carry + (long)slot * CARRY;
    ET *ring = (ET *)r.out + (long)slot * r.ring_frames * p.nmel;
    const int at = (int)(((long)first + m0) % r.ring_frames);   // ring row of the tile's first frame
    fbank_tile(q, m0, [&](long s0) { return CarryThenChunk{car, row, c, s0}; }, [&](const float *O, int ldo, int) {
        const int nvalid = min(FPB, m - m0);
        for (int i = tid; i < nvalid * q.nmel; i += 256) {
            const int f = i / q.nmel, k = i % q.nmel;
            const int at_f = (at + f) % r.ring_frames;          // (a ring shorter than a tile wraps more than once)
            Elem<ET>::store(ring + (long)at_f * q.nmel + k, O[f * ldo + k]);
        }
    });
}

// fbank_carry_kernel per row of the descriptor table, on carry[slot]; a row without new samples is left alone.
__global__ __launch_bounds__(256) void fbank_slot_carry_kernel(float *carry, const int *rows, const float *chunk, long ld_chunk) {
    const int *d = rows + 4 * blockIdx.x;
    const int slot = d[0], c = d[1], n = d[2];
    if (n <= 0) return;                                         // block-uniform
    const int c_next = c + n - SHIFT * (int)fbank_host::num_frames((long)c + n);
    float *car = carry + (long)slot * CARRY;
    const float *row = chunk + (long)blockIdx.x * ld_chunk;
    const int first = c + n - c_next;
    float v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = threadIdx.x + 256 * q;
        v[q] = 0.f;
        if (j < c_next) {
            const int s = first + j;
            v[q] = s < c ? car[s] : row[s - c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = threadIdx.x + 256 * q;
        if (j < c_next) car[j] = v[q];
    }
}

size_t tile_lds_bytes(int nmel) {
    const size_t a_bytes = sizeof(float) * FPB * LDA;
    const size_t po_bytes = sizeof(float) * (FPB * LDP + 64 + FPB * (nmel | 1));
    return a_bytes > po_bytes ? a_bytes : po_bytes;
}

template <typename ET, bool STREAM>
int launch_rows(const FbankParams &p, const RowsParams &r, long tiles, int B, hipStream_t stream) {
    // > 64 KiB of dynamic LDS needs the attribute; it is per device and idempotent, so set it on every call
    if (hipFuncSetAttribute((const void *)fbank_rows_kernel<ET, STREAM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess)
        return PAFC_ERR_LAUNCH;
    hipLaunchKernelGGL((fbank_rows_kernel<ET, STREAM>), dim3((unsigned)tiles, (unsigned)B), dim3(256), tile_lds_bytes(p.nmel),
                       stream, p, r);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

template <typename ET>
int launch_slot_rows(const FbankParams &p, const SlotRowsParams &r, long tiles, int R, hipStream_t stream) {
    if (hipFuncSetAttribute((const void *)fbank_slot_rows_kernel<ET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
        return PAFC_ERR_LAUNCH;
    hipLaunchKernelGGL((fbank_slot_rows_kernel<ET>), dim3((unsigned)tiles, (unsigned)R), dim3(256), tile_lds_bytes(p.nmel), stream,
                       p, r);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

}  // namespace
}  // namespace pafc

extern "C" {

long pafc_fbank_num_frames(long num_samples) { return pafc::fbank_host::num_frames(num_samples); }

int pafc_fbank_tables_cols(void) { return pafc::NCOL; }

int pafc_fbank_f32(const float *wave, long num_samples, const float *window, const float *dft_table,
                   const float *mel_weights, const int *mel_lo, const int *mel_hi, int num_mel_bins,
                   const float *noise, float dither, float preemph, float *out, pafc_stream_t stream) {
    if (!wave || !window || !dft_table || !mel_weights || !mel_lo || !mel_hi || !out) return PAFC_ERR_NULL_POINTER;
    if (num_mel_bins <= 0 || num_mel_bins > pafc::MAXMEL) return PAFC_ERR_BAD_DIMS;
    const long m = pafc_fbank_num_frames(num_samples);
    if (m <= 0 || m > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    pafc::FbankParams p{wave, num_samples, (int)m, window, dft_table, mel_weights, mel_lo, mel_hi, num_mel_bins,
                        noise, dither, preemph, out};
    const size_t lds = pafc::tile_lds_bytes(num_mel_bins);
    // > 64 KiB of dynamic LDS needs the attribute; it is per device and idempotent, so set it on every call
    if (hipFuncSetAttribute((const void *)pafc::fbank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
        return PAFC_ERR_LAUNCH;
    const unsigned blocks = (unsigned)((m + pafc::FPB - 1) / pafc::FPB);
    hipLaunchKernelGGL(pafc::fbank_kernel, dim3(blocks), dim3(256), lds, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_fbank_stream_plan(int c, long n, long *frames, int *c_next) {
    return pafc::fbank_host::stream_plan(c, n, frames, c_next);
}

int pafc_fbank_batch(const float *waves, long ld_wave, const long *lengths, int B, long max_samples, const float *window,
                     const float *dft_table, const float *mel_weights, const int *mel_lo, const int *mel_hi, int num_mel_bins,
                     const float *noise, float dither, float preemph, void *out, int out_dtype, int *out_frames,
                     pafc_stream_t stream) {
    long t_max = 0;
    const int rc = pafc::fbank_host::batch_check(waves, ld_wave, B, max_samples,
                                                 pafc::fbank_host::tables_null(window, dft_table, mel_weights, mel_lo, mel_hi),
                                                 num_mel_bins, out, out_dtype, &t_max);
    if (rc != PAFC_OK) return rc;
    pafc::FbankParams p{waves, max_samples, (int)t_max, window, dft_table, mel_weights, mel_lo, mel_hi, num_mel_bins,
                        noise, dither, preemph, nullptr};
    pafc::RowsParams r{nullptr, 0, ld_wave, lengths, max_samples, (int)t_max, out, t_max * num_mel_bins, 0, out_frames};
    const long tiles = (t_max + pafc::FPB - 1) / pafc::FPB;
    return out_dtype == PAFC_BF16 ? pafc::launch_rows<pafc::bf16_t, false>(p, r, tiles, B, (hipStream_t)stream)
                                  : pafc::launch_rows<float, false>(p, r, tiles, B, (hipStream_t)stream);
}

int pafc_fbank_stream(float *carry, int c, const float *chunk, long ld_chunk, long n, int B, const float *window,
                      const float *dft_table, const float *mel_weights, const int *mel_lo, const int *mel_hi, int num_mel_bins,
                      float dither, float preemph, void *out, int out_dtype, long out_row_stride, long first_frame,
                      pafc_stream_t stream) {
    long frames = 0;
    int c_next = 0;
    int rc = pafc::fbank_host::stream_check(carry, c, chunk, ld_chunk, n, B,
                                            pafc::fbank_host::tables_null(window, dft_table, mel_weights, mel_lo, mel_hi),
                                            num_mel_bins, dither, out, out_dtype, out_row_stride, first_frame, &frames, &c_next);
    if (rc != PAFC_OK || n == 0) return rc;
    if (frames > 0) {
        pafc::FbankParams p{chunk, c + n, (int)frames, window, dft_table, mel_weights, mel_lo, mel_hi, num_mel_bins,
                            nullptr, 0.f, preemph, nullptr};
        pafc::RowsParams r{carry, c, ld_chunk, nullptr, c + n, (int)frames, out, out_row_stride, first_frame * num_mel_bins,
                           nullptr};
        const long tiles = (frames + pafc::FPB - 1) / pafc::FPB;
        rc = out_dtype == PAFC_BF16 ? pafc::launch_rows<pafc::bf16_t, true>(p, r, tiles, B, (hipStream_t)stream)
                                    : pafc::launch_rows<float, true>(p, r, tiles, B, (hipStream_t)stream);
        if (rc != PAFC_OK) return rc;
    }
    hipLaunchKernelGGL(pafc::fbank_carry_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, carry, c, chunk, ld_chunk,
                       n, c_next);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_fbank_stream_rows(float *carry, int S, const int *rows, const int *rows_dev, int R, const float *chunk, long ld_chunk,
                           long n_max, const float *window, const float *dft_table, const float *mel_weights, const int *mel_lo,
                           const int *mel_hi, int num_mel_bins, float dither, float preemph, void *out, int out_dtype,
                           int ring_frames, pafc_stream_t stream) {
    long frames = 0;
    bool any_new = false;
    int rc = pafc::fbank_host::stream_rows_check(carry, S, rows, rows_dev, R, chunk, ld_chunk, n_max,
                                                 pafc::fbank_host::tables_null(window, dft_table, mel_weights, mel_lo, mel_hi),
                                                 num_mel_bins, dither, out, out_dtype, ring_frames, &frames, &any_new);
    if (rc != PAFC_OK || !any_new) return rc;
    if (frames > 0) {
        pafc::FbankParams p{chunk, 0, 0, window, dft_table, mel_weights, mel_lo, mel_hi, num_mel_bins, nullptr, 0.f, preemph,
                            nullptr};
        pafc::SlotRowsParams r{carry, rows_dev, ld_chunk, out, ring_frames};
        const long tiles = (frames + pafc::FPB - 1) / pafc::FPB;
        rc = out_dtype == PAFC_BF16 ? pafc::launch_slot_rows<pafc::bf16_t>(p, r, tiles, R, (hipStream_t)stream)
                                    : pafc::launch_slot_rows<float>(p, r, tiles, R, (hipStream_t)stream);
        if (rc != PAFC_OK) return rc;
    }
    hipLaunchKernelGGL(pafc::fbank_slot_carry_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, carry, rows_dev, chunk,
                       ld_chunk);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

}  // extern "C"
