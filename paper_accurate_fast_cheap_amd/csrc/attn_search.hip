// attn_search.hip -- the two kernels of the attention decoder's beam search (include/pafc_attn_search.h).
//
// mha_step_kernel: one wave per (row, head); its body is mha_step_body.h, shared with pafc_mha_step_paths.  A step's self-attention is a GEMV per (row, head) over at most P keys of 64
// dimensions, bound by the reads of the cache: nothing for the matrix cores.  QK runs with the lanes over the keys of a tile
// of 64 (a lane reads its key's 64 contiguous elements as 16-byte accesses and holds q in registers), the online softmax
// merges a tile with two wave reductions, and PV runs with the lanes over the 64 dimensions (one coalesced row segment per
// key, its probability and cache row broadcast from the lane that owns the key).
//
// beam_rows_kernel / beam_utt_kernel: the two top-N selections of a step.  Both take the N best by N passes of an arg-max
// over the elements that come after the previous pass's winner in the order (value descending, index ascending): exact
// ties go to the lowest index without an exclusion list, and a NaN is never selected.
#include "pafc_attn_search.h"
#include "mha_step_body.h"

#include <math.h>

namespace pafc {

constexpr int kMaxBeam = 16;

struct StepArgs {
    int R, N, H, P;
    const void *qkv;
    long ldqkv;
    void *cache;
    const int32_t *anc, *pos, *done;
    void *out;
    long ldo;
};

template <typename ET> __global__ __launch_bounds__(kStepWaves * kWave) void mha_step_kernel(StepArgs a) {
    const int r = blockIdx.x, lane = threadIdx.x & (kWave - 1);
    const int h = blockIdx.y * kStepWaves + (threadIdx.x >> 6);
    const int p = *a.pos;
    if (h >= a.H || *a.done != 0 || p < 0 || p >= a.P) return;          // (wave-uniform)
    const long d = (long)a.H * kStepDk;
    const ET *qkv = static_cast<const ET *>(a.qkv) + (long)r * a.ldqkv;
    ET *cache = static_cast<ET *>(a.cache);
    const int32_t *anc = a.anc + ((long)(p & 1) * a.R + r) * a.P;
    const int base = (r / a.N) * a.N, R = a.R, N = a.N;
    // the cache row of key j < p through the ancestor table     (P * R fits an int: checked before the launch)
    mha_step_row<ET>(qkv, cache, d, h, lane, p, cache + ((long)p * a.R + r) * 2 * d,
                     [=](int j) { return j * R + base + min(max(anc[j], 0), N - 1); },
                     static_cast<ET *>(a.out) + (long)r * a.ldo);
}

// ---- selection ----

// does (v, i) come strictly after (pv, pi) in the order value descending, index ascending?  (false for a NaN v)
__device__ __forceinline__ bool after(float v, int i, float pv, int pi) { return v < pv || (v == pv && i > pi); }
// is (v, i) better than the best so far (bv, bi)?  bi < 0: nothing yet
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return bi < 0 || v > bv || (v == bv && i < bi); }

__device__ __forceinline__ void wave_best(float &bv, int &bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, kWave);
        const int oi = __shfl_xor(bi, off, kWave);
        if (oi >= 0 && better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
}

// (max, sum of exp(x - max)) pairs in double: the row's logsumexp is then exact to float32, so that a slot's score carries
// one float32 rounding per step and nothing else
__device__ __forceinline__ void lse_pair_merge(double &m, double &s, double m2, double s2) {
    const double M = fmax(m, m2);
    const double x = (m == -INFINITY) ? 0.0 : s * exp(m - M);
    const double y = (m2 == -INFINITY) ? 0.0 : s2 * exp(m2 - M);
    m = M;
    s = x + y;
}

// per row: logsumexp and the N largest logits -> cand_lp / cand_tok (R, N)
template <typename ET>
__global__ __launch_bounds__(256) void beam_rows_kernel(int N, int V, int cap, int eos, const ET *logits, long ldl,
                                                        const int32_t *ended, const int32_t *pos, const int32_t *done,
                                                        double *cand_lp, int32_t *cand_tok) {
    if (*done != 0 || *pos >= cap || *pos < 0) return;
    const int r = blockIdx.x, t = threadIdx.x;
    if (ended[r] != 0) {
        if (t < N) {
            cand_lp[r * N + t] = t == 0 ? 0.0 : -(double)INFINITY;
            cand_tok[r * N + t] = eos;
        }
        return;
    }
    const ET *row = logits + (long)r * ldl;
    __shared__ double dm[4], ds[4];
    __shared__ float sv[4];
    __shared__ int si[4];
    // logsumexp
    double m = -INFINITY, s = 0.0;
    for (int v = t; v < V; v += 256) {
        const double x = (double)Elem<ET>::load(row + v);
        if (x > m) {
            s = s * exp(m - x) + 1.0;
            m = x;
        } else if (x > -INFINITY) {
            s += exp(x - m);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lse_pair_merge(m, s, __shfl_xor(m, off, kWave), __shfl_xor(s, off, kWave));
    if ((t & 63) == 0) {
        dm[t >> 6] = m;
        ds[t >> 6] = s;
    }
    __syncthreads();
    m = dm[0];
    s = ds[0];
    for (int w = 1; w < 4; ++w) lse_pair_merge(m, s, dm[w], ds[w]);
    const double lse = m + log(s);
    float pv = INFINITY;
    int pi = -1;                       // nothing selected yet: every element comes after (+inf, -1)
    for (int k = 0; k < N; ++k) {
        float bv = 0.f;
        int bi = -1;
        for (int v = t; v < V; v += 256) {
            const float x = Elem<ET>::load(row + v);
            if ((k == 0 ? x == x : after(x, v, pv, pi)) && better(x, v, bv, bi)) {
                bv = x;
                bi = v;
            }
        }
        wave_best(bv, bi);
        if ((t & 63) == 0) {
            sv[t >> 6] = bv;
            si[t >> 6] = bi;
        }
        __syncthreads();
        bv = sv[0];
        bi = si[0];
        for (int w = 1; w < 4; ++w)
            if (si[w] >= 0 && better(sv[w], si[w], bv, bi)) {
                bv = sv[w];
                bi = si[w];
            }
        __syncthreads();
        if (t == 0) {
            // (fewer than N selectable logits -- NaNs -- leave (eos, -inf) candidates)
            cand_lp[r * N + k] = bi >= 0 ? (double)bv - lse : -(double)INFINITY;
            cand_tok[r * N + k] = bi >= 0 ? bi : eos;
        }
        if (bi < 0) {
            pv = -INFINITY;
            pi = V;                    // nothing comes after this
        } else {
            pv = bv;
            pi = bi;
        }
    }
}

struct UttArgs {
    int B, N, P, cap, eos;
    const double *cand_lp;
    const int32_t *cand_tok;
    float *score;
    int32_t *ended, *token, *anc, *trace_parent, *trace_token;
    float *trace_score;
    int32_t *pos, *done;
};

// one block: a wave per utterance in turn, then pos and done
__global__ __launch_bounds__(256) void beam_utt_kernel(UttArgs a) {
    const int p = *a.pos;
    if (*a.done != 0 || p >= a.cap || p < 0) return;          // (block-uniform, read before anything is written)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = a.N, R = a.B * a.N;
    __shared__ int live[4];
    int my_live = 0;
    for (int b = wave; b < a.B; b += 4) {
        // candidate c = i * N + k, up to 256: four per lane
        float tot[4];
        for (int u = 0; u < 4; ++u) {
            const int c = lane + 64 * u;
            tot[u] = c < N * N ? (float)((double)a.score[b * N + c / N] + a.cand_lp[(long)b * N * N + c]) : NAN;
        }
        float pv = INFINITY;
        int pi = -1;
        int my_c = 0;                  // lane s < N keeps the s-th best
        float my_v = -INFINITY;
        for (int s = 0; s < N; ++s) {
            float bv = 0.f;
            int bi = -1;
            for (int u = 0; u < 4; ++u) {
                const int c = lane + 64 * u;
                if (c < N * N && (s == 0 ? tot[u] == tot[u] : after(tot[u], c, pv, pi)) && better(tot[u], c, bv, bi)) {
                    bv = tot[u];
                    bi = c;
                }
            }
            wave_best(bv, bi);
            if (bi < 0) {              // NaN scores only: the slot repeats candidate s at -inf rather than reading outside
                bv = -INFINITY;
                bi = s;
                pv = -INFINITY;
                pi = N * N;
            } else {
                pv = bv;
                pi = bi;
            }
            if (lane == s) {
                my_c = bi;
                my_v = bv;
            }
        }
        // every read of score above precedes the writes below in this wave, and no other wave touches this utterance
        int tok = 0, par = 0;
        if (lane < N) {
            par = my_c / N;
            tok = a.cand_tok[(long)b * N * N + my_c];
            const int r = b * N + lane;
            a.score[r] = my_v;
            a.token[r] = tok;
            a.ended[r] = tok == a.eos;
            a.trace_parent[(long)p * R + r] = par;
            a.trace_token[(long)p * R + r] = tok;
            a.trace_score[(long)p * R + r] = my_v;
            if (tok != a.eos) my_live += 1;
        }
        const int32_t *src = a.anc + (long)(p & 1) * R * a.P;
        int32_t *dst = a.anc + (long)((p + 1) & 1) * R * a.P;
        for (int s = 0; s < N; ++s) {
            const int ps = __shfl(par, s, kWave);
            const int32_t *from = src + (long)(b * N + ps) * a.P;
            int32_t *to = dst + (long)(b * N + s) * a.P;
            for (int j = lane; j < p; j += kWave) to[j] = from[j];
            if (lane == 0) to[p] = ps;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) my_live += __shfl_xor(my_live, off, kWave);
    if (lane == 0) live[wave] = my_live;
    __syncthreads();
    if (threadIdx.x == 0) {
        *a.done = (live[0] + live[1] + live[2] + live[3]) == 0;
        *a.pos = p + 1;
    }
}

}  // namespace pafc

extern "C" int pafc_mha_step(int dtype, int R, int N, int H, int dk, int P, const void *qkv, long ldqkv, void *cache,
                             const int32_t *anc, const int32_t *pos, const int32_t *done, void *out, long ldo,
                             pafc_stream_t stream) {
    if (!qkv || !cache || !anc || !pos || !done || !out) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (R <= 0 || N <= 0 || H <= 0 || dk <= 0 || P <= 0 || R % N || H > 65535 * pafc::kStepWaves ||
        (long)P * R > 0x7fffffffL)
        return PAFC_ERR_BAD_DIMS;
    if (dk != pafc::kStepDk || N > pafc::kMaxBeam) return PAFC_ERR_UNSUPPORTED;
    const long width = (long)H * dk, per16 = dtype == PAFC_F32 ? 4 : 8;
    if (ldqkv < 3 * width || ldo < width || ldqkv % per16 || ldo % per16) return PAFC_ERR_BAD_DIMS;
    if (((uintptr_t)qkv | (uintptr_t)cache | (uintptr_t)out) & 15) return PAFC_ERR_ALIGNMENT;
    pafc::StepArgs a{R, N, H, P, qkv, ldqkv, cache, anc, pos, done, out, ldo};
    const dim3 grid((unsigned)R, (unsigned)((H + pafc::kStepWaves - 1) / pafc::kStepWaves)), block(pafc::kStepWaves * pafc::kWave);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::mha_step_kernel<float>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((pafc::mha_step_kernel<pafc::bf16_t>), grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" size_t pafc_attn_beam_select_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0 || N > pafc::kMaxBeam) return 0;
    return (size_t)B * N * N * 12;
}

extern "C" int pafc_attn_beam_select(int dtype, int B, int N, int V, int P, int cap, int eos, const void *logits, long ldl,
                                     float *score, int32_t *ended, int32_t *token, int32_t *anc, int32_t *trace_parent,
                                     int32_t *trace_token, float *trace_score, int32_t *pos, int32_t *done, void *workspace,
                                     size_t workspace_bytes, pafc_stream_t stream) {
    if (!logits || !score || !ended || !token || !anc || !trace_parent || !trace_token || !trace_score || !pos || !done ||
        !workspace)
        return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (B <= 0 || N <= 0 || V <= 0 || P <= 1 || cap < 1 || cap >= P || ldl < V || eos < 0 || eos >= V ||
        (long)B * N > 0x7fffffffL / (N > 0 ? N : 1))
        return PAFC_ERR_BAD_DIMS;
    if (N > pafc::kMaxBeam || V < N) return PAFC_ERR_UNSUPPORTED;
    if (workspace_bytes < pafc_attn_beam_select_workspace_bytes(B, N)) return PAFC_ERR_WORKSPACE;
    if ((uintptr_t)workspace & 7) return PAFC_ERR_ALIGNMENT;
    const int R = B * N;
    double *cand_lp = static_cast<double *>(workspace);
    int32_t *cand_tok = reinterpret_cast<int32_t *>(cand_lp + (size_t)R * N);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::beam_rows_kernel<float>), dim3((unsigned)R), dim3(256), 0, s, N, V, cap, eos,
                           (const float *)logits, ldl, ended, pos, done, cand_lp, cand_tok);
    else
        hipLaunchKernelGGL((pafc::beam_rows_kernel<pafc::bf16_t>), dim3((unsigned)R), dim3(256), 0, s, N, V, cap, eos,
                           (const pafc::bf16_t *)logits, ldl, ended, pos, done, cand_lp, cand_tok);
    if (hipGetLastError() != hipSuccess) return PAFC_ERR_LAUNCH;
    pafc::UttArgs a{B, N, P, cap, eos, cand_lp, cand_tok, score, ended, token, anc, trace_parent, trace_token, trace_score,
                    pos, done};
    hipLaunchKernelGGL(pafc::beam_utt_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
