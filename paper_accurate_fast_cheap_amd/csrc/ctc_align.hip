// CTC forced alignment on the GPU (C ABI: include/pafc_search.h: pafc_ctc_align).
//
// The reference's force_align (wenet/utils/ctc_utils.py:105-161) is a Python double loop over (t, s) for one utterance on the
// host, with a (T, S) fp32 alpha table and a (T, S) int16 path table.  Here: one block per utterance walks the same extended
// labels l' = (blank, y_1, blank, ..., y_L, blank) as ctc_lattice_kernel (ctc_loss.hip), max-plus instead of log-sum-exp:
//
//   forward   threads stride over the S = 2 L + 1 states; alpha_{t-1} lives in LDS, double-buffered, two -inf guard entries in
//             front, so that state s reads [s], [s-1], [s-2] without a branch.  A thread keeps the labels of its states (and
//             whether the skip from s-2 is allowed) in registers for the whole utterance and gathers only those columns of a
//             frame, the next frame's while this frame is computed.  alpha_t(s) = max(cands) + lp[t, l'_s]: one fp32 add, so
//             every alpha is the bit pattern the reference's arithmetic gives.  A later candidate wins only when strictly greater.
//   pointers  the winning candidate (0, 1, 2) is 2 bits.  A wave holds 64 consecutive states: two ballots give the low and the
//             high bit of all 64 as two 64-bit planes, and lane 0 stores them as one 16-byte word -- 2 bits per (t, s), a row of
//             ceil(Smax / 64) such words per frame, written in order by the waves of the block.
//   backtrace in the same launch: one lane walks t = hlen-1 .. 1 through the planes, writes the frame's token, and records where
//             it enters (last frame) and leaves (first frame) every label state.
//
// A row that cannot be aligned (see the header) gets ok = 0, score = -inf and -1 everywhere; padding is never read.
#include <math.h>

#include "pafc_common.h"
#include "../../include/pafc_search.h"

namespace pafc {
namespace {

constexpr int kAlignMaxThreads = 1024;
constexpr int kAlignMaxIters = 16;                    // states per thread: 20 would fill the LDS, and spill registers
constexpr int kSkipBit = 1 << 30;

__device__ __forceinline__ void align_wipe(int tid, int nt, int from, int T, int ldt, int32_t *al, int32_t *fi, int32_t *la) {
    for (int t = from + tid; t < T; t += nt) al[t] = -1;
    if (from == 0)
        for (int i = tid; i < ldt; i += nt) { fi[i] = -1; la[i] = -1; }
}

// The strides K .. ITERS-1 of one frame for this thread's wave, which leaves at its first stride without a state: the test is
// uniform over the wave, a branch per stride.  (As a predicate per stride it costs an SGPR pair each for the whole frame loop, and
// 16 strides spill; as a loop with a break the unroll is refused.  The recursion is unrolled by construction.)
template <int ITERS, int K>
__device__ __forceinline__ void align_strides(int kn, int tid, int nt, int lane, const int (&col)[ITERS],
                                              const float (&e)[ITERS], const float *prev, float *cur, uint4 *bpw) {
    if constexpr (K < ITERS) {
        if (K >= kn) return;
        const int s = tid + K * nt;
        const int s2 = s & -((col[K] >> 30) & 1);           // s, or the guard entry 0 (-inf) where s-2 is no candidate
        float best = prev[2 + s];
        const float a1 = prev[1 + s], a2 = prev[s2];
        int w = 0;
        if (a1 > best) { best = a1; w = 1; }
        if (a2 > best) { best = a2; w = 2; }
        cur[2 + s] = best + e[K];
        const unsigned long long lo = __ballot(w & 1), hi = __ballot(w >> 1);
        if (lane == 0) {
            uint4 q;
            q.x = (unsigned)lo; q.y = (unsigned)(lo >> 32); q.z = (unsigned)hi; q.w = (unsigned)(hi >> 32);
            bpw[K * (nt >> 6)] = q;                         // (nt is a constant where K > 0: an immediate offset)
        }
        align_strides<ITERS, K + 1>(kn, tid, nt, lane, col, e, prev, cur, bpw);
    }
}

// ITERS: states per thread (blockDim.x * ITERS >= Smax); bp: [b][t][C] two-plane words; stamps: [b][4] wall-clock ticks
// (start, recursion done, backtrace done) -- a diagnostic for tools/bench_ctc_align.py, not part of the result
template <typename ET, int ITERS>
__global__ __launch_bounds__(kAlignMaxThreads) void ctc_align_kernel(int T, int V, long ldl, const ET *lp, const int32_t *hlens,
                                                                     const int64_t *ys, int ldy, const int32_t *ylens, int blank,
                                                                     int Smax, int C, uint4 *bp, long long *stamps,
                                                                     int32_t *align, int32_t *first, int32_t *last, int ldt,
                                                                     float *score, int32_t *ok) {
    using E = Elem<ET>;
    extern __shared__ float sh[];                   // [2][C * 64 + 2]: the previous frame, two guard entries in front
    __shared__ int s_bad, s_rep, s_end;
    // (more than one state per thread only in blocks of kAlignMaxThreads: the strides k nt are constants then)
    const int b = blockIdx.x, tid = threadIdx.x, nt = ITERS == 1 ? (int)blockDim.x : kAlignMaxThreads, lane = tid & 63;
    const int Tb = hlens[b], L = ylens[b];
    const int64_t *y = ys + (long)b * ldy;
    const ET *lb = lp + (long)b * T * ldl;
    int32_t *al = align + (long)b * T, *fi = first + (long)b * ldt, *la = last + (long)b * ldt;
    uint4 *bpb = bp + (long)b * T * C;
    if (tid == 0) stamps[4 * b] = wall_clock64();
    if (Tb <= 0 || Tb > T || L < 0 || L > ldy) {    // (lengths that would index outside the row's own data: not alignable)
        align_wipe(tid, nt, 0, T, ldt, al, fi, la);
        if (tid == 0) { score[b] = -INFINITY; ok[b] = 0; stamps[4 * b + 1] = stamps[4 * b + 2] = wall_clock64(); }
        return;
    }
    // ---- the labels: all of them tokens of the vocabulary, and few enough adjacent repeats to fit ------------------------------
    if (tid == 0) { s_bad = 0; s_rep = 0; }
    __syncthreads();
    {
        int bad = 0, rep = 0;
        for (int j = tid; j < L; j += nt) {
            const int64_t c = y[j];
            bad |= (c < 0 || c >= V || c == blank);
            rep += (j > 0 && c == y[j - 1]);
        }
        if (bad) atomicOr(&s_bad, 1);
        if (rep) atomicAdd(&s_rep, rep);
    }
    __syncthreads();
    if (s_bad || L + s_rep > Tb) {
        align_wipe(tid, nt, 0, T, ldt, al, fi, la);
        if (tid == 0) { score[b] = -INFINITY; ok[b] = 0; stamps[4 * b + 1] = stamps[4 * b + 2] = wall_clock64(); }
        return;
    }
    const int S = 2 * L + 1, W = C * 64 + 2;
    // A wave owns the 64 states from wbase + k nt on and skips them when none exists; the states of a row's last wave beyond
    // S are computed like blanks (LDS holds C * 64 of them): nothing flows from a state to a lower one, and nothing reads
    // their pointers, so the frame loop needs no test per lane.  col: this thread's column of lp per state, bit 30 set
    // where alpha(s-2) is a candidate.
    const int wbase = __builtin_amdgcn_readfirstlane(tid - lane);
    const int kn = wbase < S ? (S - wbase + nt - 1) / nt : 0;      // this wave's share of the ITERS strides
    int col[ITERS];
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
        const int s = tid + k * nt;
        col[k] = blank;
        if (s < S && (s & 1)) {
            col[k] = (int)y[s >> 1];
            if (s >= 2 && col[k] != (int)y[(s >> 1) - 1]) col[k] |= kSkipBit;
        }
    }
    // ---- forward ---------------------------------------------------------------------------------------------------------
    for (int s = tid; s < W; s += nt) sh[s] = sh[W + s] = -INFINITY;
    __syncthreads();
    float e[ITERS];
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
        const int s = tid + k * nt;
        e[k] = E::load(lb + (col[k] & ~kSkipBit));   // (a stride without a state reads the blank's column: no test per stride)
        if (s < 2 && s < S) sh[2 + s] = e[k];
    }
    if (Tb > 1) {
#pragma unroll
        for (int k = 0; k < ITERS; ++k)
            e[k] = E::load(lb + ldl + (col[k] & ~kSkipBit));
    }
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        const float *prev = sh + ((t - 1) & 1) * W;
        float *cur = sh + (t & 1) * W;
        float en[ITERS];
        const ET *row = lb + (long)(t + 1 < Tb ? t + 1 : t) * ldl;      // the next frame's columns, in flight over this frame's work
#pragma unroll
        for (int k = 0; k < ITERS; ++k) en[k] = E::load(row + (col[k] & ~kSkipBit));
        align_strides<ITERS, 0>(kn, tid, nt, lane, col, e, prev, cur, bpb + (long)t * C + (wbase >> 6));     // (this wave's word of frame t)
#pragma unroll
        for (int k = 0; k < ITERS; ++k) e[k] = en[k];
        __syncthreads();
    }
    // ---- the end state -------------------------------------------------------------------------------------------------------
    if (tid == 0) {
        const float *fin = sh + ((Tb - 1) & 1) * W;
        int end = S - 1;
        if (S >= 2 && fin[2 + S - 2] > fin[2 + S - 1]) end = S - 2;
        const float sc = fin[2 + end];
        const bool feasible = sc > -INFINITY;
        s_end = feasible ? end : -1;
        score[b] = feasible ? sc : -INFINITY;
        ok[b] = feasible ? 1 : 0;
        stamps[4 * b + 1] = wall_clock64();
    }
    __threadfence();                                // the planes of the other waves, before lane 0 reads them back
    __syncthreads();
    const int end = s_end;
    if (end < 0) {
        align_wipe(tid, nt, 0, T, ldt, al, fi, la);
        if (tid == 0) stamps[4 * b + 2] = wall_clock64();
        return;
    }
    for (int t = Tb + tid; t < T; t += nt) al[t] = -1;
    for (int i = L + tid; i < ldt; i += nt) { fi[i] = -1; la[i] = -1; }
    // ---- backtrace: one lane, from the last frame down ---------------------------------------------------------------------------
    if (tid == 0) {
        int s = end;
        if (s & 1) la[s >> 1] = Tb - 1;
        for (int t = Tb - 1; t >= 1; --t) {
            al[t] = (s & 1) ? (int)y[s >> 1] : blank;
            const uint4 q = bpb[(long)t * C + (s >> 6)];
            const int bit = s & 63;
            const unsigned lo = bit < 32 ? q.x >> bit : q.y >> (bit - 32), hi = bit < 32 ? q.z >> bit : q.w >> (bit - 32);
            const int w = (int)(lo & 1u) + 2 * (int)(hi & 1u);
            if (w) {                                // the walk leaves state s at its first frame, enters s - w at its last
                if (s & 1) fi[s >> 1] = t;
                s -= w;
                if (s & 1) la[s >> 1] = t - 1;
            }
        }
        al[0] = (s & 1) ? (int)y[s >> 1] : blank;
        if (s & 1) fi[s >> 1] = 0;
        stamps[4 * b + 2] = wall_clock64();
    }
}

template <typename ET, int ITERS>
int align_launch(int B, int T, int V, const void *lp, long ldl, const int32_t *hlens, const int64_t *ys, int ldy,
                 const int32_t *ylens, int blank, int Smax, int C, int threads, size_t lds, void *workspace, int32_t *align,
                 int32_t *first, int32_t *last, int ldt, float *score, int32_t *ok, hipStream_t s) {
    auto k = ctc_align_kernel<ET, ITERS>;
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return PAFC_ERR_LAUNCH;
    uint4 *bp = (uint4 *)workspace;
    long long *stamps = (long long *)(bp + (size_t)B * T * C);
    hipLaunchKernelGGL(k, dim3(B), dim3(threads), lds, s, T, V, ldl, (const ET *)lp, hlens, ys, ldy, ylens, blank, Smax, C, bp,
                       stamps, align, first, last, ldt, score, ok);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

template <typename ET, typename... A>
int align_dispatch(int iters, A... a) {
    if (iters <= 1) return align_launch<ET, 1>(a...);
    if (iters <= 2) return align_launch<ET, 2>(a...);
    if (iters <= 4) return align_launch<ET, 4>(a...);
    if (iters <= 8) return align_launch<ET, 8>(a...);
    return align_launch<ET, 16>(a...);
}

}  // namespace
}  // namespace pafc

extern "C" size_t pafc_ctc_align_workspace_bytes(int B, int T, int Lmax) {
    if (B <= 0 || T <= 0 || Lmax < 0) return 0;
    const size_t C = (2 * (size_t)Lmax + 1 + 63) / 64;
    return (size_t)B * T * C * 16 + (size_t)B * 32;
}

extern "C" int pafc_ctc_align(int dtype, int B, int T, int V, const void *lp, long ldl, const int32_t *hlens, const int64_t *ys,
                              int ldy, const int32_t *ylens, int blank, void *workspace, size_t workspace_bytes, int32_t *align,
                              int32_t *first, int32_t *last, int ld_times, float *score, int32_t *ok, pafc_stream_t stream) {
    if (!lp || !hlens || !ylens || !workspace || !align || !score || !ok) return PAFC_ERR_NULL_POINTER;
    if ((ldy > 0 && !ys) || (ld_times > 0 && (!first || !last))) return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || T <= 0 || V <= 0 || ldl < V || ldy < 0 || ld_times < ldy || blank < 0 || blank >= V) return PAFC_ERR_BAD_DIMS;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (V >= pafc::kSkipBit) return PAFC_ERR_UNSUPPORTED;
    const long Smax = 2 * (long)ldy + 1, Cl = (Smax + 63) / 64;
    const size_t lds = (size_t)2 * (Cl * 64 + 2) * sizeof(float);
    if (Cl * 64 > (long)pafc::kAlignMaxThreads * pafc::kAlignMaxIters) return PAFC_ERR_UNSUPPORTED;     // ldy <= 8191: 128 KiB of LDS
    if (workspace_bytes < pafc_ctc_align_workspace_bytes(B, T, ldy)) return PAFC_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return PAFC_ERR_ALIGNMENT;
    const int C = (int)Cl;
    const int threads = C * 64 < pafc::kAlignMaxThreads ? C * 64 : pafc::kAlignMaxThreads;
    const int iters = (int)((Smax + threads - 1) / threads);       // <= kAlignMaxIters
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        return pafc::align_dispatch<float>(iters, B, T, V, lp, ldl, hlens, ys, ldy, ylens, blank, (int)Smax, C, threads, lds, workspace,
                                           align, first, last, ld_times, score, ok, s);
    return pafc::align_dispatch<pafc::bf16_t>(iters, B, T, V, lp, ldl, hlens, ys, ldy, ylens, blank, (int)Smax, C, threads, lds,
                                              workspace, align, first, last, ld_times, score, ok, s);
}
