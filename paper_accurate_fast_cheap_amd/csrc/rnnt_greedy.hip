// Batched RNN-T greedy search on gfx950 (C ABI: include/pafc_search.h: pafc_rnnt_greedy_*, and pafc_rnnt_greedy_stream_* for
// chunk-by-chunk decoding with carried state).
//
// basic_greedy_search (wenet/transducer/search/greedy_search.py) for every utterance of a batch at once, in lockstep: one step
// advances every live row by one decision.  Per row: frame t, predictor input tok, need_pred, k (symbols emitted in this frame),
// the committed LSTM state and the pending one (the output of the last predictor run), pred_out, P = pred_ffn(pred_out).
// The two states live in two slots per row; committing the pending state after a non-blank flips the row's slot index, so no
// state is ever copied.  E = enc_ffn(encoder_out) (B, T, J) is computed once per call by the caller.
//
//   lstm     one launch per layer, rows with need_pred only; a wave owns one hidden unit: its four gate rows (i, f, g, o) of
//            W_ih and W_hh stream straight to VGPRs (16 bytes per lane per row and step of k), 8 rows of the batch per pass;
//            layer 0 gathers the embedding row of tok itself; the cell update runs in the wave's lanes
//   matvec   projection, then pred_ffn: a wave per output element, the same streaming form
//   joint    a workgroup per 32-column slice of V, rows still running: h = tanh(E[b, t_b] + P_b) into LDS, logits of the slice
//            (8 lanes per vocabulary row), per (slice, row) only max, argmax (lowest index on ties) and sum of exp -- the (B, V)
//            logits are never stored
//   update   one workgroup: the slices' partials combined in slice order, log p(y) = -log sum_s psum_s e^(pmax_s - max),
//            the state machine of the reference, the token / frame appended, then the lists of running rows and of rows that
//            need the predictor for the next step (and their count, which the next step's kernels exit on when zero)
// Every kernel reads its row counts from the device, so a step holds no host read and can be captured in a graph.  No float
// atomics and no communication between workgroups inside a launch: the result is bitwise reproducible.
#include <math.h>

#include "pafc_common.h"
#include "rnnt_net.h"

namespace pafc {
namespace {

constexpr int GNB = 8;         // batch rows per pass of the streaming kernels
constexpr int VS = 32;         // vocabulary rows per joint workgroup
constexpr int kMaxB = 256;     // one update workgroup, a thread per row

__device__ __forceinline__ void ld4(const float *p, float *f) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
}
__device__ __forceinline__ void ld4(const bf16_t *p, float *f) {
    const uint2 q = *reinterpret_cast<const uint2 *>(p);
    Elem<bf16_t>::unpack4(q, f);
}
template <typename T> __device__ __forceinline__ float ld1(const T *p) { return Elem<T>::load(p); }

// w . x over four elements as one fixed chain: w0 x0 rounded, then three fmas.  Written out, because the compiler's own
// contraction of `w0 x0 + w1 x1 + w2 x2 + w3 x3` differs between the unrolled slots of a pass (some fused, some not), which
// made an fp32 row's result depend on its position among the rows of a step.  (bf16 operands: the products are exact in
// fp32, so fused and unfused agree and this is the arithmetic bf16 always had.)
__device__ __forceinline__ float dot4(float w0, float w1, float w2, float w3, float x0, float x1, float x2, float x3) {
    return fmaf(w3, x3, fmaf(w2, x2, fmaf(w1, x1, w0 * x0)));
}
__device__ __forceinline__ float dot4(const float *w, const float *x) { return dot4(w[0], w[1], w[2], w[3], x[0], x[1], x[2], x[3]); }

// device state, one layout for every kernel (B rows, L layers)
struct GState {
    int B, T, L, H, Pd, J, V, nsteps, blank, ns;
    long cap;                      // tokens a row can emit: T * nsteps
    int32_t *Tb, *t, *tok, *need, *k, *ntok, *slot;
    int32_t *ctl;                  // [0] rows that need the predictor, [1] rows still running
    int32_t *act, *live;           // their row ids
    double *score;
    float *hs, *cs;                // [2 slots][L][B][H]
    float *pred, *P;               // (B, Pd), (B, J)
    float *pmax, *psum;            // (ns, B)
    int32_t *parg;                 // (ns, B)
    int32_t *otok, *ofr;           // (B, cap)
};

__device__ __forceinline__ long hidx(const GState &s, int slot, int layer, int row) {
    return (((long)slot * s.L + layer) * s.B + row) * s.H;
}

__global__ __launch_bounds__(256) void greedy_init_kernel(GState s, const int64_t *lens) {
    const int tid = threadIdx.x;
    for (int b = tid; b < s.B; b += 256) {
        const int64_t l = lens[b];
        s.Tb[b] = (int)(l < 0 ? 0 : l > s.T ? s.T : l);
        s.t[b] = 0; s.tok[b] = s.blank; s.need[b] = 1; s.k[b] = 0; s.ntok[b] = 0; s.slot[b] = 0;
        s.score[b] = 0.0;
    }
    const long nh = (long)s.L * s.B * s.H;       // slot 0 = the committed zero state
    for (long q = tid; q < nh; q += 256) { s.hs[q] = 0.f; s.cs[q] = 0.f; }
    __syncthreads();
    if (tid == 0) {
        int na = 0;
        for (int b = 0; b < s.B; ++b)
            if (s.Tb[b] > 0) { s.live[na] = b; s.act[na] = b; ++na; }
        s.ctl[0] = na; s.ctl[1] = na;
    }
}

// one LSTM layer for the rows in s.act: gates = W_ih x + b_ih + W_hh h + b_hh (x: embedding of tok for layer 0, else the
// pending h of the layer below), committed (h, c) in, pending (h, c) out
template <typename WT, bool EMB>
__global__ __launch_bounds__(256) void greedy_lstm_kernel(GState s, int layer, int In, const WT *emb, const WT *Wih, const WT *Whh,
                                                          const WT *bih, const WT *bhh) {
    const int nact = s.ctl[0];
    if (nact == 0) return;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= s.H) return;
    const int H = s.H;
    for (int b0 = 0; b0 < nact; b0 += GNB) {
        const int nb = min(GNB, nact - b0);
        const WT *xe[GNB];
        const float *xf[GNB], *hr[GNB];
#pragma unroll
        for (int i = 0; i < GNB; ++i) {
            const int row = s.act[b0 + min(i, nb - 1)];
            if (EMB) xe[i] = emb + (long)s.tok[row] * In;
            else xf[i] = s.hs + hidx(s, 1 - s.slot[row], layer - 1, row);
            hr[i] = s.hs + hidx(s, s.slot[row], layer, row);
        }
        float acc[4][GNB];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < GNB; ++i) acc[g][i] = 0.f;
        for (int kk = lane * 4; kk < In; kk += 256) {
            float w[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) ld4(Wih + ((long)g * H + j) * In + kk, w[g]);
#pragma unroll
            for (int i = 0; i < GNB; ++i) {
                float x[4];
                if (EMB) ld4(xe[i] + kk, x); else ld4(xf[i] + kk, x);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g][i] += dot4(w[g], x);
            }
        }
        for (int kk = lane * 4; kk < H; kk += 256) {
            float w[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) ld4(Whh + ((long)g * H + j) * H + kk, w[g]);
#pragma unroll
            for (int i = 0; i < GNB; ++i) {
                float x[4];
                ld4(hr[i] + kk, x);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g][i] += dot4(w[g], x);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < GNB; ++i) acc[g][i] = wave_sum(acc[g][i]);
        if (lane < nb) {
            float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;
#pragma unroll
            for (int i = 0; i < GNB; ++i)
                if (i == lane) { gi = acc[0][i]; gf = acc[1][i]; gg = acc[2][i]; go = acc[3][i]; }
            if (bih) { gi += ld1(bih + j); gf += ld1(bih + H + j); gg += ld1(bih + 2 * H + j); go += ld1(bih + 3 * H + j); }
            if (bhh) { gi += ld1(bhh + j); gf += ld1(bhh + H + j); gg += ld1(bhh + 2 * H + j); go += ld1(bhh + 3 * H + j); }
            const int row = s.act[b0 + lane];
            const float c0 = s.cs[hidx(s, s.slot[row], layer, row) + j];
            const float c1 = sigm(gf) * c0 + sigm(gi) * tanhf(gg);
            const float h1 = sigm(go) * tanhf(c1);
            const long o = hidx(s, 1 - s.slot[row], layer, row) + j;
            s.cs[o] = Elem<WT>::round(c1);
            s.hs[o] = Elem<WT>::round(h1);
        }
    }
}

// out[row][n] = W[n] x_row + bias[n] for the rows in s.act, rounded to the weight type.  x_row = x + row * K, or, with
// from_pending, the pending h of the last layer.
template <typename WT>
__global__ __launch_bounds__(256) void greedy_matvec_kernel(GState s, int N, int K, const float *x, bool from_pending, const WT *W,
                                                            const WT *bias, float *out) {
    const int nact = s.ctl[0];
    if (nact == 0) return;
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    for (int b0 = 0; b0 < nact; b0 += GNB) {
        const int nb = min(GNB, nact - b0);
        const float *xr[GNB];
#pragma unroll
        for (int i = 0; i < GNB; ++i) {
            const int row = s.act[b0 + min(i, nb - 1)];
            xr[i] = from_pending ? s.hs + hidx(s, 1 - s.slot[row], s.L - 1, row) : x + (long)row * K;
        }
        float acc[GNB];
#pragma unroll
        for (int i = 0; i < GNB; ++i) acc[i] = 0.f;
        for (int kk = lane * 4; kk < K; kk += 256) {
            float w[4];
            ld4(W + (long)n * K + kk, w);
#pragma unroll
            for (int i = 0; i < GNB; ++i) {
                float v[4];
                ld4(xr[i] + kk, v);
                acc[i] += dot4(w, v);
            }
        }
#pragma unroll
        for (int i = 0; i < GNB; ++i) acc[i] = wave_sum(acc[i]);
        if (lane < nb) {
            float r = 0.f;
#pragma unroll
            for (int i = 0; i < GNB; ++i)
                if (i == lane) r = acc[i];
            if (bias) r += ld1(bias + n);
            out[(long)s.act[b0 + lane] * N + n] = Elem<WT>::round(r);
        }
    }
}

// logits of vocabulary rows [32 blockIdx.x, + 32) for the running rows, reduced to (max, argmax, sum of exp) per row
template <typename WT>
__global__ __launch_bounds__(256) void greedy_joint_kernel(GState s, const WT *E, const WT *W, const WT *bias) {
    extern __shared__ __attribute__((aligned(16))) float hsh[];   // [GNB][J]
    __shared__ float zs[GNB][VS];
    const int nlive = s.ctl[1];
    if (nlive == 0) return;
    const int tid = threadIdx.x, grp = tid >> 3, sub = tid & 7;
    const int J = s.J, v0 = blockIdx.x * VS, v = v0 + grp;
    const float bv = (bias && v < s.V) ? ld1(bias + v) : 0.f;
    for (int b0 = 0; b0 < nlive; b0 += GNB) {
        const int nb = min(GNB, nlive - b0);
        __syncthreads();                           // the previous pass is done with hsh / zs
        for (int q = tid; q < nb * J; q += 256) {
            const int i = q / J, c = q - i * J;
            const int row = s.live[b0 + i];
            float a = ld1(E + ((long)row * s.T + s.t[row]) * J + c) + s.P[(long)row * J + c];
            a = Elem<WT>::round(a);
            hsh[i * J + c] = Elem<WT>::round(tanhf(a));
        }
        __syncthreads();
        float acc[GNB];
#pragma unroll
        for (int i = 0; i < GNB; ++i) acc[i] = 0.f;
        if (v < s.V) {
            for (int kk = sub * 4; kk < J; kk += 32) {
                float w[4];
                ld4(W + (long)v * J + kk, w);
#pragma unroll
                for (int i = 0; i < GNB; ++i) {
                    const float4 h = *reinterpret_cast<const float4 *>(hsh + i * J + kk);
                    acc[i] += dot4(w[0], w[1], w[2], w[3], h.x, h.y, h.z, h.w);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < GNB; ++i) {
            float a = acc[i];
            a += __shfl_xor(a, 4, 8);
            a += __shfl_xor(a, 2, 8);
            a += __shfl_xor(a, 1, 8);
            if (sub == 0) zs[i][grp] = v < s.V ? a + bv : -INFINITY;
        }
        __syncthreads();
        if (tid < nb) {
            const int row = s.live[b0 + tid];
            float m = -INFINITY;
            int am = v0;
            const int nv = min(VS, s.V - v0);
            for (int g = 0; g < nv; ++g)
                if (zs[tid][g] > m) { m = zs[tid][g]; am = v0 + g; }
            float sum = 0.f;
            for (int g = 0; g < nv; ++g) sum += expf(zs[tid][g] - m);
            s.pmax[(long)blockIdx.x * s.B + row] = m;
            s.psum[(long)blockIdx.x * s.B + row] = sum;
            s.parg[(long)blockIdx.x * s.B + row] = am;
        }
    }
}

__global__ __launch_bounds__(256) void greedy_update_kernel(GState s, int32_t *running) {
    __shared__ unsigned char flags[kMaxB];            // bit 0: still running, bit 1: needs the predictor
    __shared__ int ysh[kMaxB];
    __shared__ float lsh[kMaxB];
    const int b = threadIdx.x, lane = b & 63, wave = b >> 6;
    const int nlive = s.ctl[1];
    if (nlive == 0) {
        if (b == 0 && running) running[0] = 0;
        return;
    }
    // a wave per running row combines the slices' partials: max (lowest index on ties), then the sum in a fixed order
    for (int i = wave; i < nlive; i += 4) {
        const int row = s.live[i];
        float m = -INFINITY;
        int y = 0x7fffffff;
        for (int q = lane; q < s.ns; q += 64) {
            const float pm = s.pmax[(long)q * s.B + row];
            const int a = s.parg[(long)q * s.B + row];
            if (pm > m || (pm == m && a < y)) { m = pm; y = a; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float om = __shfl_xor(m, off, 64);
            const int oy = __shfl_xor(y, off, 64);
            if (om > m || (om == m && oy < y)) { m = om; y = oy; }
        }
        float sum = 0.f;
        for (int q = lane; q < s.ns; q += 64) sum += s.psum[(long)q * s.B + row] * expf(s.pmax[(long)q * s.B + row] - m);
        sum = wave_sum(sum);
        if (lane == 0) {
            ysh[row] = (y >= 0 && y < s.V) ? y : s.blank;   // (no finite logit at all: blank, never an id outside V)
            lsh[row] = -logf(sum);                           // log p(y) = z_y - lse = -log sum
        }
    }
    __syncthreads();
    int fl = 0;
    if (b < s.B && s.t[b] < s.Tb[b]) {
        const int y = ysh[b];
        s.score[b] += (double)lsh[b];
        int t = s.t[b], k = s.k[b];
        if (y != s.blank) {
            const int n = s.ntok[b];
            if (n < s.cap) { s.otok[(long)b * s.cap + n] = y; s.ofr[(long)b * s.cap + n] = t; }
            s.ntok[b] = n + 1;
            s.tok[b] = y;
            s.slot[b] ^= 1;                                // commit the pending state
            s.need[b] = 1;
            ++k;
        }
        if (y == s.blank || k >= s.nsteps) {
            if (y == s.blank) s.need[b] = 0;
            ++t;
            k = 0;
        }
        s.t[b] = t;
        s.k[b] = k;
        if (t < s.Tb[b]) fl = 1 | (s.need[b] ? 2 : 0);
    }
    if (b < s.B) flags[b] = (unsigned char)fl;
    __syncthreads();
    if (b == 0) {                                     // the lists in row order, from LDS
        int na = 0, nl = 0;
        for (int r = 0; r < s.B; ++r) {
            const int f = flags[r];
            if (f & 1) s.live[nl++] = r;
            if (f & 2) s.act[na++] = r;
        }
        s.ctl[0] = na; s.ctl[1] = nl;
        if (running) running[0] = nl;
    }
}

__global__ __launch_bounds__(256) void greedy_finish_kernel(GState s, int ld, int32_t *tokens, int32_t *frames, int32_t *ntok,
                                                            double *score, int32_t *running) {
    const int b = blockIdx.x;
    const int n = s.ntok[b];
    const int m = (int)min((long)min(n, ld), s.cap);
    for (int i = threadIdx.x; i < m; i += 256) {
        tokens[(long)b * ld + i] = s.otok[(long)b * s.cap + i];
        if (frames) frames[(long)b * ld + i] = s.ofr[(long)b * s.cap + i];
    }
    if (threadIdx.x == 0) {
        ntok[b] = n;
        if (score) score[b] = s.score[b];
        if (b == 0 && running) running[0] = s.ctl[1];
    }
}

// ---- streaming (pafc_rnnt_greedy_stream_*) ----------------------------------------------------------------------------------
// The stream workspace is the GState layout for (B, Tmax) followed by an int64 frame base per row (the absolute index of the
// current chunk's frame 0), so the step kernels above advance it unchanged with T = Tmax over a fixed (B, Tmax, J) E.  When a
// row leaves a chunk its state is (t = Tb, k = 0, tok, need, slot, pred, P, score): what the whole-utterance run holds at that
// frame boundary.  feed only moves the frame window; everything the decisions depend on carries over.

// the lists of running rows / rows that need the predictor, in row order (thread 0 of a block, after a barrier)
__device__ __forceinline__ void rebuild_lists(const GState &s, int32_t *running) {
    int na = 0, nl = 0;
    for (int r = 0; r < s.B; ++r) {
        if (s.t[r] < s.Tb[r]) {
            s.live[nl++] = r;
            if (s.need[r]) s.act[na++] = r;
        }
    }
    s.ctl[0] = na; s.ctl[1] = nl;
    if (running) running[0] = nl;
}

__global__ __launch_bounds__(256) void greedy_stream_reset_kernel(GState s, int64_t *base, const int32_t *mask) {
    const int tid = threadIdx.x;
    for (int b = tid; b < s.B; b += 256) {
        if (mask && !mask[b]) continue;
        s.Tb[b] = 0; s.t[b] = 0; s.tok[b] = s.blank; s.need[b] = 1; s.k[b] = 0; s.ntok[b] = 0; s.slot[b] = 0;
        s.score[b] = 0.0;
        base[b] = 0;
    }
    const long nh = (long)s.L * s.B * s.H;       // slot 0 = the committed zero state
    for (long q = tid; q < nh; q += 256) {
        const int row = (int)((q / s.H) % s.B);
        if (!mask || mask[row]) { s.hs[q] = 0.f; s.cs[q] = 0.f; }
    }
    __syncthreads();
    if (tid == 0) rebuild_lists(s, nullptr);
}

__global__ __launch_bounds__(256) void greedy_stream_feed_kernel(GState s, int64_t *base, const int64_t *nframes, int32_t *running) {
    const int tid = threadIdx.x;
    for (int b = tid; b < s.B; b += 256) {
        const int64_t l = nframes[b];
        base[b] += s.Tb[b];
        s.Tb[b] = (int)(l < 0 ? 0 : l > s.T ? s.T : l);
        s.t[b] = 0;
        s.ntok[b] = 0;
    }
    __syncthreads();
    if (tid == 0) rebuild_lists(s, running);
}

__global__ __launch_bounds__(256) void greedy_stream_drain_kernel(GState s, const int64_t *base, int ld, int32_t *tokens, int64_t *frames,
                                                                  int32_t *ntok, double *score, int32_t *running) {
    const int b = blockIdx.x;
    const int n = s.ntok[b];
    const int m = (int)min((long)min(n, ld), s.cap);
    const int64_t f0 = base[b];
    for (int i = threadIdx.x; i < m; i += 256) {
        tokens[(long)b * ld + i] = s.otok[(long)b * s.cap + i];
        if (frames) frames[(long)b * ld + i] = f0 + s.ofr[(long)b * s.cap + i];
    }
    if (threadIdx.x == 0) {
        ntok[b] = n;
        if (score) score[b] = s.score[b];
        if (b == 0 && running) running[0] = s.ctl[1];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

GState layout(void *ws, int B, int T, int L, int H, int Pd, int J, int V, int nsteps, int blank, size_t *bytes) {
    GState s{};
    s.B = B; s.T = T; s.L = L; s.H = H; s.Pd = Pd; s.J = J; s.V = V; s.nsteps = nsteps; s.blank = blank;
    s.ns = (V + VS - 1) / VS;
    s.cap = (long)T * nsteps;
    char *p = (char *)ws;
    size_t o = 0;
    auto take = [&](size_t b) { char *q = p ? p + o : nullptr; o += al256(b); return q; };
    int32_t **ints[] = {&s.Tb, &s.t, &s.tok, &s.need, &s.k, &s.ntok, &s.slot, &s.act, &s.live};
    for (int32_t **q : ints) *q = (int32_t *)take((size_t)B * sizeof(int32_t));
    s.ctl = (int32_t *)take(2 * sizeof(int32_t));
    s.score = (double *)take((size_t)B * sizeof(double));
    s.hs = (float *)take((size_t)2 * L * B * H * sizeof(float));
    s.cs = (float *)take((size_t)2 * L * B * H * sizeof(float));
    s.pred = (float *)take((size_t)B * Pd * sizeof(float));
    s.P = (float *)take((size_t)B * J * sizeof(float));
    s.pmax = (float *)take((size_t)s.ns * B * sizeof(float));
    s.psum = (float *)take((size_t)s.ns * B * sizeof(float));
    s.parg = (int32_t *)take((size_t)s.ns * B * sizeof(int32_t));
    s.otok = (int32_t *)take((size_t)B * s.cap * sizeof(int32_t));
    s.ofr = (int32_t *)take((size_t)B * s.cap * sizeof(int32_t));
    *bytes = o;
    return s;
}

int check_dims(int B, int T, int n_steps, int blank, int V) {
    if (B <= 0 || B > kMaxB || T <= 0 || n_steps <= 0 || V <= 0 || blank < 0 || blank >= V) return PAFC_ERR_BAD_DIMS;
    if ((long)T * n_steps > 0x7fffffffL) return PAFC_ERR_UNSUPPORTED;
    return PAFC_OK;
}

// the stream workspace: the GState layout, then the frame bases
GState stream_layout(void *ws, const pafc_rnnt_greedy_net *n, int B, int Tmax, int nsteps, int blank, int64_t **base, size_t *bytes) {
    size_t o = 0;
    const GState s = layout(ws, B, Tmax, n->num_layers, n->hidden, n->pred_dim, n->join_dim, n->vocab, nsteps, blank, &o);
    if (base) *base = ws ? (int64_t *)((char *)ws + o) : nullptr;
    *bytes = o + al256((size_t)B * sizeof(int64_t));
    return s;
}

template <typename WT>
void launch_step(const pafc_rnnt_greedy_net *n, const GState &s, const void *E, int32_t *running, hipStream_t st) {
    const int L = n->num_layers;
    const dim3 blk(256);
    for (int l = 0; l < L; ++l) {
        const WT *bih = n->b_ih ? (const WT *)n->b_ih[l] : nullptr, *bhh = n->b_hh ? (const WT *)n->b_hh[l] : nullptr;
        const dim3 g((unsigned)((s.H + 3) / 4));
        if (l == 0)
            hipLaunchKernelGGL((greedy_lstm_kernel<WT, true>), g, blk, 0, st, s, 0, n->embed_dim, (const WT *)n->embed,
                               (const WT *)n->w_ih[0], (const WT *)n->w_hh[0], bih, bhh);
        else
            hipLaunchKernelGGL((greedy_lstm_kernel<WT, false>), g, blk, 0, st, s, l, s.H, (const WT *)nullptr, (const WT *)n->w_ih[l],
                               (const WT *)n->w_hh[l], bih, bhh);
    }
    hipLaunchKernelGGL(greedy_matvec_kernel<WT>, dim3((unsigned)((s.Pd + 3) / 4)), blk, 0, st, s, s.Pd, s.H, (const float *)nullptr, true,
                       (const WT *)n->proj_w, (const WT *)n->proj_b, s.pred);
    hipLaunchKernelGGL(greedy_matvec_kernel<WT>, dim3((unsigned)((s.J + 3) / 4)), blk, 0, st, s, s.J, s.Pd, (const float *)s.pred, false,
                       (const WT *)n->pred_ffn_w, (const WT *)n->pred_ffn_b, s.P);
    hipLaunchKernelGGL(greedy_joint_kernel<WT>, dim3((unsigned)s.ns), blk, (size_t)GNB * s.J * sizeof(float), st, s, (const WT *)E,
                       (const WT *)n->out_w, (const WT *)n->out_b);
    hipLaunchKernelGGL(greedy_update_kernel, dim3(1), blk, 0, st, s, running);
}

}  // namespace
}  // namespace pafc

extern "C" {

size_t pafc_rnnt_greedy_workspace_bytes(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps) {
    if (!net || net->num_layers <= 0 || net->hidden <= 0 || net->pred_dim <= 0 || net->join_dim <= 0 || net->vocab <= 0) return 0;
    if (pafc::check_dims(B, T, n_steps, 0, net->vocab) != PAFC_OK) return 0;
    size_t bytes = 0;
    pafc::layout(nullptr, B, T, net->num_layers, net->hidden, net->pred_dim, net->join_dim, net->vocab, n_steps, 0, &bytes);
    return bytes;
}

int pafc_rnnt_greedy_init(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps, int blank_id, const int64_t *lens,
                          void *workspace, size_t workspace_bytes, pafc_stream_t stream) {
    int rc = pafc::rnnt_check_net(net);
    if (rc != PAFC_OK) return rc;
    if (!lens || !workspace) return PAFC_ERR_NULL_POINTER;
    rc = pafc::check_dims(B, T, n_steps, blank_id, net->vocab);
    if (rc != PAFC_OK) return rc;
    if (workspace_bytes < pafc_rnnt_greedy_workspace_bytes(net, B, T, n_steps)) return PAFC_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 255) != 0) return PAFC_ERR_ALIGNMENT;
    size_t bytes = 0;
    const pafc::GState s = pafc::layout(workspace, B, T, net->num_layers, net->hidden, net->pred_dim, net->join_dim, net->vocab, n_steps,
                                        blank_id, &bytes);
    hipLaunchKernelGGL(pafc::greedy_init_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, s, lens);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_rnnt_greedy_step(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps, int blank_id, const void *E, void *workspace,
                          size_t workspace_bytes, int32_t *running, pafc_stream_t stream) {
    int rc = pafc::rnnt_check_net(net);
    if (rc != PAFC_OK) return rc;
    if (!E || !workspace) return PAFC_ERR_NULL_POINTER;
    rc = pafc::check_dims(B, T, n_steps, blank_id, net->vocab);
    if (rc != PAFC_OK) return rc;
    if (workspace_bytes < pafc_rnnt_greedy_workspace_bytes(net, B, T, n_steps)) return PAFC_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 255) != 0 || !pafc::aligned16(E)) return PAFC_ERR_ALIGNMENT;
    size_t bytes = 0;
    const pafc::GState s = pafc::layout(workspace, B, T, net->num_layers, net->hidden, net->pred_dim, net->join_dim, net->vocab, n_steps,
                                        blank_id, &bytes);
    hipStream_t st = (hipStream_t)stream;
    if (net->dtype == PAFC_F32) pafc::launch_step<float>(net, s, E, running, st);
    else pafc::launch_step<pafc::bf16_t>(net, s, E, running, st);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_rnnt_greedy_finish(const pafc_rnnt_greedy_net *net, int B, int T, int n_steps, const void *workspace, size_t workspace_bytes,
                            int ld, int32_t *tokens, int32_t *frames, int32_t *ntok, double *score, int32_t *running,
                            pafc_stream_t stream) {
    if (!net || !workspace || !tokens || !ntok) return PAFC_ERR_NULL_POINTER;
    int rc = pafc::check_dims(B, T, n_steps, 0, net->vocab);
    if (rc != PAFC_OK) return rc;
    if (ld <= 0) return PAFC_ERR_BAD_DIMS;
    if (workspace_bytes < pafc_rnnt_greedy_workspace_bytes(net, B, T, n_steps)) return PAFC_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 255) != 0) return PAFC_ERR_ALIGNMENT;
    size_t bytes = 0;
    const pafc::GState s = pafc::layout(const_cast<void *>(workspace), B, T, net->num_layers, net->hidden, net->pred_dim, net->join_dim,
                                        net->vocab, n_steps, 0, &bytes);
    hipLaunchKernelGGL(pafc::greedy_finish_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, s, ld, tokens, frames, ntok,
                       score, running);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

size_t pafc_rnnt_greedy_stream_workspace_bytes(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps) {
    if (!net || net->num_layers <= 0 || net->hidden <= 0 || net->pred_dim <= 0 || net->join_dim <= 0 || net->vocab <= 0) return 0;
    if (pafc::check_dims(B, Tmax, n_steps, 0, net->vocab) != PAFC_OK) return 0;
    size_t bytes = 0;
    pafc::stream_layout(nullptr, net, B, Tmax, n_steps, 0, nullptr, &bytes);
    return bytes;
}

static int stream_check(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps, int blank_id, const void *workspace,
                        size_t workspace_bytes) {
    if (!net || !workspace) return PAFC_ERR_NULL_POINTER;
    int rc = pafc::check_dims(B, Tmax, n_steps, blank_id, net->vocab);
    if (rc != PAFC_OK) return rc;
    if (workspace_bytes < pafc_rnnt_greedy_stream_workspace_bytes(net, B, Tmax, n_steps)) return PAFC_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 255) != 0) return PAFC_ERR_ALIGNMENT;
    return PAFC_OK;
}

int pafc_rnnt_greedy_stream_reset(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps, int blank_id, const int32_t *row_mask,
                                  void *workspace, size_t workspace_bytes, pafc_stream_t stream) {
    int rc = pafc::rnnt_check_net(net);
    if (rc != PAFC_OK) return rc;
    rc = stream_check(net, B, Tmax, n_steps, blank_id, workspace, workspace_bytes);
    if (rc != PAFC_OK) return rc;
    size_t bytes = 0;
    int64_t *base = nullptr;
    const pafc::GState s = pafc::stream_layout(workspace, net, B, Tmax, n_steps, blank_id, &base, &bytes);
    hipLaunchKernelGGL(pafc::greedy_stream_reset_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, s, base, row_mask);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_rnnt_greedy_stream_feed(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps, int blank_id, const int64_t *nframes,
                                 void *workspace, size_t workspace_bytes, int32_t *running, pafc_stream_t stream) {
    int rc = pafc::rnnt_check_net(net);
    if (rc != PAFC_OK) return rc;
    if (!nframes) return PAFC_ERR_NULL_POINTER;
    rc = stream_check(net, B, Tmax, n_steps, blank_id, workspace, workspace_bytes);
    if (rc != PAFC_OK) return rc;
    size_t bytes = 0;
    int64_t *base = nullptr;
    const pafc::GState s = pafc::stream_layout(workspace, net, B, Tmax, n_steps, blank_id, &base, &bytes);
    hipLaunchKernelGGL(pafc::greedy_stream_feed_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, s, base, nframes, running);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_rnnt_greedy_stream_drain(const pafc_rnnt_greedy_net *net, int B, int Tmax, int n_steps, const void *workspace,
                                  size_t workspace_bytes, int ld, int32_t *tokens, int64_t *frames, int32_t *ntok, double *score,
                                  int32_t *running, pafc_stream_t stream) {
    if (!tokens || !ntok) return PAFC_ERR_NULL_POINTER;
    int rc = stream_check(net, B, Tmax, n_steps, 0, workspace, workspace_bytes);
    if (rc != PAFC_OK) return rc;
    if (ld <= 0) return PAFC_ERR_BAD_DIMS;
    size_t bytes = 0;
    int64_t *base = nullptr;
    const pafc::GState s = pafc::stream_layout(const_cast<void *>(workspace), net, B, Tmax, n_steps, 0, &base, &bytes);
    hipLaunchKernelGGL(pafc::greedy_stream_drain_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, s, base, ld, tokens,
                       frames, ntok, score, running);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

}  // extern "C"
