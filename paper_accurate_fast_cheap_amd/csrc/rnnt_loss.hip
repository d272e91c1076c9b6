// RNN-T joint + loss of the training step without the (rows, V) logits, on gfx950 (C ABI: include/pafc_encoder_ops.h:
// pafc_rnnt_joint_loss_*).
//
// Replaces TransducerJoint.forward_optimized (wenet/transducer/joint.py:111-149) + the optimized_transducer loss of
// Transducer._compute_loss (wenet/transducer/transducer.py:506-561) and their autograd for the paper's joint (pre-join
// projections, additive join, tanh, no post-join projection).  E = enc_ffn(encoder_out) (B, T, J) and P = pred_ffn(predictor_out)
// (B, U + 1, J) bf16; W (V, J) and b (V) bf16.  Lattice row r = (n, t, u) in forward_optimized's compacted order:
// r = off_n + t (U_n + 1) + u.  h_r = bf16(tanh(E[n][t] + P[n][u])) (add and tanh in fp32, one rounding), z_r = W h_r + b.
//
//   offsets   one thread: off_n = sum_{m < n} T_m (U_m + 1) from the device lengths (an utterance whose lengths do not fit the
//             padded operands gets no rows and a NaN loss)
//   join      H (R, J) bf16 = h_r, written once: the A operand of every product below and the tanh derivative
//   stats     H W^T + b on the matrix cores (the 128 x 128 x 64 tile loop of gemm_bf16.hip); the epilogue writes NO logits: per row
//             and 128-column tile the max and sum of exp, and z[blank], z[y_u] from whichever tile owns those columns
//   lse       one thread per row: lse_r from the tiles' partials
//   lattice   one block per utterance over anti-diagonals, fp32, "log 0" = -1e30: alpha, nll_n = -(alpha(T-1, U) +
//             lp_blank(T-1, U)), then beta and the per-node gradients g_B = d nll / d lp_blank, g_L = d nll / d lp_label
//   backward  in slabs of whole utterances: the stats product again with an epilogue that writes
//             dz = s_n (g_B [c = blank] + g_L [c = y] - (g_B + g_L) softmax(z)_c) bf16 into rows of Vp = V rounded up to 64
//             (tail zero), s_n = grad_out[n] * scale; dH = dz W (pafc_gemm_bf16_f32out against a zero-padded W^T, fp32);
//             dW, db += dz^T H (pafc_gemm_tn_bf16, summed over slabs in slab order); dpre = dH (1 - h^2) reduced in a fixed
//             order into dE[n][t] = sum_u dpre and dP[n][u] = sum_t dpre.
// No float atomics: forward and backward are bitwise reproducible.
//
// pafc_rnnt_score (include/pafc_search.h) scores n-best lists with the same join, stats and lse kernels: its rows are (utterance,
// frame, arc of the hypotheses' prefix trie) instead of (utterance, frame, label count), and its lattice kernel keeps the alpha
// pass only.  A hypothesis scored there has the bits of -nll of the training forward fed that hypothesis alone.
#include <math.h>
#include <vector>

#include "pafc_common.h"
#include "../../include/pafc_encoder_ops.h"
#include "../../include/pafc_search.h"

namespace pafc {
namespace {

constexpr int RBM = 128, RBN = 128, RBK = 64;
constexpr float NEG = -1e30f;     // "log 0", finite as in ctc_loss.hip

__device__ __forceinline__ bool utt_ok(int Tn, int Un, int T, int Up1, int ldy) {
    return Tn >= 1 && Tn <= T && Un >= 0 && Un + 1 <= Up1 && Un <= ldy;
}

// utterance that owns row r < off[B] (the largest n with off[n] <= r; utterances without rows share their offset with the next)
__device__ __forceinline__ int find_utt(const int64_t *off, int B, long r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    return m <= NEG ? NEG : m + logf(expf(a - m) + expf(b - m));
}

// 8 columns of h = bf16(tanh(e + p)): the add and tanh in fp32, one rounding (the join of the training forward and of the scorer)
__device__ __forceinline__ uint4 join8(const bf16_t *ep, const bf16_t *pp) {
    float e[8], p[8], h[8];
    Elem<bf16_t>::unpack(*reinterpret_cast<const uint4 *>(ep), e);
    Elem<bf16_t>::unpack(*reinterpret_cast<const uint4 *>(pp), p);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = tanhf(e[i] + p[i]);
    uint4 o;
    o.x = f32_to_bf16_bits(h[0]) | (f32_to_bf16_bits(h[1]) << 16);
    o.y = f32_to_bf16_bits(h[2]) | (f32_to_bf16_bits(h[3]) << 16);
    o.z = f32_to_bf16_bits(h[4]) | (f32_to_bf16_bits(h[5]) << 16);
    o.w = f32_to_bf16_bits(h[6]) | (f32_to_bf16_bits(h[7]) << 16);
    return o;
}

__global__ void rnnt_offsets_kernel(int B, int T, int Up1, int ldy, const int32_t *hlens, const int32_t *ylens, int64_t *off) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t acc = 0;
    for (int n = 0; n < B; ++n) {
        off[n] = acc;
        const int Tn = hlens[n], Un = ylens[n];
        if (utt_ok(Tn, Un, T, Up1, ldy)) acc += (int64_t)Tn * (Un + 1);
    }
    off[B] = acc;
}

// one thread per 8 columns of a row; rows beyond the lattice (r >= off[B]) are written as zeros
__global__ __launch_bounds__(256) void rnnt_join_kernel(long R, int B, int J, const bf16_t *E, long lde, long sE, const bf16_t *P,
                                                        long ldp, long sP, const int32_t *ylens, const int64_t *off, bf16_t *H) {
    const int cpr = J / 8;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= R * cpr) return;
    const long r = q / cpr;
    const int c = (int)(q % cpr) * 8;
    uint4 o = make_uint4(0, 0, 0, 0);
    if (r < off[B]) {
        const int n = find_utt(off, B, r);
        const int U1 = ylens[n] + 1;
        const long k = r - off[n], t = k / U1, u = k % U1;
        o = join8(E + n * sE + t * lde + c, P + n * sP + u * ldp + c);
    }
    *reinterpret_cast<uint4 *>(H + r * J + c) = o;
}

struct RnntGemm {
    const bf16_t *A;              // H + row0 * K: the rows of this launch
    const bf16_t *W, *bias;       // (N, K), (N) or null
    long M, row0, R;              // rows of this launch, its first lattice row, all rows
    int N, K, mtiles, ntiles;     // N = V, K = J
    int B, blank, ldy;
    const int64_t *ys, *off;
    const int32_t *ylens;
    // stats (MODE 0): per 128-column tile nt and row r: pmax / psum[nt * R + r]; zb[r] = z[blank], zy[r] = z[y_u] (u < U_n)
    float *pmax, *psum, *zb, *zy;
    // dz (MODE 1)
    const float *lse, *gB, *gL, *grad_out;
    float scale;
    bf16_t *dz;
    long ldz;                     // Vp
    // stats of the hypothesis scorer (MODE 0): null, or the label of row r, written by its join (-1: the row has none)
    const int32_t *rowlab;
};

// label of lattice row r (global), or -1 when the row has none (u = U_n) or lies beyond the lattice
__device__ __forceinline__ int row_label(const RnntGemm &p, long r, int *n_out) {
    *n_out = -1;
    if (r >= p.off[p.B]) return -1;
    const int n = find_utt(p.off, p.B, r);
    *n_out = n;
    const int Un = p.ylens[n];
    const int u = (int)((r - p.off[n]) % (Un + 1));
    return u < Un ? (int)p.ys[(long)n * p.ldy + u] : -1;
}

// 256 threads (2 x 2 waves), tile 128 x 128 x 64, MFMA 16x16x32 bf16, two LDS stages filled by LDS-DMA with the XOR swizzle on
// the source side: the loop of gemm_bf16_kernel<0>.  MODE 0: row statistics epilogue (the row's label from ys / ylens, or from
// rowlab when that is given: the arc tables of pafc_rnnt_score); MODE 1: dz epilogue.
template <int MODE>
__global__ __launch_bounds__(256, 2) void rnnt_gemm_kernel(const RnntGemm p) {
    extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
    constexpr int MI = 4, NI = 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const long nblk = (long)p.mtiles * p.ntiles;
    long bid = blockIdx.x;
    const long per = nblk / 8;
    if (bid < per * 8) bid = (bid % 8) * per + bid / 8;   // the N-tiles of one M-tile on one XCD (they share its A rows in L2)
    const int mt0 = (int)(bid / p.ntiles), nt0 = (int)(bid % p.ntiles);
    const long m0 = (long)mt0 * RBM;
    const int n0 = nt0 * RBN;

    const int sub = lane >> 3, pch = lane & 7;
    const bf16_t *a_src[MI];
    const bf16_t *w_src[NI];
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const int row = wave * (RBM / 4) + j * 8 + sub;
        long m = m0 + row;
        if (m >= p.M) m = p.M - 1;                          // clamped rows are computed, never used
        a_src[j] = p.A + m * p.K + 8 * (pch ^ (row & 7));
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int row = wave * (RBN / 4) + j * 8 + sub;
        const int n = min(n0 + row, p.N - 1);               // columns >= V are masked in the epilogue
        w_src[j] = p.W + (long)n * p.K + 8 * (pch ^ (row & 7));
    }
    const int iters = p.K / RBK;
    constexpr int STAGE = (RBM + RBN) * RBK;
    auto issue = [&](int it, int buf) {
        bf16_t *A = lds + buf * STAGE;
        bf16_t *Wt = A + RBM * RBK;
        const int koff = it * RBK;
#pragma unroll
        for (int j = 0; j < MI; ++j) global_to_lds16(a_src[j] + koff, A + (wave * (RBM / 4) + j * 8) * RBK);
#pragma unroll
        for (int j = 0; j < NI; ++j) global_to_lds16(w_src[j] + koff, Wt + (wave * (RBN / 4) + j * 8) * RBK);
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, kq = lane >> 4;
    issue(0, 0);
    for (int it = 0; it < iters; ++it) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (it + 1 < iters) issue(it + 1, (it + 1) & 1);
        const bf16_t *A = lds + (it & 1) * STAGE;
        const bf16_t *Wt = A + RBM * RBK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[MI], wf[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int row = wm * (RBM / 2) + i * 16 + fr;
                af[i] = *reinterpret_cast<const bf16x8 *>(A + row * RBK + (((ks * 4 + kq) ^ (row & 7)) * 8));
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int row = wn * (RBN / 2) + j * 16 + fr;
                wf[j] = *reinterpret_cast<const bf16x8 *>(Wt + row * RBK + (((ks * 4 + kq) ^ (row & 7)) * 8));
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], wf[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();   // the operand buffers are free

    // C/D layout: col = lane & 15 (n), row = 4 (lane >> 4) + reg (m)
    if constexpr (MODE == 0) {
        constexpr int LDF = RBN + 4;
        float *O = reinterpret_cast<float *>(lds);   // [128][132] fp32 logits of the tile (columns >= V never read)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int col = wn * (RBN / 2) + j * 16 + fr;
            const float bv = p.bias ? bf16_bits_to_f32(p.bias[min(n0 + col, p.N - 1)]) : 0.f;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) O[(wm * (RBM / 2) + i * 16 + 4 * kq + g) * LDF + col] = acc[i][j][g] + bv;
        }
        __syncthreads();
        // two threads per row (adjacent lanes), 64 columns each
        const int row = tid >> 1, half = tid & 1;
        const int cend = min(64, p.N - (n0 + half * 64));   // columns of this half below V (may be <= 0)
        const float *orow = O + row * LDF + half * 64;
        float mx = -INFINITY;
        for (int c = 0; c < cend; ++c) mx = fmaxf(mx, orow[c]);
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        float s = 0.f;
        for (int c = 0; c < cend; ++c) s += __expf(orow[c] - mx);
        s += __shfl_xor(s, 1, 64);
        const long m = m0 + row;
        if (half == 0 && m < p.M) {
            const long r = p.row0 + m;
            p.pmax[(long)nt0 * p.R + r] = mx;
            p.psum[(long)nt0 * p.R + r] = s;
            const float *full = O + row * LDF;
            if (p.blank >= n0 && p.blank < n0 + RBN) p.zb[r] = full[p.blank - n0];
            int n;
            const int y = p.rowlab ? p.rowlab[r] : row_label(p, r, &n);
            if (y >= n0 && y < n0 + RBN && y < p.N) p.zy[r] = full[y - n0];
        }
    } else {
        constexpr int LDO = RBN + 8;
        bf16_t *O = lds;                                                    // [128][136] bf16 dz of the tile
        float *ri = reinterpret_cast<float *>(lds + RBM * LDO);             // per row: lse, s g_B, s g_L, label
        if (tid < RBM) {
            const long m = m0 + tid;
            float l = 0.f, gb = 0.f, gl = 0.f;
            int y = -1;
            if (m < p.M) {
                const long r = p.row0 + m;
                int n;
                y = row_label(p, r, &n);
                if (n >= 0) {
                    const float s = p.grad_out[n] * p.scale;
                    l = p.lse[r]; gb = s * p.gB[r]; gl = s * p.gL[r];
                }
            }
            ri[4 * tid] = l; ri[4 * tid + 1] = gb; ri[4 * tid + 2] = gl; ri[4 * tid + 3] = __int_as_float(y);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int col = wn * (RBN / 2) + j * 16 + fr;
            const int c = n0 + col;
            const float bv = p.bias ? bf16_bits_to_f32(p.bias[min(c, p.N - 1)]) : 0.f;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = wm * (RBM / 2) + i * 16 + 4 * kq + g;
                    const float l = ri[4 * row], gb = ri[4 * row + 1], gl = ri[4 * row + 2];
                    const int y = __float_as_int(ri[4 * row + 3]);
                    float v = 0.f;
                    if (c < p.N)
                        v = (c == p.blank ? gb : 0.f) + (c == y ? gl : 0.f) - (gb + gl) * __expf(acc[i][j][g] + bv - l);
                    O[row * LDO + col] = (bf16_t)f32_to_bf16_bits(v);
                }
        }
        __syncthreads();
        constexpr int CPR = RBN / 8, RPP = 256 / CPR;
#pragma unroll
        for (int q = 0; q < RBM / RPP; ++q) {
            const int row = q * RPP + tid / CPR, c8 = (tid % CPR) * 8;
            const long m = m0 + row;
            if (m < p.M && n0 + c8 < p.ldz)
                *reinterpret_cast<uint4 *>(p.dz + m * p.ldz + n0 + c8) = *reinterpret_cast<const uint4 *>(O + row * LDO + c8);
        }
    }
}

// lse_r from the tiles' partials; g_B / g_L cleared (the lattice writes the rows of its utterances; null for the scorer, which
// has no gradients)
__global__ __launch_bounds__(256) void rnnt_lse_kernel(long R, int ntiles, const float *pmax, const float *psum, float *lse, float *gB,
                                                       float *gL) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float M = -INFINITY;
    for (int nt = 0; nt < ntiles; ++nt) M = fmaxf(M, pmax[(long)nt * R + r]);
    float s = 0.f;
    for (int nt = 0; nt < ntiles; ++nt) s += psum[(long)nt * R + r] * expf(pmax[(long)nt * R + r] - M);
    lse[r] = M + logf(s);
    if (gB) {
        gB[r] = 0.f;
        gL[r] = 0.f;
    }
}

// one block per utterance, a thread per label count u on each anti-diagonal d = t + u.  LDS: the previous diagonal's alpha,
// lp_blank, lp_label (then the next diagonal's beta) indexed by u, two buffers.
__global__ __launch_bounds__(256) void rnnt_lattice_kernel(long R, int B, int T, int Up1, const int32_t *hlens, const int32_t *ylens,
                                                           const int64_t *ys, int ldy, int V, const int64_t *off, const float *zb,
                                                           const float *zy, const float *lse, float *alpha, float *lpb, float *lpl,
                                                           float *gB, float *gL, float *nll) {
    extern __shared__ float sh[];                 // [2][3][Up1 + 1]
    __shared__ float ll_sh;
    const int n = blockIdx.x, Tn = hlens[n], Un = ylens[n];
    const long base = off[n];
    if (!utt_ok(Tn, Un, T, Up1, ldy) || base + (long)Tn * (Un + 1) > R) {   // lengths outside the operands, or a row count
        if (threadIdx.x == 0) nll[n] = __int_as_float(0x7fc00000);          // that disagrees with R: NaN, nothing touched
        return;
    }
    const int U1 = Un + 1, W = Up1 + 1;
    const int64_t *y = ys + (long)n * ldy;
    // ---- alpha ---------------------------------------------------------------------------------------------------------
    for (int d = 0; d < Tn + Un; ++d) {
        const float *pa = sh + ((d + 1) & 1) * 3 * W, *pb = pa + W, *pl = pb + W;
        float *ca = sh + (d & 1) * 3 * W, *cb = ca + W, *cl = cb + W;
        for (int u = threadIdx.x; u < U1; u += blockDim.x) {
            const int t = d - u;
            float a = NEG, b = NEG, l = NEG;
            if (t >= 0 && t < Tn) {
                const long r = base + (long)t * U1 + u;
                const float ls = lse[r];
                b = zb[r] - ls;
                if (u < Un) {
                    const long c = y[u];
                    l = (c >= 0 && c < V) ? zy[r] - ls : NEG;
                }
                if (d == 0) a = 0.f;
                else a = lse2(t >= 1 ? pa[u] + pb[u] : NEG, u >= 1 ? pa[u - 1] + pl[u - 1] : NEG);
                alpha[r] = a; lpb[r] = b; lpl[r] = l;
                if (t == Tn - 1 && u == Un) ll_sh = a + b;
            }
            ca[u] = a; cb[u] = b; cl[u] = l;
        }
        __syncthreads();
    }
    const float ll = ll_sh;
    if (threadIdx.x == 0) nll[n] = -ll;
    // ---- beta and the gradients ------------------------------------------------------------------------------------------
    // the diagonal Tn + Un holds only the virtual end (Tn, Un) with beta 0; index U1 is always "log 0"
    {
        float *nb = sh + ((Tn + Un) & 1) * 3 * W;
        for (int u = threadIdx.x; u <= U1; u += blockDim.x) nb[u] = u == Un ? 0.f : NEG;
        float *cb0 = sh + ((Tn + Un + 1) & 1) * 3 * W;
        if (threadIdx.x == 0) cb0[U1] = NEG;
    }
    __syncthreads();
    for (int d = Tn + Un - 1; d >= 0; --d) {
        const float *nb = sh + ((d + 1) & 1) * 3 * W;
        float *cb = sh + (d & 1) * 3 * W;
        for (int u = threadIdx.x; u < U1; u += blockDim.x) {
            const int t = d - u;
            float be = NEG;
            if (t >= 0 && t < Tn) {
                const long r = base + (long)t * U1 + u;
                const float a = alpha[r], b = lpb[r], l = lpl[r];
                const float via_b = b + nb[u], via_l = u < Un ? l + nb[u + 1] : NEG;
                be = lse2(via_b, via_l);
                gB[r] = -expf(fminf(a + via_b - ll, 0.f));
                gL[r] = u < Un ? -expf(fminf(a + via_l - ll, 0.f)) : 0.f;
            }
            cb[u] = be;
        }
        if (threadIdx.x == 0) cb[U1] = NEG;
        __syncthreads();
    }
}

// Wt (J, Vp) = W^T with zero columns V .. Vp - 1
__global__ __launch_bounds__(256) void rnnt_wt_kernel(int V, int J, int Vp, const bf16_t *W, bf16_t *Wt) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)J * Vp) return;
    const int j = (int)(q / Vp), c = (int)(q % Vp);
    Wt[q] = c < V ? W[(long)c * J + j] : (bf16_t)0;
}

__global__ __launch_bounds__(256) void rnnt_add_kernel(long n, float *acc, const float *x) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q < n) acc[q] += x[q];
}

// dE[n][t] = sum_u dH[r] (1 - h_r^2) in u order, for the utterances [n0, n1) of a slab whose first row is row0
template <typename OT>
__global__ __launch_bounds__(256) void rnnt_dE_kernel(int n0, int T, int J, const int32_t *hlens, const int32_t *ylens,
                                                      const int64_t *off, long row0, long rows, const float *dH, const bf16_t *H, OT *dE) {
    const int n = n0 + blockIdx.y, t = blockIdx.x, Tn = hlens[n];
    if (t >= Tn || off[n + 1] == off[n] || off[n] < row0 || off[n + 1] > row0 + rows) return;   // (host and device offsets disagree)
    const int U1 = ylens[n] + 1;
    const long r0 = off[n] + (long)t * U1;
    for (int j = threadIdx.x; j < J; j += 256) {
        float s = 0.f;
        for (int u = 0; u < U1; ++u) {
            const float h = bf16_bits_to_f32(H[(r0 + u) * J + j]);
            s += dH[(r0 + u - row0) * J + j] * (1.f - h * h);
        }
        Elem<OT>::store(dE + ((long)n * T + t) * J + j, s);
    }
}

// dP[n][u] = sum_t dH[r] (1 - h_r^2) in t order
template <typename OT>
__global__ __launch_bounds__(256) void rnnt_dP_kernel(int n0, int Up1, int J, const int32_t *hlens, const int32_t *ylens,
                                                      const int64_t *off, long row0, long rows, const float *dH, const bf16_t *H, OT *dP) {
    const int n = n0 + blockIdx.y, u = blockIdx.x, U1 = ylens[n] + 1;
    if (u >= U1 || off[n + 1] == off[n] || off[n] < row0 || off[n + 1] > row0 + rows) return;
    const int Tn = hlens[n];
    for (int j = threadIdx.x; j < J; j += 256) {
        float s = 0.f;
        for (int t = 0; t < Tn; ++t) {
            const long r = off[n] + (long)t * U1 + u;
            const float h = bf16_bits_to_f32(H[r * J + j]);
            s += dH[(r - row0) * J + j] * (1.f - h * h);
        }
        Elem<OT>::store(dP + ((long)n * Up1 + u) * J + j, s);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

struct FwdLayout {
    int64_t *off;
    bf16_t *H;
    float *pmax, *psum, *zb, *zy, *lse, *alpha, *lpb, *lpl, *gB, *gL;
    size_t bytes;
};

FwdLayout fwd_layout(void *ws, int B, int J, int V, long R) {
    FwdLayout L{};
    char *p = (char *)ws;
    size_t o = 0;
    const int nt = (V + RBN - 1) / RBN;
    auto take = [&](size_t b) { char *q = p ? p + o : nullptr; o += al256(b); return q; };
    L.off = (int64_t *)take((size_t)(B + 1) * sizeof(int64_t));
    L.H = (bf16_t *)take((size_t)R * J * sizeof(bf16_t));
    L.pmax = (float *)take((size_t)nt * R * sizeof(float));
    L.psum = (float *)take((size_t)nt * R * sizeof(float));
    float **rows[] = {&L.zb, &L.zy, &L.lse, &L.alpha, &L.lpb, &L.lpl, &L.gB, &L.gL};
    for (float **f : rows) *f = (float *)take((size_t)R * sizeof(float));
    L.bytes = o;
    return L;
}

// slabs: consecutive whole utterances with at most slab_rows rows; returns the count (-1: an utterance alone exceeds slab_rows)
int plan_slabs(int B, const int64_t *row_off, long slab_rows, int *first /* B + 1 */) {
    int ns = 0, n = 0;
    while (n < B) {
        while (n < B && row_off[n + 1] == row_off[n]) ++n;            // utterances without rows belong to no slab
        if (n >= B) break;
        first[ns++] = n;
        const int64_t start = row_off[n];
        if (row_off[n + 1] - start > slab_rows) return -1;
        while (n < B && row_off[n + 1] - start <= slab_rows) ++n;
    }
    first[ns] = B;
    return ns;
}

struct BwdLayout {
    bf16_t *Wt, *dz;
    float *dH, *dWt, *dbt;
    void *tn;
    size_t tn_bytes, bytes;
};

BwdLayout bwd_layout(void *scratch, int J, int V, long slab_rows, size_t tn_bytes) {
    BwdLayout L{};
    char *p = (char *)scratch;
    size_t o = 0;
    const int Vp = (V + 63) / 64 * 64;
    auto take = [&](size_t b) { char *q = p ? p + o : nullptr; o += al256(b); return q; };
    L.Wt = (bf16_t *)take((size_t)J * Vp * sizeof(bf16_t));
    L.dz = (bf16_t *)take((size_t)slab_rows * Vp * sizeof(bf16_t));
    L.dH = (float *)take((size_t)slab_rows * J * sizeof(float));
    L.dWt = (float *)take((size_t)V * J * sizeof(float));
    L.dbt = (float *)take((size_t)V * sizeof(float));
    L.tn = take(tn_bytes);
    L.tn_bytes = tn_bytes;
    L.bytes = o;
    return L;
}

constexpr int kMaxB = 65535;

int check_common(int B, int T, int Up1, int J, int V, const void *E, long lde, long sE, const void *P, long ldp, long sP, const void *W,
                 const int32_t *hlens, const int32_t *ylens, const int64_t *ys, int ldy, int blank, long R) {
    if (!E || !P || !W || !hlens || !ylens || !ys) return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || B > kMaxB || T <= 0 || Up1 <= 0 || J <= 0 || V <= 0 || R <= 0 || ldy < 0 || lde < J || ldp < J || sE < (long)(T - 1) * lde + J ||
        sP < (long)(Up1 - 1) * ldp + J || blank < 0 || blank >= V)
        return PAFC_ERR_BAD_DIMS;
    if (J % 64 || V % 8 || V < 8) return PAFC_ERR_UNSUPPORTED;
    if ((size_t)6 * (Up1 + 1) * sizeof(float) > 60 * 1024) return PAFC_ERR_UNSUPPORTED;     // lattice LDS
    const long mt = (R + RBM - 1) / RBM, nt = (V + RBN - 1) / RBN;
    if (mt * nt > 0x7fffffffL || R * (J / 8) / 256 > 0x7fffffffL) return PAFC_ERR_UNSUPPORTED;
    if ((lde | sE | ldp | sP) % 8) return PAFC_ERR_ALIGNMENT;
    if ((((uintptr_t)E | (uintptr_t)P | (uintptr_t)W) & 15) != 0) return PAFC_ERR_ALIGNMENT;
    return PAFC_OK;
}

const size_t kGemmLds = (size_t)RBM * (RBN + 4) * sizeof(float);   // 66 KiB: the fp32 tile of the stats epilogue (> the 64 KiB ring)

int launch_gemm(int mode, const RnntGemm &g, hipStream_t s) {
    const void *k = mode == 0 ? (const void *)rnnt_gemm_kernel<0> : (const void *)rnnt_gemm_kernel<1>;
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGemmLds) != hipSuccess) return PAFC_ERR_LAUNCH;
    const dim3 grid((unsigned)((long)g.mtiles * g.ntiles));
    if (mode == 0) hipLaunchKernelGGL(rnnt_gemm_kernel<0>, grid, dim3(256), kGemmLds, s, g);
    else hipLaunchKernelGGL(rnnt_gemm_kernel<1>, grid, dim3(256), kGemmLds, s, g);
    return PAFC_OK;
}


// ---- hypothesis scorer (pafc_rnnt_score, include/pafc_search.h) ------------------------------------------------------------------
// The packed int32 tables of one batch of n-best lists, in this order (transducer/search/rescoring.py builds them).  The same
// view serves the host copy (validation, sizing) and the device copy (kernels).
struct ScoreTab {
    const int32_t *utt_enc, *utt_T;       // (nutt) row of E / hlens, and frames T_b
    const int32_t *arc_off, *hyp_off;     // (nutt + 1) first arc / first hypothesis of utterance b
    const int32_t *arc_prow, *arc_label;  // (narc) row of Pnode of the arc's node, its label or -1
    const int32_t *hyp_utt, *hyp_len;     // (nhyp)
    const int32_t *col_off;               // (nhyp + 1) first entry of col of hypothesis n
    const int32_t *col;                   // (ncol) column (arc of its utterance) of position u
};

inline ScoreTab score_tab(const int32_t *t, int nutt, int nhyp, int narc) {
    ScoreTab S;
    S.utt_enc = t; t += nutt;
    S.utt_T = t; t += nutt;
    S.arc_off = t; t += nutt + 1;
    S.hyp_off = t; t += nutt + 1;
    S.arc_prow = t; t += narc;
    S.arc_label = t; t += narc;
    S.hyp_utt = t; t += nhyp;
    S.hyp_len = t; t += nhyp;
    S.col_off = t; t += nhyp + 1;
    S.col = t;
    return S;
}

// one thread: off[i] = rows of the utterances [utt0, utt0 + i) of the group, T_b K_b each (the tables' T_b: validated on the host)
__global__ void rnnt_score_offsets_kernel(ScoreTab S, int utt0, int nu, int64_t *off) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t acc = 0;
    for (int i = 0; i < nu; ++i) {
        off[i] = acc;
        const int b = utt0 + i;
        const int K = S.arc_off[b + 1] - S.arc_off[b];
        if (K > 0) acc += (int64_t)S.utt_T[b] * K;
    }
    off[nu] = acc;
}

// rnnt_join_kernel over arcs: row r = off_b + t K_b + k is h = join8(E[enc_b][t], Pnode[prow[k]]); the thread of column 0 also
// writes the row's label
__global__ __launch_bounds__(256) void rnnt_score_join_kernel(long R, int utt0, int nu, int J, const bf16_t *E, long lde, long sE,
                                                              const bf16_t *P, long ldp, ScoreTab S, const int64_t *off, bf16_t *H,
                                                              int32_t *rowlab) {
    const int cpr = J / 8;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= R * cpr) return;
    const long r = q / cpr;
    const int c = (int)(q % cpr) * 8;
    uint4 o = make_uint4(0, 0, 0, 0);
    int lab = -1;
    if (r < off[nu]) {
        const int i = find_utt(off, nu, r), b = utt0 + i;
        const int a0 = S.arc_off[b], K = S.arc_off[b + 1] - a0;
        const long k = r - off[i], t = k / K;
        const int a = a0 + (int)(k % K);
        o = join8(E + S.utt_enc[b] * sE + t * lde + c, P + S.arc_prow[a] * ldp + c);
        lab = S.arc_label[a];
    }
    *reinterpret_cast<uint4 *>(H + r * J + c) = o;
    if (c == 0) rowlab[r] = lab;
}

// one block per hypothesis, a thread per label count u on each anti-diagonal d = t + u: the alpha pass of rnnt_lattice_kernel
// (the same fp32 recurrence, operand order and "log 0") with lp_blank / lp_label read through the hypothesis's columns; nothing
// but the score is written.  LDS: alpha, lp_blank, lp_label of the previous diagonal indexed by u, two buffers.
__global__ __launch_bounds__(256) void rnnt_score_lattice_kernel(long R, int Benc, int T, int Umax1, int utt0, int hyp0, ScoreTab S,
                                                                 const int32_t *hlens, const int64_t *off, const float *zb,
                                                                 const float *zy, const float *lse, float *score) {
    extern __shared__ float sh[];                 // [2][3][Umax1 + 1]
    __shared__ float ll_sh;
    const int n = hyp0 + blockIdx.x, b = S.hyp_utt[n], Un = S.hyp_len[n];
    const int Tn = S.utt_T[b], a0 = S.arc_off[b], K = S.arc_off[b + 1] - a0;
    const long base = off[b - utt0];
    if ((hlens && hlens[S.utt_enc[b]] != Tn) || Tn < 1 || Tn > T || Un + 1 > Umax1 || base + (long)Tn * K > R) {
        if (threadIdx.x == 0) score[n] = __int_as_float(0x7fc00000);   // the device length is outside E or not the tables': NaN
        return;
    }
    const int U1 = Un + 1, W = Umax1 + 1;
    const int32_t *col = S.col + S.col_off[n];
    for (int d = 0; d < Tn + Un; ++d) {
        const float *pa = sh + ((d + 1) & 1) * 3 * W, *pb = pa + W, *pl = pb + W;
        float *ca = sh + (d & 1) * 3 * W, *cb = ca + W, *cl = cb + W;
        for (int u = threadIdx.x; u < U1; u += blockDim.x) {
            const int t = d - u;
            float a = NEG, bl = NEG, l = NEG;
            if (t >= 0 && t < Tn) {
                const long r = base + (long)t * K + col[u];
                const float ls = lse[r];
                bl = zb[r] - ls;
                if (u < Un) l = zy[r] - ls;
                if (d == 0) a = 0.f;
                else a = lse2(t >= 1 ? pa[u] + pb[u] : NEG, u >= 1 ? pa[u - 1] + pl[u - 1] : NEG);
                if (t == Tn - 1 && u == Un) ll_sh = a + bl;
            }
            ca[u] = a; cb[u] = bl; cl[u] = l;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) score[n] = ll_sh;
}

struct ScoreLayout {
    int64_t *off;
    bf16_t *H;
    float *pmax, *psum, *zb, *zy, *lse;
    int32_t *rowlab;
    size_t bytes;
};

ScoreLayout score_layout(void *ws, int nu, int J, int V, long R) {
    ScoreLayout L{};
    char *p = (char *)ws;
    size_t o = 0;
    const int nt = (V + RBN - 1) / RBN;
    auto take = [&](size_t b) { char *q = p ? p + o : nullptr; o += al256(b); return q; };
    L.off = (int64_t *)take((size_t)(nu + 1) * sizeof(int64_t));
    L.H = (bf16_t *)take((size_t)R * J * sizeof(bf16_t));
    L.pmax = (float *)take((size_t)nt * R * sizeof(float));
    L.psum = (float *)take((size_t)nt * R * sizeof(float));
    float **rows[] = {&L.zb, &L.zy, &L.lse};
    for (float **f : rows) *f = (float *)take((size_t)R * sizeof(float));
    L.rowlab = (int32_t *)take((size_t)R * sizeof(int32_t));
    L.bytes = o;
    return L;
}

constexpr int kMaxScoreU1 = 2559;     // U + 1: the lattice LDS of the training forward
}  // namespace
}  // namespace pafc

extern "C" {

size_t pafc_rnnt_joint_loss_workspace_bytes(int B, int J, int V, long R, long slab_rows, const int64_t *row_off, int backward) {
    if (B <= 0 || J <= 0 || V <= 0 || R <= 0) return 0;
    if (!backward) return pafc::fwd_layout(nullptr, B, J, V, R).bytes;
    if (!row_off || slab_rows <= 0 || B > pafc::kMaxB) return 0;
    std::vector<int> first(B + 1);
    const int ns = pafc::plan_slabs(B, row_off, slab_rows, first.data());
    if (ns < 0) return 0;
    size_t tn = 0;
    for (int i = 0; i < ns; ++i) {
        const size_t b = pafc_gemm_tn_batched_workspace_bytes(row_off[first[i + 1]] - row_off[first[i]], V, J, 1);
        if (b > tn) tn = b;
    }
    return pafc::bwd_layout(nullptr, J, V, slab_rows, tn).bytes;
}

int pafc_rnnt_joint_loss_forward(int B, int T, int Up1, int J, int V, const void *E, long lde, long strideE, const void *P, long ldp,
                                 long strideP, const void *W, const void *bias, const int32_t *hlens, const int32_t *ylens,
                                 const int64_t *ys, int ldy, int blank, long R, float *nll, void *workspace, size_t workspace_bytes,
                                 pafc_stream_t stream) {
    if (!nll || !workspace) return PAFC_ERR_NULL_POINTER;
    const int rc = pafc::check_common(B, T, Up1, J, V, E, lde, strideE, P, ldp, strideP, W, hlens, ylens, ys, ldy, blank, R);
    if (rc != PAFC_OK) return rc;
    if (workspace_bytes < pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, 0, nullptr, 0)) return PAFC_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 255) != 0) return PAFC_ERR_ALIGNMENT;
    using namespace pafc;
    const FwdLayout L = fwd_layout(workspace, B, J, V, R);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rnnt_offsets_kernel, dim3(1), dim3(64), 0, s, B, T, Up1, ldy, hlens, ylens, L.off);
    const long q = R * (J / 8);
    hipLaunchKernelGGL(rnnt_join_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, s, R, B, J, (const bf16_t *)E, lde, strideE,
                       (const bf16_t *)P, ldp, strideP, ylens, L.off, L.H);
    RnntGemm g{};
    g.A = L.H; g.W = (const bf16_t *)W; g.bias = (const bf16_t *)bias;
    g.M = R; g.row0 = 0; g.R = R; g.N = V; g.K = J;
    g.mtiles = (int)((R + RBM - 1) / RBM); g.ntiles = (V + RBN - 1) / RBN;
    g.B = B; g.blank = blank; g.ldy = ldy; g.ys = ys; g.off = L.off; g.ylens = ylens;
    g.pmax = L.pmax; g.psum = L.psum; g.zb = L.zb; g.zy = L.zy;
    if (launch_gemm(0, g, s) != PAFC_OK) return PAFC_ERR_LAUNCH;
    hipLaunchKernelGGL(rnnt_lse_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, R, g.ntiles, L.pmax, L.psum, L.lse, L.gB,
                       L.gL);
    hipLaunchKernelGGL(rnnt_lattice_kernel, dim3(B), dim3(Up1 <= 64 ? 64 : Up1 <= 128 ? 128 : 256),
                       (size_t)6 * (Up1 + 1) * sizeof(float), s, R, B, T, Up1, hlens, ylens, ys, ldy, V, L.off, L.zb, L.zy, L.lse,
                       L.alpha, L.lpb, L.lpl, L.gB, L.gL, nll);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_rnnt_joint_loss_backward(int B, int T, int Up1, int J, int V, const void *E, long lde, long strideE, const void *P, long ldp,
                                  long strideP, const void *W, const void *bias, const int32_t *hlens, const int32_t *ylens,
                                  const int64_t *ys, int ldy, int blank, long R, const int64_t *row_off, long slab_rows,
                                  const float *grad_out, float scale, int grad_dtype, void *dE, void *dP, float *dW, float *db,
                                  const void *workspace, size_t workspace_bytes, void *scratch, size_t scratch_bytes,
                                  pafc_stream_t stream) {
    if (!row_off || !grad_out || !dE || !dP || !dW || !workspace || !scratch) return PAFC_ERR_NULL_POINTER;
    const int rc = pafc::check_common(B, T, Up1, J, V, E, lde, strideE, P, ldp, strideP, W, hlens, ylens, ys, ldy, blank, R);
    if (rc != PAFC_OK) return rc;
    if (grad_dtype != PAFC_F32 && grad_dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (row_off[0] != 0 || row_off[B] != R || slab_rows <= 0) return PAFC_ERR_BAD_DIMS;
    for (int n = 0; n < B; ++n)
        if (row_off[n + 1] < row_off[n]) return PAFC_ERR_BAD_DIMS;
    if (workspace_bytes < pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, 0, nullptr, 0)) return PAFC_ERR_WORKSPACE;
    const size_t need = pafc_rnnt_joint_loss_workspace_bytes(B, J, V, R, slab_rows, row_off, 1);
    if (need == 0) return PAFC_ERR_UNSUPPORTED;                    // an utterance alone has more rows than slab_rows
    if (scratch_bytes < need) return PAFC_ERR_WORKSPACE;
    if ((((uintptr_t)workspace | (uintptr_t)scratch) & 255) != 0 || (((uintptr_t)dW | (uintptr_t)db) & 15) != 0)
        return PAFC_ERR_ALIGNMENT;
    using namespace pafc;
    std::vector<int> first(B + 1);
    const int ns = plan_slabs(B, row_off, slab_rows, first.data());
    const int Vp = (V + 63) / 64 * 64;
    size_t tn = 0;
    for (int i = 0; i < ns; ++i) {
        const size_t b = pafc_gemm_tn_batched_workspace_bytes(row_off[first[i + 1]] - row_off[first[i]], V, J, 1);
        if (b > tn) tn = b;
    }
    const FwdLayout F = fwd_layout(const_cast<void *>(workspace), B, J, V, R);
    const BwdLayout S = bwd_layout(scratch, J, V, slab_rows, tn);
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = grad_dtype == PAFC_F32 ? 4 : 2;
    if (hipMemsetAsync(dE, 0, (size_t)B * T * J * esz, s) != hipSuccess || hipMemsetAsync(dP, 0, (size_t)B * Up1 * J * esz, s) != hipSuccess)
        return PAFC_ERR_LAUNCH;
    if (ns == 0) {                                                 // no lattice rows at all
        if (hipMemsetAsync(dW, 0, (size_t)V * J * sizeof(float), s) != hipSuccess) return PAFC_ERR_LAUNCH;
        if (db && hipMemsetAsync(db, 0, (size_t)V * sizeof(float), s) != hipSuccess) return PAFC_ERR_LAUNCH;
        return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
    }
    const long nwt = (long)J * Vp;
    hipLaunchKernelGGL(rnnt_wt_kernel, dim3((unsigned)((nwt + 255) / 256)), dim3(256), 0, s, V, J, Vp, (const bf16_t *)W, S.Wt);
    for (int i = 0; i < ns; ++i) {
        const int u0 = first[i], u1 = first[i + 1];
        const long row0 = row_off[u0], rows = row_off[u1] - row0;
        RnntGemm g{};
        g.A = F.H + row0 * J; g.W = (const bf16_t *)W; g.bias = (const bf16_t *)bias;
        g.M = rows; g.row0 = row0; g.R = R; g.N = V; g.K = J;
        g.mtiles = (int)((rows + RBM - 1) / RBM); g.ntiles = (V + RBN - 1) / RBN;
        g.B = B; g.blank = blank; g.ldy = ldy; g.ys = ys; g.off = F.off; g.ylens = ylens;
        g.lse = F.lse; g.gB = F.gB; g.gL = F.gL; g.grad_out = grad_out; g.scale = scale; g.dz = S.dz; g.ldz = Vp;
        if (launch_gemm(1, g, s) != PAFC_OK) return PAFC_ERR_LAUNCH;
        int e = pafc_gemm_bf16_f32out(rows, J, Vp, S.dz, Vp, 0, S.Wt, Vp, nullptr, nullptr, 0, S.dH, 1, J, 0, 1.f, 0, nullptr, 0, stream);
        if (e != PAFC_OK) return e;
        float *dw_i = i == 0 ? dW : S.dWt, *db_i = db ? (i == 0 ? db : S.dbt) : nullptr;
        e = pafc_gemm_tn_bf16_batched(rows, V, J, 1, S.dz, Vp, 0, F.H + row0 * J, J, 0, dw_i, db_i, PAFC_F32, S.tn, S.tn_bytes, stream);
        if (e != PAFC_OK) return e;
        if (i > 0) {                                               // fp32 sums in slab order
            const long nw = (long)V * J;
            hipLaunchKernelGGL(rnnt_add_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, nw, dW, (const float *)S.dWt);
            if (db) hipLaunchKernelGGL(rnnt_add_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, (long)V, db, (const float *)S.dbt);
        }
        const dim3 ge(T, u1 - u0), gp(Up1, u1 - u0);
        if (grad_dtype == PAFC_F32) {
            hipLaunchKernelGGL(rnnt_dE_kernel<float>, ge, dim3(256), 0, s, u0, T, J, hlens, ylens, F.off, row0, rows, S.dH, F.H, (float *)dE);
            hipLaunchKernelGGL(rnnt_dP_kernel<float>, gp, dim3(256), 0, s, u0, Up1, J, hlens, ylens, F.off, row0, rows, S.dH, F.H, (float *)dP);
        } else {
            hipLaunchKernelGGL(rnnt_dE_kernel<bf16_t>, ge, dim3(256), 0, s, u0, T, J, hlens, ylens, F.off, row0, rows, S.dH, F.H, (bf16_t *)dE);
            hipLaunchKernelGGL(rnnt_dP_kernel<bf16_t>, gp, dim3(256), 0, s, u0, Up1, J, hlens, ylens, F.off, row0, rows, S.dH, F.H, (bf16_t *)dP);
        }
    }
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

size_t pafc_rnnt_score_workspace_bytes(int nutt, int J, int V, long rows) {
    if (nutt <= 0 || J <= 0 || V <= 0 || rows <= 0) return 0;
    return pafc::score_layout(nullptr, nutt, J, V, rows).bytes;
}

int pafc_rnnt_score(int Benc, int T, int J, int V, const void *E, long lde, long strideE, const void *Pnode, long ldp, long prows,
                    const void *W, const void *bias, const int32_t *hlens, int nutt, int nhyp, int narc, int ncol,
                    const int32_t *tab_host, const int32_t *tab_dev, int utt0, int utt1, int blank, float *score, void *workspace,
                    size_t workspace_bytes, pafc_stream_t stream) {
    using namespace pafc;
    if (!E || !Pnode || !W || !tab_host || !tab_dev || !score || !workspace) return PAFC_ERR_NULL_POINTER;
    if (Benc <= 0 || T <= 0 || J <= 0 || V <= 0 || prows <= 0 || nutt <= 0 || nutt > kMaxB || nhyp < 0 || narc < 0 || ncol < 0 ||
        utt0 < 0 || utt1 <= utt0 || utt1 > nutt || lde < J || ldp < J || strideE < (long)(T - 1) * lde + J || blank < 0 || blank >= V)
        return PAFC_ERR_BAD_DIMS;
    if (J % 64 || V % 8 || V < 8) return PAFC_ERR_UNSUPPORTED;
    if ((lde | strideE | ldp) % 8) return PAFC_ERR_ALIGNMENT;
    if ((((uintptr_t)E | (uintptr_t)Pnode | (uintptr_t)W) & 15) != 0 || ((uintptr_t)workspace & 255) != 0) return PAFC_ERR_ALIGNMENT;
    // ---- the tables of this group, on the host copy: everything a kernel indexes with is in range ----
    const ScoreTab S = score_tab(tab_host, nutt, nhyp, narc);
    long R = 0;
    int Umax1 = 1;
    for (int b = utt0; b < utt1; ++b) {
        const int a0 = S.arc_off[b], a1 = S.arc_off[b + 1], h0 = S.hyp_off[b], h1 = S.hyp_off[b + 1];
        if (a0 < 0 || a1 < a0 || a1 > narc || h0 < 0 || h1 < h0 || h1 > nhyp) return PAFC_ERR_BAD_DIMS;
        if ((h1 > h0) != (a1 > a0)) return PAFC_ERR_BAD_DIMS;                 // arcs without hypotheses, or the reverse
        const int K = a1 - a0;
        if (K == 0) continue;                                                 // an utterance without hypotheses has no rows
        if (S.utt_enc[b] < 0 || S.utt_enc[b] >= Benc || S.utt_T[b] < 1 || S.utt_T[b] > T) return PAFC_ERR_BAD_DIMS;
        for (int a = a0; a < a1; ++a)
            if (S.arc_prow[a] < 0 || S.arc_prow[a] >= prows || S.arc_label[a] < -1 || S.arc_label[a] >= V) return PAFC_ERR_BAD_DIMS;
        for (int n = h0; n < h1; ++n) {
            const int U = S.hyp_len[n], c0 = S.col_off[n];
            if (S.hyp_utt[n] != b || U < 0 || c0 < 0 || S.col_off[n + 1] - c0 != U + 1 || S.col_off[n + 1] > ncol) return PAFC_ERR_BAD_DIMS;
            if (U + 1 > kMaxScoreU1) return PAFC_ERR_UNSUPPORTED;
            for (int u = 0; u <= U; ++u) {
                const int k = S.col[c0 + u];
                if (k < 0 || k >= K || (u < U && S.arc_label[a0 + k] < 0)) return PAFC_ERR_BAD_DIMS;
            }
            if (U + 1 > Umax1) Umax1 = U + 1;
        }
        R += (long)S.utt_T[b] * K;
    }
    const int hyp0 = S.hyp_off[utt0], nh = S.hyp_off[utt1] - hyp0, nu = utt1 - utt0;
    if (nh == 0) return PAFC_OK;                                              // a group without hypotheses has no rows
    const long mt = (R + RBM - 1) / RBM, ntl = (V + RBN - 1) / RBN;
    if (mt * ntl > 0x7fffffffL || R * (J / 8) / 256 > 0x7fffffffL) return PAFC_ERR_UNSUPPORTED;
    if (workspace_bytes < pafc_rnnt_score_workspace_bytes(nu, J, V, R)) return PAFC_ERR_WORKSPACE;
    // ---- device ----
    const ScoreTab D = score_tab(tab_dev, nutt, nhyp, narc);
    const ScoreLayout L = score_layout(workspace, nu, J, V, R);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rnnt_score_offsets_kernel, dim3(1), dim3(64), 0, s, D, utt0, nu, L.off);
    const long q = R * (J / 8);
    hipLaunchKernelGGL(rnnt_score_join_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, s, R, utt0, nu, J, (const bf16_t *)E,
                       lde, strideE, (const bf16_t *)Pnode, ldp, D, L.off, L.H, L.rowlab);
    RnntGemm g{};
    g.A = L.H; g.W = (const bf16_t *)W; g.bias = (const bf16_t *)bias;
    g.M = R; g.row0 = 0; g.R = R; g.N = V; g.K = J;
    g.mtiles = (int)mt; g.ntiles = (int)ntl;
    g.blank = blank; g.rowlab = L.rowlab;
    g.pmax = L.pmax; g.psum = L.psum; g.zb = L.zb; g.zy = L.zy;
    if (launch_gemm(0, g, s) != PAFC_OK) return PAFC_ERR_LAUNCH;
    hipLaunchKernelGGL(rnnt_lse_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, R, g.ntiles, L.pmax, L.psum, L.lse,
                       (float *)nullptr, (float *)nullptr);
    hipLaunchKernelGGL(rnnt_score_lattice_kernel, dim3(nh), dim3(Umax1 <= 64 ? 64 : Umax1 <= 128 ? 128 : 256),
                       (size_t)6 * (Umax1 + 1) * sizeof(float), s, R, Benc, T, Umax1, utt0, hyp0, D, hlens, L.off, L.zb, L.zy, L.lse,
                       score);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

}  // extern "C"
