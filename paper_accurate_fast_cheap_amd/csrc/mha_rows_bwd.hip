// The training half of include/pafc_attention.h: the backward of pafc_mha_rows, and the label-smoothing loss per row
// straight from the logits with its gradient.
//
// pafc_mha_rows_bwd.  Two launches, each one block per (group, head) of eight waves, no atomics: every row of dq, dk and dv
// has one owner, so two runs give the same bits.  With P = exp(S / 8 - lse), delta_i = sum_d dO_id O_id and
// dS = P o (dO V^T - delta):
//   dQ pass   a wave owns 16 queries and walks the keys.  As in the forward both score products are taken TRANSPOSED,
//             S^T = K Q^T and dP^T = V dO^T, so they land in the same C/D map (lane l: key 4(l>>4) + r, query l&15) and
//             dS^T is, register for register, the B operand of dQ^T = K^T dS^T -- the forward's PV step with K for V.
//             The query is a lane column: lse and delta are one scalar per lane.  delta is also written to the (rows, H)
//             workspace for the second pass.
//   dK/dV pass a wave owns 16 keys and walks the queries (under `causal` from its own tile on).  S = Q K^T and dP = dO V^T
//             (lane l: query 4(l>>4) + r, key l&15), then dV^T = dO^T P and dK^T = Q^T dS with P / dS as B operands.
// fp32: v_mfma_f32_16x16x4_f32, tiles of 16; bf16: v_mfma_f32_16x16x32_bf16, tiles of 32, P and dS rounded to bf16.
// Rows past the end of a group or of its keys are never read: the index is clamped to the last valid row and the duplicate
// is masked (P = 0) or not stored.
#include "pafc_attention.h"
#include "pafc_common.h"

#include <limits.h>
#include <math.h>

namespace pafc {

constexpr int kBwdDk = 64;
constexpr int kBwdWaves = 8;      // (four: 2.3 ms of pafc_mha_rows_bwd per training-batch step instead of 1.5)

__device__ __forceinline__ float bwd_sum_over_lane_groups(float x) {
    x += __shfl_xor(x, 16, kWave);
    return x + __shfl_xor(x, 32, kWave);
}

struct MhaBwdArgs {
    int H;
    const void *q; long ldq;
    const void *k, *v; long ldkv;
    const void *o; long ldo;
    const void *dout; long lddo;
    const float *lse;
    float *delta;
    const int32_t *q_off, *kv_off, *kv_len;
    int causal;
    void *dq; long lddq;
    void *dk, *dv; long lddkv;
};

// a lane's 4 x 4 results (dimensions 16 c + 4 lq + r of one row) times `scale`, as 16-byte (fp32) or 8-byte (bf16) stores
__device__ __forceinline__ void bwd_store(float *p, const f32x4 *o, float scale) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
        *reinterpret_cast<float4 *>(p + 16 * c) = make_float4(o[c][0] * scale, o[c][1] * scale, o[c][2] * scale, o[c][3] * scale);
}
__device__ __forceinline__ void bwd_store(bf16_t *p, const f32x4 *o, float scale) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint2 w;
        w.x = pack_bf16_rne(o[c][0] * scale, o[c][1] * scale);
        w.y = pack_bf16_rne(o[c][2] * scale, o[c][3] * scale);
        *reinterpret_cast<uint2 *>(p + 16 * c) = w;
    }
}

__device__ __forceinline__ void load16(const float *p, float *f) {
    load8<float>(p, f);
    load8<float>(p + 8, f + 8);
}

#define PAFC_ZERO4 {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}

// ---- dQ pass ----
__device__ __forceinline__ void dq_tile(const MhaBwdArgs &a, float, int h, int q0, int nq, int kv0, int nkv, int t, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const int qidx = 16 * t + lr;
    const long qrow = (long)q0 + min(qidx, nq - 1);
    float qa[16], da[16], oa[16];
    load16((const float *)a.q + qrow * a.ldq + h * kBwdDk + lq * 16, qa);
    load16((const float *)a.dout + qrow * a.lddo + h * kBwdDk + lq * 16, da);
    load16((const float *)a.o + qrow * a.ldo + h * kBwdDk + lq * 16, oa);
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) dl = fmaf(da[e], oa[e], dl);
    dl = bwd_sum_over_lane_groups(dl);
    const float lse = a.lse[qrow * a.H + h];
    if (lq == 0 && qidx < nq) a.delta[qrow * a.H + h] = dl;
    const int kend = a.causal ? min(nkv, 16 * t + 16) : nkv;
    f32x4 dq[4] = PAFC_ZERO4;
    const float *kbase = (const float *)a.k + h * kBwdDk, *vbase = (const float *)a.v + h * kBwdDk;
    for (int k0 = 0; k0 < kend; k0 += 16) {
        const long krow = (long)kv0 + min(k0 + lr, nkv - 1);
        float ka[16], va[16];
        load16(kbase + krow * a.ldkv + lq * 16, ka);
        load16(vbase + krow * a.ldkv + lq * 16, va);
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[e], qa[e], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[e], da[e], dp, 0, 0, 0);
        }
        float ds[4];
        const float *kg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + lq * 4 + r;
            const bool seen = key < nkv && (!a.causal || key <= qidx);
            const float p = seen ? expf(st[r] * 0.125f - lse) : 0.f;
            ds[r] = seen ? p * (dp[r] - dl) : 0.f;
            kg[r] = kbase + ((long)kv0 + min(key, nkv - 1)) * a.ldkv + lr;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) dq[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kg[r][16 * c], ds[r], dq[c], 0, 0, 0);
    }
    if (qidx < nq) bwd_store((float *)a.dq + qrow * a.lddq + h * kBwdDk + lq * 4, dq, 0.125f);
}

__device__ __forceinline__ void dq_tile(const MhaBwdArgs &a, bf16_t, int h, int q0, int nq, int kv0, int nkv, int t, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const int qidx = 16 * t + lr;
    const long qrow = (long)q0 + min(qidx, nq - 1);
    const bf16_t *qp = (const bf16_t *)a.q + qrow * a.ldq + h * kBwdDk + lq * 8;
    const bf16_t *dop = (const bf16_t *)a.dout + qrow * a.lddo + h * kBwdDk + lq * 8;
    const bf16_t *op = (const bf16_t *)a.o + qrow * a.ldo + h * kBwdDk + lq * 8;
    const uint4 qa0 = *reinterpret_cast<const uint4 *>(qp), qa1 = *reinterpret_cast<const uint4 *>(qp + 32);
    const uint4 da0 = *reinterpret_cast<const uint4 *>(dop), da1 = *reinterpret_cast<const uint4 *>(dop + 32);
    float dl = 0.f;
    {
        float df[16], of[16];
        Elem<bf16_t>::unpack(da0, df);
        Elem<bf16_t>::unpack(da1, df + 8);
        load8<bf16_t>(op, of);
        load8<bf16_t>(op + 32, of + 8);
#pragma unroll
        for (int e = 0; e < 16; ++e) dl = fmaf(df[e], of[e], dl);
    }
    dl = bwd_sum_over_lane_groups(dl);
    const float lse = a.lse[qrow * a.H + h];
    if (lq == 0 && qidx < nq) a.delta[qrow * a.H + h] = dl;
    const int kend = a.causal ? min(nkv, 16 * t + 16) : nkv;
    f32x4 dq[4] = PAFC_ZERO4;
    const bf16_t *kbase = (const bf16_t *)a.k + h * kBwdDk, *vbase = (const bf16_t *)a.v + h * kBwdDk;
    for (int k0 = 0; k0 < kend; k0 += 32) {
        float ds[8];
        const bf16_t *kg[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const long krow = (long)kv0 + min(k0 + 16 * half + lr, nkv - 1);
            const bf16_t *kp = kbase + krow * a.ldkv + lq * 8, *vp = vbase + krow * a.ldkv + lq * 8;
            const uint4 ka0 = *reinterpret_cast<const uint4 *>(kp), ka1 = *reinterpret_cast<const uint4 *>(kp + 32);
            const uint4 va0 = *reinterpret_cast<const uint4 *>(vp), va1 = *reinterpret_cast<const uint4 *>(vp + 32);
            f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            st = mfma_bf16_packed(ka0, qa0, st);
            st = mfma_bf16_packed(ka1, qa1, st);
            dp = mfma_bf16_packed(va0, da0, dp);
            dp = mfma_bf16_packed(va1, da1, dp);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * half + lq * 4 + r;
                const bool seen = key < nkv && (!a.causal || key <= qidx);
                const float p = seen ? expf(st[r] * 0.125f - lse) : 0.f;
                ds[4 * half + r] = seen ? p * (dp[r] - dl) : 0.f;
                kg[4 * half + r] = kbase + ((long)kv0 + min(key, nkv - 1)) * a.ldkv + lr;
            }
        }
        // element j of the operands of the third product is key k0 + 4 lq + j (j < 4) or k0 + 16 + 4 lq + j - 4: ds[]'s order
        u32x4 dsb;
#pragma unroll
        for (int j = 0; j < 4; ++j) dsb[j] = pack_bf16_rne(ds[2 * j], ds[2 * j + 1]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u32x4 kt;
#pragma unroll
            for (int j = 0; j < 4; ++j) kt[j] = (uint32_t)kg[2 * j][16 * c] | ((uint32_t)kg[2 * j + 1][16 * c] << 16);
            dq[c] = mfma_bf16_packed(kt, dsb, dq[c]);
        }
    }
    if (qidx < nq) bwd_store((bf16_t *)a.dq + qrow * a.lddq + h * kBwdDk + lq * 4, dq, 0.125f);
}

template <typename ET> __global__ __launch_bounds__(kBwdWaves * kWave) void mha_rows_bwd_dq_kernel(MhaBwdArgs a) {
    const int g = blockIdx.x, h = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = a.q_off[g], nq = a.q_off[g + 1] - q0;
    if (nq <= 0) return;
    const int kv0 = a.kv_off[g], nkv = a.kv_len[g];
    const int ntile = (nq + 15) >> 4;
    for (int t = wave; t < ntile; t += kBwdWaves) {
        if (nkv <= 0) {                                   // no keys: the output did not depend on q
            const f32x4 z[4] = PAFC_ZERO4;
            const int qidx = 16 * t + (lane & 15);
            if (qidx < nq) bwd_store((ET *)a.dq + ((long)q0 + qidx) * a.lddq + h * kBwdDk + (lane >> 4) * 4, z, 0.f);
            continue;
        }
        dq_tile(a, ET(), h, q0, nq, kv0, nkv, t, lane);
    }
}

// ---- dK / dV pass ----
__device__ __forceinline__ void dkv_tile(const MhaBwdArgs &a, float, int h, int q0, int nq, int kv0, int nkv, int kt, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const int kidx = 16 * kt + lr;
    const long krow = (long)kv0 + min(kidx, nkv - 1);
    float ka[16], va[16];
    load16((const float *)a.k + krow * a.ldkv + h * kBwdDk + lq * 16, ka);
    load16((const float *)a.v + krow * a.ldkv + h * kBwdDk + lq * 16, va);
    f32x4 dk[4] = PAFC_ZERO4, dv[4] = PAFC_ZERO4;
    const float *qbase = (const float *)a.q + h * kBwdDk, *dobase = (const float *)a.dout + h * kBwdDk;
    for (int i0 = a.causal ? 16 * kt : 0; i0 < nq; i0 += 16) {
        const long qrow = (long)q0 + min(i0 + lr, nq - 1);
        float qa[16], da[16];
        load16(qbase + qrow * a.ldq + lq * 16, qa);
        load16(dobase + qrow * a.lddo + lq * 16, da);
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            st = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], ka[e], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x4f32(da[e], va[e], dp, 0, 0, 0);
        }
        float p[4], ds[4];
        const float *qg[4], *dg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = i0 + lq * 4 + r;
            const bool seen = qi < nq && kidx < nkv && (!a.causal || kidx <= qi);
            const long qr = (long)q0 + min(qi, nq - 1);
            const float lse = a.lse[qr * a.H + h], dl = a.delta[qr * a.H + h];
            p[r] = seen ? expf(st[r] * 0.125f - lse) : 0.f;
            ds[r] = seen ? p[r] * (dp[r] - dl) : 0.f;
            qg[r] = qbase + qr * a.ldq + lr;
            dg[r] = dobase + qr * a.lddo + lr;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dv[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dg[r][16 * c], p[r], dv[c], 0, 0, 0);
                dk[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(qg[r][16 * c], ds[r], dk[c], 0, 0, 0);
            }
    }
    if (kidx < nkv) {
        bwd_store((float *)a.dk + krow * a.lddkv + h * kBwdDk + lq * 4, dk, 0.125f);
        bwd_store((float *)a.dv + krow * a.lddkv + h * kBwdDk + lq * 4, dv, 1.f);
    }
}

__device__ __forceinline__ void dkv_tile(const MhaBwdArgs &a, bf16_t, int h, int q0, int nq, int kv0, int nkv, int kt, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const int kidx = 16 * kt + lr;
    const long krow = (long)kv0 + min(kidx, nkv - 1);
    const bf16_t *kp = (const bf16_t *)a.k + krow * a.ldkv + h * kBwdDk + lq * 8;
    const bf16_t *vp = (const bf16_t *)a.v + krow * a.ldkv + h * kBwdDk + lq * 8;
    const uint4 ka0 = *reinterpret_cast<const uint4 *>(kp), ka1 = *reinterpret_cast<const uint4 *>(kp + 32);
    const uint4 va0 = *reinterpret_cast<const uint4 *>(vp), va1 = *reinterpret_cast<const uint4 *>(vp + 32);
    f32x4 dk[4] = PAFC_ZERO4, dv[4] = PAFC_ZERO4;
    const bf16_t *qbase = (const bf16_t *)a.q + h * kBwdDk, *dobase = (const bf16_t *)a.dout + h * kBwdDk;
    for (int i0 = a.causal ? 16 * kt : 0; i0 < nq; i0 += 32) {
        float p[8], ds[8];
        const bf16_t *qg[8], *dg[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const long qrow = (long)q0 + min(i0 + 16 * half + lr, nq - 1);
            const bf16_t *qp = qbase + qrow * a.ldq + lq * 8, *dop = dobase + qrow * a.lddo + lq * 8;
            const uint4 qa0 = *reinterpret_cast<const uint4 *>(qp), qa1 = *reinterpret_cast<const uint4 *>(qp + 32);
            const uint4 da0 = *reinterpret_cast<const uint4 *>(dop), da1 = *reinterpret_cast<const uint4 *>(dop + 32);
            f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            st = mfma_bf16_packed(qa0, ka0, st);
            st = mfma_bf16_packed(qa1, ka1, st);
            dp = mfma_bf16_packed(da0, va0, dp);
            dp = mfma_bf16_packed(da1, va1, dp);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = i0 + 16 * half + lq * 4 + r;
                const bool seen = qi < nq && kidx < nkv && (!a.causal || kidx <= qi);
                const long qr = (long)q0 + min(qi, nq - 1);
                const float lse = a.lse[qr * a.H + h], dl = a.delta[qr * a.H + h];
                const float pr = seen ? expf(st[r] * 0.125f - lse) : 0.f;
                p[4 * half + r] = pr;
                ds[4 * half + r] = seen ? pr * (dp[r] - dl) : 0.f;
                qg[4 * half + r] = qbase + qr * a.ldq + lr;
                dg[4 * half + r] = dobase + qr * a.lddo + lr;
            }
        }
        // element j of the operands below is query i0 + 4 lq + j (j < 4) or i0 + 16 + 4 lq + j - 4: the order of p[] and ds[]
        u32x4 pb, dsb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pb[j] = pack_bf16_rne(p[2 * j], p[2 * j + 1]);
            dsb[j] = pack_bf16_rne(ds[2 * j], ds[2 * j + 1]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u32x4 dt, qt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dt[j] = (uint32_t)dg[2 * j][16 * c] | ((uint32_t)dg[2 * j + 1][16 * c] << 16);
                qt[j] = (uint32_t)qg[2 * j][16 * c] | ((uint32_t)qg[2 * j + 1][16 * c] << 16);
            }
            dv[c] = mfma_bf16_packed(dt, pb, dv[c]);
            dk[c] = mfma_bf16_packed(qt, dsb, dk[c]);
        }
    }
    if (kidx < nkv) {
        bwd_store((bf16_t *)a.dk + krow * a.lddkv + h * kBwdDk + lq * 4, dk, 0.125f);
        bwd_store((bf16_t *)a.dv + krow * a.lddkv + h * kBwdDk + lq * 4, dv, 1.f);
    }
}

template <typename ET> __global__ __launch_bounds__(kBwdWaves * kWave) void mha_rows_bwd_dkv_kernel(MhaBwdArgs a) {
    const int g = blockIdx.x, h = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = a.q_off[g], nq = a.q_off[g + 1] - q0;
    const int kv0 = a.kv_off[g], nkv = a.kv_len[g];
    if (nq <= 0 || nkv <= 0) return;                      // a group without query rows owns no key rows
    const int ntile = (nkv + 15) >> 4;
    for (int kt = wave; kt < ntile; kt += kBwdWaves) dkv_tile(a, ET(), h, q0, nq, kv0, nkv, kt, lane);
}

// ---- label-smoothing loss per row ----
// One block per row, one pass over the logits: every thread keeps (max, sum of exp), the plain sum and the argmax of its
// strided share, the block merges them, thread 0 forms the loss.
__device__ __forceinline__ void lsm_lse_merge(float &m, float &s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    const float a = (m == -INFINITY) ? 0.f : s * expf(m - M);
    const float b = (m2 == -INFINITY) ? 0.f : s2 * expf(m2 - M);
    m = M;
    s = a + b;
}
__device__ __forceinline__ void lsm_argmax_merge(float &b, int &bi, float b2, int bi2) {
    if (b2 > b || (b2 == b && bi2 < bi)) {
        b = b2;
        bi = bi2;
    }
}

template <typename ET>
__global__ __launch_bounds__(256) void lsm_loss_kernel(int V, const ET *x, long ldl, const int32_t *target, float smoothing,
                                                       float *loss, float *lse_out, int32_t *correct) {
    const long r = blockIdx.x;
    const ET *row = x + r * ldl;
    float m = -INFINITY, s = 0.f, sum = 0.f, best = -INFINITY;
    int bi = INT_MAX;
    for (int v = threadIdx.x; v < V; v += 256) {
        const float a = Elem<ET>::load(row + v);
        sum += a;
        if (a > best) {                                    // strict: the lowest index of a thread's share wins a tie
            best = a;
            bi = v;
        }
        if (a > m) {
            s = s * expf(m - a) + 1.f;
            m = a;
        } else if (a > -INFINITY) {
            s += expf(a - m);
        } else if (a != a) {
            m = s = a;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lsm_lse_merge(m, s, __shfl_xor(m, off, kWave), __shfl_xor(s, off, kWave));
        sum += __shfl_xor(sum, off, kWave);
        lsm_argmax_merge(best, bi, __shfl_xor(best, off, kWave), __shfl_xor(bi, off, kWave));
    }
    __shared__ float sm[4], ss[4], su[4], sb[4];
    __shared__ int si[4];
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        sm[w] = m;
        ss[w] = s;
        su[w] = sum;
        sb[w] = best;
        si[w] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lsm_lse_merge(m, s, sm[w], ss[w]);
            sum += su[w];
            lsm_argmax_merge(best, bi, sb[w], si[w]);
        }
        const float lse = m + logf(s);
        lse_out[r] = lse;
        const int t = target[r];
        if (t == -1) {                                     // the ignore id
            loss[r] = 0.f;
            correct[r] = 0;
        } else if (t < 0 || t >= V) {
            loss[r] = NAN;
            correct[r] = 0;
        } else {
            // the KL sum  conf (log conf - logp_y) + sum_{v != y} sv (log sv - logp_v)  without the log-softmax; the few
            // scalar steps in double, so that V * lse cancels against the sum of the logits without a float32 rounding
            const double conf = 1.0 - (double)smoothing, sv = (double)smoothing / (V - 1);
            const double C = (conf > 0.0 ? conf * log(conf) : 0.0) + (sv > 0.0 ? (V - 1) * sv * log(sv) : 0.0);
            const double logp = (double)Elem<ET>::load(row + t) - (double)lse;
            loss[r] = (float)(C - conf * logp - sv * ((double)sum - (double)V * (double)lse - logp));
            correct[r] = bi == t;
        }
    }
}

template <typename ET>
__global__ __launch_bounds__(256) void lsm_loss_bwd_kernel(int V, const ET *x, long ldl, const int32_t *target, float smoothing,
                                                           const float *lse, const float *gp, ET *dx, long ldd) {
    const long r = blockIdx.x;
    const ET *row = x + r * ldl;
    ET *drow = dx + r * ldd;
    const int t = target[r];
    const float g = *gp, l = lse[r];
    const float conf = 1.f - smoothing, sv = smoothing / (float)(V - 1);
    const bool ignored = t == -1, bad = !ignored && (t < 0 || t >= V);
    for (int v = threadIdx.x; v < ldd; v += 256) {         // the columns [V, ldd) are the zero padding of the dX GEMM's K
        float o = 0.f;
        if (v < V && !ignored) o = bad ? NAN : g * (expf(Elem<ET>::load(row + v) - l) - (v == t ? conf : sv));
        Elem<ET>::store(drow + v, o);
    }
}

}  // namespace pafc

extern "C" int pafc_mha_rows_bwd(int dtype, int G, int H, int dk, long rows, const void *q, long ldq, const void *k, const void *v,
                                 long ldkv, const void *out, long ldo, const void *dout, long lddo, const float *lse,
                                 const int32_t *q_off, const int32_t *kv_off, const int32_t *kv_len, int causal, void *dq,
                                 long lddq, void *dk_out, void *dv_out, long lddkv, void *workspace, size_t workspace_bytes,
                                 pafc_stream_t stream) {
    if (!q || !k || !v || !out || !dout || !lse || !q_off || !kv_off || !kv_len || !dq || !dk_out || !dv_out || !workspace)
        return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (G <= 0 || H <= 0 || dk <= 0 || H > 65535 || rows <= 0) return PAFC_ERR_BAD_DIMS;
    if (dk != pafc::kBwdDk) return PAFC_ERR_UNSUPPORTED;
    const long width = (long)H * dk, per16 = dtype == PAFC_F32 ? 4 : 8;
    const long lds[6] = {ldq, ldkv, ldo, lddo, lddq, lddkv};
    for (long ld : lds)
        if (ld < width || ld % per16) return PAFC_ERR_BAD_DIMS;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk_out |
         (uintptr_t)dv_out) & 15)
        return PAFC_ERR_ALIGNMENT;
    if (((uintptr_t)workspace | (uintptr_t)lse) & 3) return PAFC_ERR_ALIGNMENT;
    if (workspace_bytes < pafc_mha_rows_bwd_workspace_bytes(rows, H)) return PAFC_ERR_WORKSPACE;
    pafc::MhaBwdArgs a{H, q, ldq, k, v, ldkv, out, ldo, dout, lddo, lse, (float *)workspace, q_off, kv_off, kv_len, causal != 0,
                       dq, lddq, dk_out, dv_out, lddkv};
    const dim3 grid((unsigned)G, (unsigned)H), block(pafc::kBwdWaves * pafc::kWave);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32) {
        hipLaunchKernelGGL((pafc::mha_rows_bwd_dq_kernel<float>), grid, block, 0, s, a);
        hipLaunchKernelGGL((pafc::mha_rows_bwd_dkv_kernel<float>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((pafc::mha_rows_bwd_dq_kernel<pafc::bf16_t>), grid, block, 0, s, a);
        hipLaunchKernelGGL((pafc::mha_rows_bwd_dkv_kernel<pafc::bf16_t>), grid, block, 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" size_t pafc_mha_rows_bwd_workspace_bytes(long rows, int H) {
    return rows > 0 && H > 0 ? (size_t)rows * (size_t)H * sizeof(float) : 0;
}

extern "C" int pafc_lsm_loss_rows(int dtype, long rows, int V, const void *logits, long ldl, const int32_t *target,
                                  float smoothing, float *loss, float *lse, int32_t *correct, pafc_stream_t stream) {
    if (!logits || !target || !loss || !lse || !correct) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (rows <= 0 || V < 2 || ldl < V || rows > 0x7fffffffL || !(smoothing >= 0.f && smoothing <= 1.f)) return PAFC_ERR_BAD_DIMS;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::lsm_loss_kernel<float>), dim3((unsigned)rows), dim3(256), 0, s, V, (const float *)logits, ldl,
                           target, smoothing, loss, lse, correct);
    else
        hipLaunchKernelGGL((pafc::lsm_loss_kernel<pafc::bf16_t>), dim3((unsigned)rows), dim3(256), 0, s, V,
                           (const pafc::bf16_t *)logits, ldl, target, smoothing, loss, lse, correct);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_lsm_loss_rows_bwd(int dtype, long rows, int V, const void *logits, long ldl, const int32_t *target,
                                      float smoothing, const float *lse, const float *g, void *dlogits, long ldd,
                                      pafc_stream_t stream) {
    if (!logits || !target || !lse || !g || !dlogits) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (rows <= 0 || V < 2 || ldl < V || ldd < V || ldd > 0x7fffffffL || rows > 0x7fffffffL ||
        !(smoothing >= 0.f && smoothing <= 1.f))
        return PAFC_ERR_BAD_DIMS;
    if (dlogits == logits && ldd != ldl) return PAFC_ERR_BAD_DIMS;       // in place: the same rows
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::lsm_loss_bwd_kernel<float>), dim3((unsigned)rows), dim3(256), 0, s, V, (const float *)logits, ldl,
                           target, smoothing, lse, g, (float *)dlogits, ldd);
    else
        hipLaunchKernelGGL((pafc::lsm_loss_bwd_kernel<pafc::bf16_t>), dim3((unsigned)rows), dim3(256), 0, s, V,
                           (const pafc::bf16_t *)logits, ldl, target, smoothing, lse, g, (pafc::bf16_t *)dlogits, ldd);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
