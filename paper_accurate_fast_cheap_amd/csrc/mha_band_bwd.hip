// pafc_mha_band_bwd (include/pafc_attention.h): the backward of pafc_mha_band, the limited-context attention with the
// positional term of the Conformer baseline.
//
// Per batch row and head, with qu_i = q_i + u_h, qv_i = q_i + vb_h (bf16: each rounded to bf16 once, as the forward rounds
// them; the backward treats that rounding as the identity), P_ij = exp(s_ij - lse_i) over the real keys of the band,
// delta_i = sum_d dO_id O_id and dS = P o (dO V^T - delta):
//   dqu = dS K / 8, dqv = dS Pos / 8, dq = dqu + dqv;  dk = dS^T QU / 8;  dv = P^T dO;
//   dp = sum_b dS^T QV / 8;  du = sum_{b,i} dqu_i;  dvb = sum_{b,i} dqv_i.
// The padding keys [T, t_pad) have a constant score and a zero value: they are in lse (so P sums to less than one) and
// nowhere else.
//
// Three launches, no atomics -- every number has one owner and every sum a fixed order, so two runs give the same bits:
//   dQ pass      grid (query tile of 64, head, batch row), four waves; a wave owns the 16 queries [a, a + 15] and walks the
//                keys [max(0, a - w), min(T - 1, a + 15 + w)] as the forward does.  Both score products are taken TRANSPOSED,
//                S^T = [K | Pos] [QU | QV]^T and dP^T = V dO^T, so they land in one C/D map (lane l: key 4(l>>4) + r, query
//                l&15) and dS^T is, register for register, the B operand of dQU^T = K^T dS^T and dQV^T = Pos^T dS^T.  The
//                query is a lane column: lse and delta are one scalar per lane.  dS = P (dP - delta) is a difference of two
//                64-term dot products of size ~|dout||v|: delta is summed and kept in float64 (16 fma per lane, once per
//                wave) and dP runs as four short accumulator chains.  delta goes to the workspace for the second
//                pass; the wave's column sums of dqu and dqv (16 queries) go to the workspace as one fp32 partial each.
//   dK/dV/dP pass grid (key tile of 64, head, batch row); a wave owns the 16 keys [j, j + 15] and walks the queries
//                [max(0, j - w), min(T - 1, j + 15 + w)]: S = [QU | QV] [K | Pos]^T and dP = dO V^T (lane l: query
//                4(l>>4) + r, key l&15), then dV^T = dO^T P, dK^T = QU^T dS and dPos^T = QV^T dS with P / dS as B operands.
//                dPos of this batch row goes to the workspace in fp32.
//   reduce       dp[j] = sum over the batch rows' partials in the order b = 0, 1, ...; du / dvb = the (tile, batch row)
//                partials in four interleaved chains of fixed order, then those four in order.
// Band edges as in the forward: a tile all of whose (query, key) pairs lie inside the band and inside [0, T) skips the
// per-element test (a wave-uniform choice between two instantiations).
// fp32: v_mfma_f32_16x16x4_f32, tiles of 16; bf16: v_mfma_f32_16x16x32_bf16, tiles of 32, P and dS rounded to bf16.
// Nothing past row T - 1 of any operand is read: the row index is clamped to the last valid one and the duplicate is
// masked (P = dS = 0) or not stored.  Row offsets are 64-bit.
#include "pafc_attention.h"
#include "mha_tile_body.h"

namespace pafc {

constexpr int kBbWaves = 4;

struct BandBwdArgs {
    int B, T, H, w, nqt;       // nqt: query tiles of 16 per batch row
    const void *q; long ldq;
    const void *k, *v; long ldkv;
    const void *p; long ldp;
    const void *u, *vb;
    const void *o; long ldo;
    const void *dout; long lddo;
    const float *lse;
    void *dq; long lddq;
    void *dk, *dv; long lddkv;
    void *dp; long lddp;
    float *du, *dvb;
    float *dp_part;            // (B, T, H * 64): dPos of each batch row
    float *col_part;           // (B * nqt, H, 2, 64): column sums of dqu | dqv of each query tile of 16
    double *delta;             // (B * T, H), float64: dS = P (dP - delta) cancels, so delta keeps every bit it has
};

#define PAFC_BB_ZERO4 {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}

__device__ __forceinline__ void bb_load16(const float *p, float *f) {
    load8<float>(p, f);
    load8<float>(p + 8, f + 8);
}

// the wave's column sums of dqu and dqv over its valid queries -> the tile's fp32 partial (scaled by 1 / 8)
__device__ __forceinline__ void bb_store_colsums(const BandBwdArgs &A, int b, int h, int qt, bool valid, int lr, int lq,
                                                 const f32x4 *dqu, const f32x4 *dqv) {
    float *dst = A.col_part + (((long)b * A.nqt + qt) * A.H + h) * 128 + lq * 4;
#pragma unroll
    for (int which = 0; which < 2; ++which)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float s[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = valid ? (which ? dqv[c][r] : dqu[c][r]) : 0.f;
                x += __shfl_xor(x, 1, kWave);
                x += __shfl_xor(x, 2, kWave);
                x += __shfl_xor(x, 4, kWave);
                x += __shfl_xor(x, 8, kWave);
                s[r] = x * 0.125f;
            }
            if (lr == 0) *reinterpret_cast<float4 *>(dst + which * 64 + 16 * c) = make_float4(s[0], s[1], s[2], s[3]);
        }
}

// ---- dQ pass, fp32: one key tile of 16 from key k0 ----
template <bool EDGE>
__device__ __forceinline__ void bb_dq_tile(const BandBwdArgs &A, const float *kbase, const float *pbase, const float *vbase,
                                           const float *qa, const float *qb, const float *da, float lse, double dl, int k0, int i,
                                           int lr, int lq, f32x4 *dqu, f32x4 *dqv) {
    const long krow = min(k0 + lr, A.T - 1);
    float ka[16], pa[16], va[16];
    bb_load16(kbase + krow * A.ldkv + lq * 16, ka);
    bb_load16(pbase + krow * A.ldp + lq * 16, pa);
    bb_load16(vbase + krow * A.ldkv + lq * 16, va);
    f32x4 sk = {0.f, 0.f, 0.f, 0.f}, sp = {0.f, 0.f, 0.f, 0.f}, dp4[4] = PAFC_BB_ZERO4;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        sk = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[e], qa[e], sk, 0, 0, 0);
        sp = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[e], qb[e], sp, 0, 0, 0);
        dp4[e & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[e], da[e], dp4[e & 3], 0, 0, 0);     // four short chains
    }
    const f32x4 dpv = (dp4[0] + dp4[1]) + (dp4[2] + dp4[3]);
    float ds[4];
    const float *kg[4], *pg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int key = k0 + lq * 4 + r;
        const bool seen = !EDGE || band_sees(key, i, A.w, A.T);
        const float pr = seen ? expf((sk[r] + sp[r]) * 0.125f - lse) : 0.f;       // the forward's score, term for term
        ds[r] = seen ? pr * (float)((double)dpv[r] - dl) : 0.f;
        const long kr = min(key, A.T - 1);
        kg[r] = kbase + kr * A.ldkv + lr;
        pg[r] = pbase + kr * A.ldp + lr;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dqu[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kg[r][16 * c], ds[r], dqu[c], 0, 0, 0);
            dqv[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(pg[r][16 * c], ds[r], dqv[c], 0, 0, 0);
        }
}

// ---- dQ pass, bf16: one key tile of 32 from key k0 ----
template <bool EDGE>
__device__ __forceinline__ void bb_dq_tile(const BandBwdArgs &A, const bf16_t *kbase, const bf16_t *pbase, const bf16_t *vbase,
                                           const uint4 *qa, const uint4 *qb, const uint4 *da, float lse, double dl, int k0, int i,
                                           int lr, int lq, f32x4 *dqu, f32x4 *dqv) {
    float ds[8];
    const bf16_t *kg[8], *pg[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long krow = min(k0 + 16 * half + lr, A.T - 1);
        const bf16_t *kp = kbase + krow * A.ldkv + lq * 8, *pp = pbase + krow * A.ldp + lq * 8;
        const bf16_t *vp = vbase + krow * A.ldkv + lq * 8;
        const uint4 ka0 = *reinterpret_cast<const uint4 *>(kp), ka1 = *reinterpret_cast<const uint4 *>(kp + 32);
        const uint4 pa0 = *reinterpret_cast<const uint4 *>(pp), pa1 = *reinterpret_cast<const uint4 *>(pp + 32);
        const uint4 va0 = *reinterpret_cast<const uint4 *>(vp), va1 = *reinterpret_cast<const uint4 *>(vp + 32);
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpv = {0.f, 0.f, 0.f, 0.f};
        st = mfma_bf16_packed(ka0, qa[0], st);
        st = mfma_bf16_packed(ka1, qa[1], st);
        st = mfma_bf16_packed(pa0, qb[0], st);
        st = mfma_bf16_packed(pa1, qb[1], st);
        dpv = mfma_bf16_packed(va0, da[0], dpv);
        dpv = mfma_bf16_packed(va1, da[1], dpv);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 16 * half + lq * 4 + r;
            const bool seen = !EDGE || band_sees(key, i, A.w, A.T);
            const float pr = seen ? expf(st[r] * 0.125f - lse) : 0.f;
            ds[4 * half + r] = seen ? pr * (float)((double)dpv[r] - dl) : 0.f;
            const long kr = min(key, A.T - 1);
            kg[4 * half + r] = kbase + kr * A.ldkv + lr;
            pg[4 * half + r] = pbase + kr * A.ldp + lr;
        }
    }
    // element j of the operands of the third products is key k0 + 4 lq + j (j < 4) or k0 + 16 + 4 lq + j - 4: ds[]'s order
    u32x4 dsb;
#pragma unroll
    for (int j = 0; j < 4; ++j) dsb[j] = pack_bf16_rne(ds[2 * j], ds[2 * j + 1]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        u32x4 kt, pt;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kt[j] = (uint32_t)kg[2 * j][16 * c] | ((uint32_t)kg[2 * j + 1][16 * c] << 16);
            pt[j] = (uint32_t)pg[2 * j][16 * c] | ((uint32_t)pg[2 * j + 1][16 * c] << 16);
        }
        dqu[c] = mfma_bf16_packed(kt, dsb, dqu[c]);
        dqv[c] = mfma_bf16_packed(pt, dsb, dqv[c]);
    }
}

// the lane's dout fragment in the layout the products read, and delta = dout . out of its row
__device__ __forceinline__ double bb_sum_over_lane_groups(double x) {
    x += __shfl_xor(x, 16, kWave);
    return x + __shfl_xor(x, 32, kWave);
}
__device__ __forceinline__ double bb_dout_delta(const float *dop, const float *op, float *da) {
    float oa[16];
    bb_load16(dop, da);
    bb_load16(op, oa);
    double dl = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) dl = fma((double)da[e], (double)oa[e], dl);
    return bb_sum_over_lane_groups(dl);
}
__device__ __forceinline__ double bb_dout_delta(const bf16_t *dop, const bf16_t *op, uint4 *da) {
    da[0] = *reinterpret_cast<const uint4 *>(dop);
    da[1] = *reinterpret_cast<const uint4 *>(dop + 32);
    float df[16], of[16];
    Elem<bf16_t>::unpack(da[0], df);
    Elem<bf16_t>::unpack(da[1], df + 8);
    load8<bf16_t>(op, of);
    load8<bf16_t>(op + 32, of + 8);
    double dl = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) dl = fma((double)df[e], (double)of[e], dl);
    return bb_sum_over_lane_groups(dl);
}

template <typename ET> struct BbFrag;
template <> struct BbFrag<float> { typedef float type; static constexpr int kN = 16, kTile = 16, kLane = 16; };
template <> struct BbFrag<bf16_t> { typedef uint4 type; static constexpr int kN = 2, kTile = 32, kLane = 8; };

template <typename ET> __global__ __launch_bounds__(kBbWaves * kWave) void mha_band_bwd_dq_kernel(BandBwdArgs A) {
    typedef BbFrag<ET> F;
    const int h = blockIdx.y, b = blockIdx.z;
    const long row0 = (long)b * A.T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = 64 * blockIdx.x + 16 * wave;
    if (a >= A.T) return;
    const int lr = lane & 15, lq = lane >> 4;
    const int T = A.T, w = A.w;
    const int i = min(a + lr, T - 1);                      // the lane's query; a duplicate of the last one is not stored
    const bool valid = a + lr < T;
    typename F::type qa[F::kN], qb[F::kN], da[F::kN];
    band_query((const ET *)A.q + (row0 + i) * A.ldq + h * kDk + lq * F::kLane, (const ET *)A.u + h * kDk + lq * F::kLane,
               (const ET *)A.vb + h * kDk + lq * F::kLane, qa, qb);
    const double dl = bb_dout_delta((const ET *)A.dout + (row0 + i) * A.lddo + h * kDk + lq * F::kLane,
                                   (const ET *)A.o + (row0 + i) * A.ldo + h * kDk + lq * F::kLane, da);
    const float lse = A.lse[(row0 + i) * A.H + h];
    if (lq == 0 && valid) A.delta[(row0 + i) * A.H + h] = dl;
    const ET *kbase = (const ET *)A.k + row0 * A.ldkv + h * kDk, *vbase = (const ET *)A.v + row0 * A.ldkv + h * kDk;
    const ET *pbase = (const ET *)A.p + h * kDk;
    const int last = min(a + 15, T - 1);
    const int klo = max(0, a - w), khi = min(T - 1, last + w);
    const int in_lo = last - w, in_hi = min(a + w, T - 1);  // every key of [in_lo, in_hi] is seen by all 16 queries
    f32x4 dqu[4] = PAFC_BB_ZERO4, dqv[4] = PAFC_BB_ZERO4;
    for (int k0 = klo; k0 <= khi; k0 += F::kTile) {
        if (k0 >= in_lo && k0 + F::kTile - 1 <= in_hi)
            bb_dq_tile<false>(A, kbase, pbase, vbase, qa, qb, da, lse, dl, k0, i, lr, lq, dqu, dqv);
        else
            bb_dq_tile<true>(A, kbase, pbase, vbase, qa, qb, da, lse, dl, k0, i, lr, lq, dqu, dqv);
    }
    f32x4 dq[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) dq[c] = dqu[c] + dqv[c];
    store_tile<ET>(A.dq, A.lddq, h, row0 + a + lr, valid, lq, dq, 0.125f);
    bb_store_colsums(A, b, h, a >> 4, valid, lr, lq, dqu, dqv);
}

// ---- dK / dV / dPos pass ----
// fp32: one query tile of 16 from query i0; the lane's key is kidx, its fragments ka / pa / va
template <bool EDGE>
__device__ __forceinline__ void bb_dkv_tile(const BandBwdArgs &A, const float *qbase, const float *dobase, long row0, int h,
                                            const float *ka, const float *pa, const float *va, const float *uu, const float *vv,
                                            const float *uc, const float *vc, int i0, int kidx, int lr, int lq, f32x4 *dk,
                                            f32x4 *dv, f32x4 *dpp) {
    const long qrow = row0 + min(i0 + lr, A.T - 1);
    float qa[16], qb[16], da[16];
    bb_load16(qbase + qrow * A.ldq + lq * 16, qa);
    bb_load16(dobase + qrow * A.lddo + lq * 16, da);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        qb[e] = qa[e] + vv[e];
        qa[e] = qa[e] + uu[e];
    }
    f32x4 sk = {0.f, 0.f, 0.f, 0.f}, sp = {0.f, 0.f, 0.f, 0.f}, dp4[4] = PAFC_BB_ZERO4;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        sk = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], ka[e], sk, 0, 0, 0);
        sp = __builtin_amdgcn_mfma_f32_16x16x4f32(qb[e], pa[e], sp, 0, 0, 0);
        dp4[e & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[e], va[e], dp4[e & 3], 0, 0, 0);     // four short chains
    }
    const f32x4 dpv = (dp4[0] + dp4[1]) + (dp4[2] + dp4[3]);
    float pr[4], ds[4];
    const float *qg[4], *dg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + lq * 4 + r;
        const bool seen = !EDGE || (qi < A.T && band_sees(kidx, qi, A.w, A.T));
        const long qr = row0 + min(qi, A.T - 1);
        const float lse = A.lse[qr * A.H + h];
        const double dl = A.delta[qr * A.H + h];
        pr[r] = seen ? expf((sk[r] + sp[r]) * 0.125f - lse) : 0.f;
        ds[r] = seen ? pr[r] * (float)((double)dpv[r] - dl) : 0.f;
        qg[r] = qbase + qr * A.ldq + lr;
        dg[r] = dobase + qr * A.lddo + lr;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float qx = qg[r][16 * c];
            dv[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dg[r][16 * c], pr[r], dv[c], 0, 0, 0);
            dk[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(qx + uc[c], ds[r], dk[c], 0, 0, 0);
            dpp[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(qx + vc[c], ds[r], dpp[c], 0, 0, 0);
        }
}

// bf16: one query tile of 32 from query i0
template <bool EDGE>
__device__ __forceinline__ void bb_dkv_tile(const BandBwdArgs &A, const bf16_t *qbase, const bf16_t *dobase, long row0, int h,
                                            const uint4 *ka, const uint4 *pa, const uint4 *va, const bf16_t *up,
                                            const bf16_t *vbp, const float *uc, const float *vc, int i0, int kidx, int lr, int lq,
                                            f32x4 *dk, f32x4 *dv, f32x4 *dpp) {
    float pr[8], ds[8];
    const bf16_t *qg[8], *dg[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long qrow = row0 + min(i0 + 16 * half + lr, A.T - 1);
        uint4 qa[2], qb[2];
        band_query(qbase + qrow * A.ldq + lq * 8, up, vbp, qa, qb);
        const bf16_t *dop = dobase + qrow * A.lddo + lq * 8;
        const uint4 da0 = *reinterpret_cast<const uint4 *>(dop), da1 = *reinterpret_cast<const uint4 *>(dop + 32);
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpv = {0.f, 0.f, 0.f, 0.f};
        st = mfma_bf16_packed(qa[0], ka[0], st);
        st = mfma_bf16_packed(qa[1], ka[1], st);
        st = mfma_bf16_packed(qb[0], pa[0], st);
        st = mfma_bf16_packed(qb[1], pa[1], st);
        dpv = mfma_bf16_packed(da0, va[0], dpv);
        dpv = mfma_bf16_packed(da1, va[1], dpv);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = i0 + 16 * half + lq * 4 + r;
            const bool seen = !EDGE || (qi < A.T && band_sees(kidx, qi, A.w, A.T));
            const long qr = row0 + min(qi, A.T - 1);
            const float lse = A.lse[qr * A.H + h];
            const double dl = A.delta[qr * A.H + h];
            const float x = seen ? expf(st[r] * 0.125f - lse) : 0.f;
            pr[4 * half + r] = x;
            ds[4 * half + r] = seen ? x * (float)((double)dpv[r] - dl) : 0.f;
            qg[4 * half + r] = qbase + qr * A.ldq + lr;
            dg[4 * half + r] = dobase + qr * A.lddo + lr;
        }
    }
    // element j of the operands below is query i0 + 4 lq + j (j < 4) or i0 + 16 + 4 lq + j - 4: the order of pr[] and ds[]
    u32x4 pb, dsb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pb[j] = pack_bf16_rne(pr[2 * j], pr[2 * j + 1]);
        dsb[j] = pack_bf16_rne(ds[2 * j], ds[2 * j + 1]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        u32x4 dt, qut, qvt;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dt[j] = (uint32_t)dg[2 * j][16 * c] | ((uint32_t)dg[2 * j + 1][16 * c] << 16);
            const float q0 = bf16_bits_to_f32(qg[2 * j][16 * c]), q1 = bf16_bits_to_f32(qg[2 * j + 1][16 * c]);
            qut[j] = pack_bf16_rne(q0 + uc[c], q1 + uc[c]);          // the forward's rounded q + u, q + v
            qvt[j] = pack_bf16_rne(q0 + vc[c], q1 + vc[c]);
        }
        dv[c] = mfma_bf16_packed(dt, pb, dv[c]);
        dk[c] = mfma_bf16_packed(qut, dsb, dk[c]);
        dpp[c] = mfma_bf16_packed(qvt, dsb, dpp[c]);
    }
}

// the lane's key fragments and bias operands, fp32 / bf16
struct BbKeyF32 {
    float ka[16], pa[16], va[16], uu[16], vv[16];
    __device__ __forceinline__ void load(const float *kp, const float *pp, const float *vp, const float *up, const float *vbp) {
        bb_load16(kp, ka);
        bb_load16(pp, pa);
        bb_load16(vp, va);
        bb_load16(up, uu);
        bb_load16(vbp, vv);
    }
};
struct BbKeyBf16 {
    uint4 ka[2], pa[2], va[2];
    const bf16_t *up, *vbp;
    __device__ __forceinline__ void load(const bf16_t *kp, const bf16_t *pp, const bf16_t *vp, const bf16_t *up_, const bf16_t *vbp_) {
        ka[0] = *reinterpret_cast<const uint4 *>(kp);
        ka[1] = *reinterpret_cast<const uint4 *>(kp + 32);
        pa[0] = *reinterpret_cast<const uint4 *>(pp);
        pa[1] = *reinterpret_cast<const uint4 *>(pp + 32);
        va[0] = *reinterpret_cast<const uint4 *>(vp);
        va[1] = *reinterpret_cast<const uint4 *>(vp + 32);
        up = up_;
        vbp = vbp_;
    }
};
template <bool EDGE>
__device__ __forceinline__ void bb_dkv_step(const BandBwdArgs &A, const float *qbase, const float *dobase, long row0, int h,
                                            const BbKeyF32 &K, const float *uc, const float *vc, int i0, int kidx, int lr, int lq,
                                            f32x4 *dk, f32x4 *dv, f32x4 *dpp) {
    bb_dkv_tile<EDGE>(A, qbase, dobase, row0, h, K.ka, K.pa, K.va, K.uu, K.vv, uc, vc, i0, kidx, lr, lq, dk, dv, dpp);
}
template <bool EDGE>
__device__ __forceinline__ void bb_dkv_step(const BandBwdArgs &A, const bf16_t *qbase, const bf16_t *dobase, long row0, int h,
                                            const BbKeyBf16 &K, const float *uc, const float *vc, int i0, int kidx, int lr, int lq,
                                            f32x4 *dk, f32x4 *dv, f32x4 *dpp) {
    bb_dkv_tile<EDGE>(A, qbase, dobase, row0, h, K.ka, K.pa, K.va, K.up, K.vbp, uc, vc, i0, kidx, lr, lq, dk, dv, dpp);
}
template <typename ET> struct BbKey;
template <> struct BbKey<float> { typedef BbKeyF32 type; };
template <> struct BbKey<bf16_t> { typedef BbKeyBf16 type; };

template <typename ET> __global__ __launch_bounds__(kBbWaves * kWave) void mha_band_bwd_dkv_kernel(BandBwdArgs A) {
    typedef BbFrag<ET> F;
    const int h = blockIdx.y, b = blockIdx.z;
    const long row0 = (long)b * A.T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ja = 64 * blockIdx.x + 16 * wave;
    if (ja >= A.T) return;
    const int lr = lane & 15, lq = lane >> 4;
    const int T = A.T, w = A.w;
    const int kidx = ja + lr, krow = min(kidx, T - 1);     // the lane's key; a duplicate of the last one is not stored
    const ET *up = (const ET *)A.u + h * kDk, *vbp = (const ET *)A.vb + h * kDk;
    typename BbKey<ET>::type K;
    K.load((const ET *)A.k + (row0 + krow) * A.ldkv + h * kDk + lq * F::kLane, (const ET *)A.p + (long)krow * A.ldp + h * kDk + lq * F::kLane,
           (const ET *)A.v + (row0 + krow) * A.ldkv + h * kDk + lq * F::kLane, up + lq * F::kLane, vbp + lq * F::kLane);
    float uc[4], vc[4];                                    // the biases at the dimensions 16 c + lr of the third products' A operand
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uc[c] = Elem<ET>::load(up + 16 * c + lr);
        vc[c] = Elem<ET>::load(vbp + 16 * c + lr);
    }
    const ET *qbase = (const ET *)A.q + h * kDk, *dobase = (const ET *)A.dout + h * kDk;
    const int jlast = min(ja + 15, T - 1);
    const int ilo = max(0, ja - w), ihi = min(T - 1, jlast + w);
    f32x4 dk[4] = PAFC_BB_ZERO4, dv[4] = PAFC_BB_ZERO4, dpp[4] = PAFC_BB_ZERO4;
    for (int i0 = ilo; i0 <= ihi; i0 += F::kTile) {
        const int iend = i0 + F::kTile - 1;
        // every query of the tile exists and sees every key of [ja, jlast]
        if (iend <= T - 1 && iend - ja <= w && jlast - i0 <= w)
            bb_dkv_step<false>(A, qbase, dobase, row0, h, K, uc, vc, i0, kidx, lr, lq, dk, dv, dpp);
        else
            bb_dkv_step<true>(A, qbase, dobase, row0, h, K, uc, vc, i0, kidx, lr, lq, dk, dv, dpp);
    }
    const bool valid = kidx < T;
    store_tile<ET>(A.dk, A.lddkv, h, row0 + kidx, valid, lq, dk, 0.125f);
    store_tile<ET>(A.dv, A.lddkv, h, row0 + kidx, valid, lq, dv, 1.f);
    store_tile<float>(A.dp_part, (long)A.H * kDk, h, row0 + kidx, valid, lq, dpp, 0.125f);
}

// ---- reduce: dp over the batch rows, du / dvb over the (tile, batch row) partials, each in a fixed order ----
__device__ __forceinline__ void bb_store4(float *p, float4 s) { *reinterpret_cast<float4 *>(p) = s; }
__device__ __forceinline__ void bb_store4(bf16_t *p, float4 s) {
    uint2 w;
    w.x = pack_bf16_rne(s.x, s.y);
    w.y = pack_bf16_rne(s.z, s.w);
    *reinterpret_cast<uint2 *>(p) = w;
}

template <typename ET> __global__ __launch_bounds__(256) void mha_band_bwd_reduce_kernel(BandBwdArgs A, unsigned dp_blocks) {
    if (blockIdx.x < dp_blocks) {
        const long per_row = (long)A.H * 16;               // groups of four floats per position row
        const long idx = (long)blockIdx.x * 256 + threadIdx.x;
        if (idx >= (long)A.T * per_row) return;
        const long row = idx / per_row, col = (idx - row * per_row) * 4;
        const long stride = (long)A.T * A.H * kDk;
        const float *src = A.dp_part + row * A.H * kDk + col;
        float4 s = *reinterpret_cast<const float4 *>(src);
        for (int b = 1; b < A.B; ++b) {
            const float4 x = *reinterpret_cast<const float4 *>(src + b * stride);
            s.x += x.x;
            s.y += x.y;
            s.z += x.z;
            s.w += x.w;
        }
        bb_store4((ET *)A.dp + row * A.lddp + col, s);
        return;
    }
    __shared__ float sm[4][64];
    const int hw = blockIdx.x - dp_blocks, h = hw >> 1, which = hw & 1;
    const int d = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long n = (long)A.B * A.nqt;
    float s = 0.f;
    for (long e = g; e < n; e += 4) s += A.col_part[(e * A.H + h) * 128 + which * 64 + d];
    sm[g][d] = s;
    __syncthreads();
    if (g == 0) (which ? A.dvb : A.du)[h * kDk + d] = ((sm[0][d] + sm[1][d]) + sm[2][d]) + sm[3][d];
}

}  // namespace pafc

// the workspace: dp_part (B, T, H * 64) | col_part (B * ceil(T / 16), H, 128), float32 | delta (B * T, H), float64
static void bb_workspace_floats(long B, long T, long H, size_t *dp_part, size_t *col_part, size_t *delta) {
    *dp_part = (size_t)B * T * H * 64;
    *col_part = (size_t)B * ((T + 15) / 16) * H * 128;
    *delta = (size_t)B * T * H;
}

extern "C" size_t pafc_mha_band_bwd_workspace_bytes(int B, int T, int H) {
    if (B <= 0 || T <= 0 || H <= 0) return 0;
    size_t a, b, c;
    bb_workspace_floats(B, T, H, &a, &b, &c);
    return (a + b) * sizeof(float) + c * sizeof(double);
}

extern "C" int pafc_mha_band_bwd(int dtype, int B, int T, int H, int dk, int w, int t_pad, const void *q, long ldq, const void *k,
                                 const void *v, long ldkv, const void *p, long ldp, const void *pos_bias_u,
                                 const void *pos_bias_v, const void *out, long ldo, const void *dout, long lddo, const float *lse,
                                 void *dq, long lddq, void *dk_out, void *dv_out, long lddkv, void *dp, long lddp, float *du,
                                 float *dvb, void *workspace, size_t workspace_bytes, pafc_stream_t stream) {
    if (!q || !k || !v || !p || !pos_bias_u || !pos_bias_v || !out || !dout || !lse || !dq || !dk_out || !dv_out || !dp || !du ||
        !dvb || !workspace)
        return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (B <= 0 || T <= 0 || H <= 0 || dk <= 0 || w < 0 || t_pad < T || B > 65535 || H > 65535 || t_pad > (1 << 30))
        return PAFC_ERR_BAD_DIMS;
    if (dk != pafc::kDk) return PAFC_ERR_UNSUPPORTED;
    // the reduce launch's grid, one block per 256 groups of four dp values plus two per head, must fit a grid dimension
    const long reduce_blocks = ((long)T * H * 16 + 255) / 256 + 2L * H;
    if (reduce_blocks > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    const long width = (long)H * dk, per16 = dtype == PAFC_F32 ? 4 : 8;
    const long lds[8] = {ldq, ldkv, ldp, ldo, lddo, lddq, lddkv, lddp};
    for (long ld : lds)
        if (ld < width || ld % per16) return PAFC_ERR_BAD_DIMS;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)p | (uintptr_t)pos_bias_u | (uintptr_t)pos_bias_v |
         (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk_out | (uintptr_t)dv_out | (uintptr_t)dp |
         (uintptr_t)workspace) & 15)
        return PAFC_ERR_ALIGNMENT;
    if (((uintptr_t)lse | (uintptr_t)du | (uintptr_t)dvb) & 3) return PAFC_ERR_ALIGNMENT;
    if (workspace_bytes < pafc_mha_band_bwd_workspace_bytes(B, T, H)) return PAFC_ERR_WORKSPACE;
    size_t n_dp, n_col, n_delta;
    bb_workspace_floats(B, T, H, &n_dp, &n_col, &n_delta);
    float *ws = (float *)workspace;
    const int nqt = (T + 15) / 16;
    // |j - i| < t_pad for every pair: a wider band is the same band, and i + w stays far from the int range.  The padding
    // keys reach the backward through lse alone, so t_pad is not needed beyond this.
    pafc::BandBwdArgs a{B, T, H, w < t_pad ? w : t_pad, nqt, q, ldq, k, v, ldkv, p, ldp, pos_bias_u, pos_bias_v, out, ldo, dout,
                        lddo, lse, dq, lddq, dk_out, dv_out, lddkv, dp, lddp, du, dvb, ws, ws + n_dp, (double *)(ws + n_dp + n_col)};
    const dim3 grid((unsigned)((T + 63) / 64), (unsigned)H, (unsigned)B), block(pafc::kBbWaves * pafc::kWave);
    const unsigned dp_blocks = (unsigned)(((long)T * H * 16 + 255) / 256);
    const dim3 rgrid(dp_blocks + 2u * (unsigned)H);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32) {
        hipLaunchKernelGGL((pafc::mha_band_bwd_dq_kernel<float>), grid, block, 0, s, a);
        hipLaunchKernelGGL((pafc::mha_band_bwd_dkv_kernel<float>), grid, block, 0, s, a);
        hipLaunchKernelGGL((pafc::mha_band_bwd_reduce_kernel<float>), rgrid, dim3(256), 0, s, a, dp_blocks);
    } else {
        hipLaunchKernelGGL((pafc::mha_band_bwd_dq_kernel<pafc::bf16_t>), grid, block, 0, s, a);
        hipLaunchKernelGGL((pafc::mha_band_bwd_dkv_kernel<pafc::bf16_t>), grid, block, 0, s, a);
        hipLaunchKernelGGL((pafc::mha_band_bwd_reduce_kernel<pafc::bf16_t>), rgrid, dim3(256), 0, s, a, dp_blocks);
    }
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
