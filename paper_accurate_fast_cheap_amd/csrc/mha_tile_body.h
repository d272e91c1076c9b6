// The wave body of the tiled attention kernels, shared by pafc_mha_rows (mha_rows.hip: packed row groups, one block per group and
// head) and pafc_mha_band (mha_band.hip: banded self-attention with a positional term, one block per query tile, head and batch
// row).  A wave owns 16 queries and walks its keys in tiles with an online softmax; both products are computed TRANSPOSED, so
// that no value changes lanes between them:
//   S^T (keys x queries) = K Q^T     lane l holds S^T[key 4(l>>4) + r][query l&15] in register r = 0..3 (the C/D map)
//   O^T (dk x queries)  = V^T P^T    and exactly that register is the B operand P^T[k-slot l>>4][query l&15] of the second
//                                     product when its step r sums over the keys 4(l>>4) + r: the A operand V^T is read
//                                     from memory in that key order, P never leaves its registers.
// A query is a lane column of both results: its running maximum and sum are one scalar per lane, reduced over the four
// 16-lane groups with two shuffles.  What differs between the kernels -- which keys a wave walks, how a score is formed and
// masked -- stays in their own files; the softmax step and the output store are here.
#pragma once
#include "pafc_common.h"

#include <math.h>

namespace pafc {

constexpr int kDk = 64;

__device__ __forceinline__ float max_over_lane_groups(float x) {
    x = fmaxf(x, __shfl_xor(x, 16, kWave));
    return fmaxf(x, __shfl_xor(x, 32, kWave));
}
__device__ __forceinline__ float sum_over_lane_groups(float x) {
    x += __shfl_xor(x, 16, kWave);
    return x + __shfl_xor(x, 32, kWave);
}

// One online-softmax step of a lane's query over NR masked scores s[] (already scaled; -inf = masked): updates m, l, rescales
// o, leaves the probabilities in s.  ROUND: the probabilities as bf16 values.  m must not be -inf together with a tile whose
// scores are all masked for the query (exp(-inf + inf)): a kernel in which that can happen starts m at a finite floor.
template <int NR, bool ROUND>
__device__ __forceinline__ void softmax_step(float *s, float &m, float &l, f32x4 *o) {
    float tmax = s[0];
#pragma unroll
    for (int r = 1; r < NR; ++r) tmax = fmaxf(tmax, s[r]);
    const float m_new = fmaxf(m, max_over_lane_groups(tmax));
    const float alpha = expf(m - m_new);                         // (m = -inf before the first tile: 0)
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        float p = expf(s[r] - m_new);
        if (ROUND) p = round_bf16(p);
        s[r] = p;
        psum += p;
    }
    l = l * alpha + sum_over_lane_groups(psum);
    m = m_new;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] *= alpha;
}

// O^T of a wave's 16 queries -> out[row, h*64 ...] * inv: lane (lr = l&15, lq = l>>4) holds the dimensions 16c + 4lq + r of
// query lr in o[c][r]; row is the lane's own query row, valid whether it exists.
template <typename ET>
__device__ __forceinline__ void store_tile(void *out, long ldo, int h, long row, bool valid, int lq, const f32x4 *o, float inv);
template <>
__device__ __forceinline__ void store_tile<float>(void *out, long ldo, int h, long row, bool valid, int lq, const f32x4 *o,
                                                 float inv) {
    if (!valid) return;
    float *op = (float *)out + row * ldo + h * kDk + lq * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        *reinterpret_cast<float4 *>(op + 16 * c) = make_float4(o[c][0] * inv, o[c][1] * inv, o[c][2] * inv, o[c][3] * inv);
}
template <>
__device__ __forceinline__ void store_tile<bf16_t>(void *out, long ldo, int h, long row, bool valid, int lq, const f32x4 *o,
                                                  float inv) {
    if (!valid) return;
    bf16_t *op = (bf16_t *)out + row * ldo + h * kDk + lq * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint2 w;
        w.x = pack_bf16_rne(o[c][0] * inv, o[c][1] * inv);
        w.y = pack_bf16_rne(o[c][2] * inv, o[c][3] * inv);
        *reinterpret_cast<uint2 *>(op + 16 * c) = w;
    }
}

// P V of one bf16 key tile of 32: s[8] holds the lane's probabilities (bf16 values) in the order element j of the PV operands
// is read -- key 4 lq + j (j < 4) of the first 16-key half, then 4 lq + j - 4 of the second -- and vp[j] points at V[that key]
// [lane & 15]; adds into O^T.
__device__ __forceinline__ void pv_tile_bf16(const float *s, const bf16_t *const *vp, f32x4 *o) {
    u32x4 pb;
#pragma unroll
    for (int j = 0; j < 4; ++j) pb[j] = pack_bf16_exact(s[2 * j], s[2 * j + 1]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        u32x4 va;
#pragma unroll
        for (int j = 0; j < 4; ++j) va[j] = (uint32_t)vp[2 * j][16 * c] | ((uint32_t)vp[2 * j + 1][16 * c] << 16);
        o[c] = mfma_bf16_packed(va, pb, o[c]);
    }
}

// The same for one fp32 key tile of 16: s[r] the probability of key 4 lq + r, vp[r] at V[that key][lane & 15].
__device__ __forceinline__ void pv_tile_f32(const float *s, const float *const *vp, f32x4 *o) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[r][16 * c], s[r], o[c], 0, 0, 0);
}

// ---- shared by the banded kernels (mha_band.hip, mha_band_bwd.hip) ----
// does query i see key `key` (|key - i| <= w, a real key)?
__device__ __forceinline__ bool band_sees(int key, int i, int w, int T) { return key < T && key >= i - w && key <= i + w; }

// the biased query fragments [q + u | q + v] of the lane's query, in the layout the tile body multiplies
__device__ __forceinline__ void band_query(const float *qp, const float *up, const float *vbp, float *qa, float *qb) {
    float uu[16], vv[16];
    load8<float>(qp, qa);
    load8<float>(qp + 8, qa + 8);
    load8<float>(up, uu);
    load8<float>(up + 8, uu + 8);
    load8<float>(vbp, vv);
    load8<float>(vbp + 8, vv + 8);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        qb[e] = qa[e] + vv[e];
        qa[e] = qa[e] + uu[e];
    }
}
__device__ __forceinline__ void band_query(const bf16_t *qp, const bf16_t *up, const bf16_t *vbp, uint4 *qa, uint4 *qb) {
#pragma unroll
    for (int part = 0; part < 2; ++part) {                 // dimensions 8 lq + [0, 8) and 32 + 8 lq + [0, 8)
        float q[8], uu[8], vv[8], su[8], sv[8];
        load8<bf16_t>(qp + 32 * part, q);
        load8<bf16_t>(up + 32 * part, uu);
        load8<bf16_t>(vbp + 32 * part, vv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            su[e] = q[e] + uu[e];
            sv[e] = q[e] + vv[e];
        }
        qa[part] = make_uint4(pack_bf16_rne(su[0], su[1]), pack_bf16_rne(su[2], su[3]), pack_bf16_rne(su[4], su[5]),
                              pack_bf16_rne(su[6], su[7]));
        qb[part] = make_uint4(pack_bf16_rne(sv[0], sv[1]), pack_bf16_rne(sv[2], sv[3]), pack_bf16_rne(sv[4], sv[5]),
                              pack_bf16_rne(sv[6], sv[7]));
    }
}

}  // namespace pafc
