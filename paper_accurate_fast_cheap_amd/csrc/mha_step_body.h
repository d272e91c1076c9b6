// The single-query self-attention of one (row, head) by one wave, shared by pafc_mha_step (attn_search.hip: the keys through
// the ancestor table of a beam search in lockstep) and pafc_mha_step_paths (joint_search.hip: rows at different positions,
// the keys through a per-row table of cache rows).
//
// A step's self-attention is a GEMV per (row, head) over at most P keys of 64 dimensions, bound by the reads of the cache:
// nothing for the matrix cores.  QK runs with the lanes over the keys of a tile of 64 (a lane reads its key's 64 contiguous
// elements as 16-byte accesses and holds q in registers), the online softmax merges a tile with two wave reductions, and PV
// runs with the lanes over the 64 dimensions (one coalesced row segment per key, its probability and cache row broadcast
// from the lane that owns the key).
#pragma once
#include "pafc_common.h"

#include <math.h>

namespace pafc {

constexpr int kStepDk = 64;
constexpr int kStepWaves = 4;

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, kWave));
    return x;
}

// qkv: the row's stacked q | k | v (d = H * 64 each); the keys [0, p]: key j < p is the cache row key_row(j) (an int, inside
// the cache: the caller clamps), key p the row's own k and v, read from qkv.  slot: where the row's own [k | v] goes in the
// cache, or nullptr to store nothing.  out: the row's (H * 64) output.
template <typename ET, typename KeyRow>
__device__ __forceinline__ void mha_step_row(const ET *qkv, ET *cache, long d, int h, int lane, int p, ET *slot, KeyRow key_row,
                                             ET *out) {
    const ET *own_k = qkv + d + h * kStepDk, *own_v = qkv + 2 * d + h * kStepDk;
    // the row's own slot: k and v of this head, one element per lane
    if (slot) {
        slot[h * kStepDk + lane] = own_k[lane];
        slot[h * kStepDk + d + lane] = own_v[lane];
    }
    float q[kStepDk];
#pragma unroll
    for (int i = 0; i < kStepDk; i += 8) load8<ET>(qkv + h * kStepDk + i, q + i);
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int j0 = 0; j0 <= p; j0 += kWave) {
        const int j = j0 + lane;
        const bool valid = j <= p;
        // the cache row of key j (key p is read from qkv: the slot above was written by other lanes of this launch)
        int row = -1;
        if (valid && j < p) row = key_row(j);
        float s = -INFINITY;
        if (valid) {
            const ET *kr = row >= 0 ? cache + (long)row * 2 * d + h * kStepDk : own_k;
            float dot = 0.f;
#pragma unroll
            for (int i = 0; i < kStepDk; i += 8) {
                float kk[8];
                load8<ET>(kr + i, kk);
#pragma unroll
                for (int e = 0; e < 8; ++e) dot = fmaf(q[i + e], kk[e], dot);
            }
            s = dot * 0.125f;
        }
        const float m_new = fmaxf(m, wave_max(s));          // finite: lane 0 of every tile is valid
        const float pj = valid ? expf(s - m_new) : 0.f;
        const float scale = expf(m - m_new);                // 0 on the first tile (m = -inf)
        l = l * scale + wave_sum(pj);
        acc *= scale;
        const int n = min(kWave, p + 1 - j0);
        for (int jj = 0; jj < n; ++jj) {
            const float pb = __shfl(pj, jj, kWave);
            const int rb = __shfl(row, jj, kWave);
            const ET *vr = rb >= 0 ? cache + (long)rb * 2 * d + d + h * kStepDk : own_v;
            acc = fmaf(pb, Elem<ET>::load(vr + lane), acc);
        }
        m = m_new;
    }
    Elem<ET>::store(out + h * kStepDk + lane, acc / l);
}

}  // namespace pafc
