// The two kernels of the attention decoder's second pass (include/pafc_attention.h): multi-head attention over packed row
// groups, and log p(target) per row straight from the logits.
//
// pafc_mha_rows.  One block per (group, head), four waves; a wave owns the 16-query tiles t = wave, wave + 4, ... of the group
// and walks the keys in tiles with an online softmax (the softmax step, the PV product and the output store are
// mha_tile_body.h, shared with mha_band.hip).  Both products are computed TRANSPOSED, so that no value changes lanes
// between them:
//   S^T (keys x queries) = K Q^T     lane l holds S^T[key 4(l>>4) + r][query l&15] in register r = 0..3 (the C/D map)
//   O^T (dk x queries)  = V^T P^T    and exactly that register is the B operand P^T[k-slot l>>4][query l&15] of the second
//                                     product when its step r sums over the keys 4(l>>4) + r: the A operand V^T is read
//                                     from memory in that key order, P never leaves its registers.
// A query is a lane column of both results: its running maximum and sum are one scalar per lane, reduced over the four
// 16-lane groups with two shuffles.  fp32: v_mfma_f32_16x16x4_f32 (exact products, fp32 accumulation), key tiles of 16; the k
// order of Q K^T is permuted (slot l>>4 of step e is dimension 16(l>>4) + e) so that a lane reads 64 contiguous bytes of its
// row.  bf16: v_mfma_f32_16x16x32_bf16, key tiles of 32 (two S^T tiles feed one PV step), P rounded to bf16 and the running
// sum taken over the rounded values, so the weights PV applies sum to one.
// Rows past the end of a group or of its keys are never read: the row index is clamped to the last valid one and the
// duplicate is masked (keys: -inf before the softmax) or not stored (queries).
// pafc_mha_rows_lse is the same kernel instantiated with one more store per query row and head, lse = m + log(l), for the
// backward (mha_rows_bwd.hip); the arithmetic of `out` is untouched, so it carries the same bits.
#include "pafc_attention.h"
#include "mha_tile_body.h"

namespace pafc {

constexpr int kMhaWaves = 4;

struct MhaArgs {
    int H;
    const void *q; long ldq;
    const void *k, *v; long ldkv;
    const int32_t *q_off, *kv_off, *kv_len;
    int causal;
    void *out; long ldo;
    float *lse;          // (rows, H) m + log(l) of every query row and head: the LSE instantiations only
};

// fp32: one 16-query tile against keys [0, kend)
template <bool LSE>
__device__ __forceinline__ void mha_tile(const MhaArgs &a, float, int h, int q0, int nq, int kv0, int nkv, int t, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const int qidx = 16 * t + lr;
    const float *qp = (const float *)a.q + (long)(q0 + min(qidx, nq - 1)) * a.ldq + h * kDk + lq * 16;
    float qa[16];
    load8<float>(qp, qa);
    load8<float>(qp + 8, qa + 8);
    const int kend = a.causal ? min(nkv, 16 * t + 16) : nkv;
    float m = -INFINITY, l = 0.f;
    f32x4 o[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float *kbase = (const float *)a.k + h * kDk, *vbase = (const float *)a.v + h * kDk;
    for (int k0 = 0; k0 < kend; k0 += 16) {
        const float *kp = kbase + (long)(kv0 + min(k0 + lr, nkv - 1)) * a.ldkv + lq * 16;
        float ka[16];
        load8<float>(kp, ka);
        load8<float>(kp + 8, ka + 8);
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 16; ++e) st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[e], qa[e], st, 0, 0, 0);
        float s[4];
        const float *vp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + lq * 4 + r;
            const bool seen = key < nkv && (!a.causal || key <= qidx);
            s[r] = seen ? st[r] * 0.125f : -INFINITY;              // 1 / sqrt(64), exact
            vp[r] = vbase + (long)(kv0 + min(key, nkv - 1)) * a.ldkv + lr;
        }
        softmax_step<4, false>(s, m, l, o);
        pv_tile_f32(s, vp, o);
    }
    store_tile<float>(a.out, a.ldo, h, (long)q0 + qidx, qidx < nq, lq, o, 1.f / l);
    if (LSE && lq == 0 && qidx < nq) a.lse[((long)q0 + qidx) * a.H + h] = m + logf(l);
}

// bf16: the same tile, keys in steps of 32
template <bool LSE>
__device__ __forceinline__ void mha_tile(const MhaArgs &a, bf16_t, int h, int q0, int nq, int kv0, int nkv, int t, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const int qidx = 16 * t + lr;
    const bf16_t *qp = (const bf16_t *)a.q + (long)(q0 + min(qidx, nq - 1)) * a.ldq + h * kDk + lq * 8;
    const uint4 qa0 = *reinterpret_cast<const uint4 *>(qp), qa1 = *reinterpret_cast<const uint4 *>(qp + 32);
    const int kend = a.causal ? min(nkv, 16 * t + 16) : nkv;
    float m = -INFINITY, l = 0.f;
    f32x4 o[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const bf16_t *kbase = (const bf16_t *)a.k + h * kDk, *vbase = (const bf16_t *)a.v + h * kDk;
    for (int k0 = 0; k0 < kend; k0 += 32) {
        float s[8];
        const bf16_t *vp[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const bf16_t *kp = kbase + (long)(kv0 + min(k0 + 16 * half + lr, nkv - 1)) * a.ldkv + lq * 8;
            const uint4 ka0 = *reinterpret_cast<const uint4 *>(kp), ka1 = *reinterpret_cast<const uint4 *>(kp + 32);
            f32x4 st = {0.f, 0.f, 0.f, 0.f};
            st = mfma_bf16_packed(ka0, qa0, st);
            st = mfma_bf16_packed(ka1, qa1, st);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * half + lq * 4 + r;
                const bool seen = key < nkv && (!a.causal || key <= qidx);
                s[4 * half + r] = seen ? st[r] * 0.125f : -INFINITY;
                vp[4 * half + r] = vbase + (long)(kv0 + min(key, nkv - 1)) * a.ldkv + lr;
            }
        }
        softmax_step<8, true>(s, m, l, o);
        // element j of the PV operands is key k0 + 4 lq + j (j < 4) or k0 + 16 + 4 lq + j - 4: the order s[] is in
        pv_tile_bf16(s, vp, o);
    }
    store_tile<bf16_t>(a.out, a.ldo, h, (long)q0 + qidx, qidx < nq, lq, o, 1.f / l);
    if (LSE && lq == 0 && qidx < nq) a.lse[((long)q0 + qidx) * a.H + h] = m + logf(l);
}

template <typename ET, bool LSE> __global__ __launch_bounds__(kMhaWaves * kWave) void mha_rows_kernel(MhaArgs a) {
    const int g = blockIdx.x, h = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = a.q_off[g], nq = a.q_off[g + 1] - q0;
    if (nq <= 0) return;
    const int kv0 = a.kv_off[g], nkv = a.kv_len[g];
    const int ntile = (nq + 15) >> 4;
    for (int t = wave; t < ntile; t += kMhaWaves) {
        if (nkv <= 0) {                                   // no keys: zeros
            const f32x4 z[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            const int qidx = 16 * t + (lane & 15);
            store_tile<ET>(a.out, a.ldo, h, (long)q0 + qidx, qidx < nq, lane >> 4, z, 0.f);
            if (LSE && lane < 16 && qidx < nq) a.lse[((long)q0 + qidx) * a.H + h] = -INFINITY;       // the sum over no keys
            continue;
        }
        mha_tile<LSE>(a, ET(), h, q0, nq, kv0, nkv, t, lane);
    }
}

// ---- log p(target) per row ----
// One block per row: every thread keeps a running (max, sum of exp) over its strided share of the row, the block merges the
// pairs, thread 0 reads the target's logit.
__device__ __forceinline__ void lse_merge(float &m, float &s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    const float a = (m == -INFINITY) ? 0.f : s * expf(m - M);
    const float b = (m2 == -INFINITY) ? 0.f : s2 * expf(m2 - M);
    m = M;
    s = a + b;
}

template <typename ET>
__global__ __launch_bounds__(256) void logp_gather_kernel(int V, const ET *x, long ldl, const int32_t *target, float *out) {
    const long r = blockIdx.x;
    const ET *row = x + r * ldl;
    float m = -INFINITY, s = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) {
        const float a = Elem<ET>::load(row + v);
        if (a > m) {
            s = s * expf(m - a) + 1.f;
            m = a;
        } else if (a > -INFINITY) {
            s += expf(a - m);
        } else if (a != a) {
            m = s = a;             // a NaN logit poisons the pair: it stays through every later update and merge, out = NaN
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lse_merge(m, s, __shfl_xor(m, off, kWave), __shfl_xor(s, off, kWave));
    __shared__ float sm[4], ss[4];
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6] = m;
        ss[threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) lse_merge(m, s, sm[w], ss[w]);
        const int t = target[r];
        out[r] = (t >= 0 && t < V) ? Elem<ET>::load(row + t) - (m + logf(s)) : NAN;
    }
}

}  // namespace pafc

static int mha_rows_launch(int dtype, int G, int H, int dk, const void *q, long ldq, const void *k, const void *v, long ldkv,
                           const int32_t *q_off, const int32_t *kv_off, const int32_t *kv_len, int causal, void *out, long ldo,
                           float *lse, bool want_lse, pafc_stream_t stream) {
    if (!q || !k || !v || !q_off || !kv_off || !kv_len || !out || (want_lse && !lse)) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (G <= 0 || H <= 0 || dk <= 0 || H > 65535) return PAFC_ERR_BAD_DIMS;
    if (dk != pafc::kDk) return PAFC_ERR_UNSUPPORTED;
    const long width = (long)H * dk, per16 = dtype == PAFC_F32 ? 4 : 8;
    if (ldq < width || ldkv < width || ldo < width || ldq % per16 || ldkv % per16 || ldo % per16) return PAFC_ERR_BAD_DIMS;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return PAFC_ERR_ALIGNMENT;
    pafc::MhaArgs a{H, q, ldq, k, v, ldkv, q_off, kv_off, kv_len, causal != 0, out, ldo, lse};
    const dim3 grid((unsigned)G, (unsigned)H), block(pafc::kMhaWaves * pafc::kWave);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32 && !want_lse)
        hipLaunchKernelGGL((pafc::mha_rows_kernel<float, false>), grid, block, 0, s, a);
    else if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::mha_rows_kernel<float, true>), grid, block, 0, s, a);
    else if (!want_lse)
        hipLaunchKernelGGL((pafc::mha_rows_kernel<pafc::bf16_t, false>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((pafc::mha_rows_kernel<pafc::bf16_t, true>), grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_mha_rows(int dtype, int G, int H, int dk, const void *q, long ldq, const void *k, const void *v, long ldkv,
                             const int32_t *q_off, const int32_t *kv_off, const int32_t *kv_len, int causal, void *out, long ldo,
                             pafc_stream_t stream) {
    return mha_rows_launch(dtype, G, H, dk, q, ldq, k, v, ldkv, q_off, kv_off, kv_len, causal, out, ldo, nullptr, false, stream);
}

extern "C" int pafc_mha_rows_lse(int dtype, int G, int H, int dk, const void *q, long ldq, const void *k, const void *v,
                                 long ldkv, const int32_t *q_off, const int32_t *kv_off, const int32_t *kv_len, int causal,
                                 void *out, long ldo, float *lse, pafc_stream_t stream) {
    return mha_rows_launch(dtype, G, H, dk, q, ldq, k, v, ldkv, q_off, kv_off, kv_len, causal, out, ldo, lse, true, stream);
}

extern "C" int pafc_logp_gather_rows(int dtype, long rows, int V, const void *logits, long ldl, const int32_t *target,
                                     float *out, pafc_stream_t stream) {
    if (!logits || !target || !out) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (rows <= 0 || V <= 0 || ldl < V || rows > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::logp_gather_kernel<float>), dim3((unsigned)rows), dim3(256), 0, s, V, (const float *)logits,
                           ldl, target, out);
    else
        hipLaunchKernelGGL((pafc::logp_gather_kernel<pafc::bf16_t>), dim3((unsigned)rows), dim3(256), 0, s, V,
                           (const pafc::bf16_t *)logits, ldl, target, out);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
