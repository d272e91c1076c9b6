// pafc_mha_band (include/pafc_attention.h): limited-context self-attention with the positional term of the Conformer baseline
// (wenet/transformer/attention.py:406-645 of the reference, global_tokens = 0).
//
// Query i of a batch row sees the keys j with |j - i| <= w and 0 <= j < t_pad; for a real key (j < T)
//   s_ij = ((q_i + u_h) . k_j + (q_i + v_h) . p_j) / 8,
// p_j the KEY's position row, and every key of [T, t_pad) is zero padding that is not masked: score 0, value 0.
//
// Grid (query tile of 64, head, batch row), four waves, a wave owns 16 queries [a, a + 15] and walks the keys
// [max(0, a - w), min(T - 1, a + 15 + w)] in tiles; the wave body -- transposed products, P in the C/D registers as the next B
// operand, online softmax with one running maximum and sum per lane -- is mha_tile_body.h, shared with mha_rows.hip.
//   * One dot product: s_ij = [q_i + u | q_i + v] . [k_j | p_j], 128 deep.  The two biased query fragments are formed once per
//     wave (bf16: rounded to bf16, as a bf16 module rounds q + u); a key tile's A operand is its k rows followed by its p rows.
//     fp32 runs the two halves as two independent accumulator chains (a dependent v_mfma_f32_16x16x4_f32 waits 40 cycles, an
//     independent one issues after 32) and adds them, which is also where the reference adds its two score matrices.
//   * Band edges: the queries [a, a + 15] see every key of [a + 15 - w, a + w] unmasked, so only the first and the last
//     tiles of a walk run the per-element test (a wave-uniform choice between two instantiations of the tile body).  A lane's
//     first tile may hold no key of its query: the running maximum starts at a finite floor, not at -inf.
//   * Padding keys are arithmetic: query i has n0 = max(0, min(t_pad - 1, i + w) - T + 1) of them, folded in once after the
//     walk as m' = max(m, 0), l' = l e^(m - m') + n0 e^(-m').  Nothing past row T - 1 of any operand is read: row indices are
//     clamped and the duplicates masked (keys) or not stored (queries).
//   * A tile's K / P fragments are loaded one tile ahead of the products that read them (band_load); V is read where it is used.
//   * Key reuse: neighbouring query tiles read almost the same keys.  Blocks are dealt round-robin over the eight XCDs, each
//     with its own L2, so the tile index is remapped to give every XCD one contiguous run of a head's tiles (a bijection for
//     every grid width; placement changes speed only).
// w >= t_pad makes the band cover everything: full attention with the positional term.
// pafc_mha_band_lse is the same kernel instantiated with one more store per query and head, lse = m' + log(l') (the padding
// keys' term included), for the backward (mha_band_bwd.hip); the arithmetic of `out` is untouched, so it carries the same bits.
#include "pafc_attention.h"
#include "mha_tile_body.h"

namespace pafc {

constexpr int kBandWaves = 4;
constexpr float kBandFloor = -1e30f;      // the running maximum before a query has seen a key: finite (see above)

struct BandArgs {
    int T, H, w, t_pad;
    const void *q; long ldq;
    const void *k, *v; long ldkv;
    const void *p; long ldp;
    const void *u, *vb;
    void *out; long ldo;
    float *lse;                // (B*T, H), written by the LSE instantiation only
};

// blockIdx.x -> query tile: the blocks x, x + 8, x + 16, ... (one XCD under round-robin placement) get consecutive tiles
__device__ __forceinline__ int band_tile_of_block(int bid, int n) {
    const int q = n >> 3, r = n & 7, x = bid & 7, idx = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + idx;
}

// the padding keys of query i (score 0, value 0), folded into the finished walk
__device__ __forceinline__ void band_fold_padding(const BandArgs &A, int i, float &m, float &l, f32x4 *o) {
    const int n0 = min(A.t_pad - 1, i + A.w) - A.T + 1;
    if (n0 <= 0) return;
    const float m_new = fmaxf(m, 0.f), alpha = expf(m - m_new);
    l = l * alpha + (float)n0 * expf(-m_new);
    m = m_new;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] *= alpha;
}

// A key tile's A operand [k rows | p rows] in the layout the products read, loaded one tile ahead of its use (band_load) so
// that the loads of tile n + 1 are in flight under the products and the softmax of tile n.
struct BandFragF32 { float ka[16], pa[16]; };
struct BandFragBf16 { uint4 ka[2][2], pa[2][2]; };          // [16-key half][dimensions 0-31 / 32-63]

__device__ __forceinline__ void band_load(const BandArgs &A, const float *kbase, const float *pbase, int k0, int lr, int lq,
                                          BandFragF32 &f) {
    const long krow = min(k0 + lr, A.T - 1);
    const float *kp = kbase + krow * A.ldkv + lq * 16, *pp = pbase + krow * A.ldp + lq * 16;
    load8<float>(kp, f.ka);
    load8<float>(kp + 8, f.ka + 8);
    load8<float>(pp, f.pa);
    load8<float>(pp + 8, f.pa + 8);
}
__device__ __forceinline__ void band_load(const BandArgs &A, const bf16_t *kbase, const bf16_t *pbase, int k0, int lr, int lq,
                                          BandFragBf16 &f) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long krow = min(k0 + 16 * half + lr, A.T - 1);
        const bf16_t *kp = kbase + krow * A.ldkv + lq * 8, *pp = pbase + krow * A.ldp + lq * 8;
        f.ka[half][0] = *reinterpret_cast<const uint4 *>(kp);
        f.ka[half][1] = *reinterpret_cast<const uint4 *>(kp + 32);
        f.pa[half][0] = *reinterpret_cast<const uint4 *>(pp);
        f.pa[half][1] = *reinterpret_cast<const uint4 *>(pp + 32);
    }
}

// fp32: one key tile of 16 from key k0
template <bool EDGE>
__device__ __forceinline__ void band_tile(const BandArgs &A, const BandFragF32 &f, const float *vbase, const float *qa,
                                          const float *qb, int k0, int i, int lr, int lq, float &m, float &l, f32x4 *o) {
    f32x4 sk = {0.f, 0.f, 0.f, 0.f}, sp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        sk = __builtin_amdgcn_mfma_f32_16x16x4f32(f.ka[e], qa[e], sk, 0, 0, 0);
        sp = __builtin_amdgcn_mfma_f32_16x16x4f32(f.pa[e], qb[e], sp, 0, 0, 0);
    }
    float s[4];
    const float *vp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int key = k0 + lq * 4 + r;
        const float sc = (sk[r] + sp[r]) * 0.125f;                  // 1 / sqrt(64), exact
        s[r] = (!EDGE || band_sees(key, i, A.w, A.T)) ? sc : -INFINITY;
        vp[r] = vbase + (long)min(key, A.T - 1) * A.ldkv + lr;
    }
    softmax_step<4, false>(s, m, l, o);
    pv_tile_f32(s, vp, o);
}

// bf16: one key tile of 32 from key k0
template <bool EDGE>
__device__ __forceinline__ void band_tile(const BandArgs &A, const BandFragBf16 &f, const bf16_t *vbase, const uint4 *qa,
                                          const uint4 *qb, int k0, int i, int lr, int lq, float &m, float &l, f32x4 *o) {
    float s[8];
    const bf16_t *vp[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
        st = mfma_bf16_packed(f.ka[half][0], qa[0], st);
        st = mfma_bf16_packed(f.ka[half][1], qa[1], st);
        st = mfma_bf16_packed(f.pa[half][0], qb[0], st);
        st = mfma_bf16_packed(f.pa[half][1], qb[1], st);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 16 * half + lq * 4 + r;
            s[4 * half + r] = (!EDGE || band_sees(key, i, A.w, A.T)) ? st[r] * 0.125f : -INFINITY;
            vp[4 * half + r] = vbase + (long)min(key, A.T - 1) * A.ldkv + lr;
        }
    }
    softmax_step<8, true>(s, m, l, o);
    pv_tile_bf16(s, vp, o);
}

template <typename ET> struct BandFrag;
template <> struct BandFrag<float> { typedef float type; typedef BandFragF32 keys; static constexpr int kN = 16, kTile = 16, kLane = 16; };
template <> struct BandFrag<bf16_t> { typedef uint4 type; typedef BandFragBf16 keys; static constexpr int kN = 2, kTile = 32, kLane = 8; };

template <typename ET, bool LSE> __global__ __launch_bounds__(kBandWaves * kWave) void mha_band_kernel(BandArgs A) {
    typedef BandFrag<ET> F;
    const int tile = band_tile_of_block(blockIdx.x, gridDim.x);
    const int h = blockIdx.y;
    const long row0 = (long)blockIdx.z * A.T;              // the batch row's first frame (64-bit: B * T * pitch passes 2^31)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = 64 * tile + 16 * wave;
    if (a >= A.T) return;
    const int lr = lane & 15, lq = lane >> 4;
    const int T = A.T, w = A.w;
    const int i = min(a + lr, T - 1);                      // the lane's query; a duplicate of the last one is not stored
    typename F::type qa[F::kN], qb[F::kN];
    band_query((const ET *)A.q + (row0 + i) * A.ldq + h * kDk + lq * F::kLane, (const ET *)A.u + h * kDk + lq * F::kLane,
               (const ET *)A.vb + h * kDk + lq * F::kLane, qa, qb);
    const ET *kbase = (const ET *)A.k + row0 * A.ldkv + h * kDk, *vbase = (const ET *)A.v + row0 * A.ldkv + h * kDk;
    const ET *pbase = (const ET *)A.p + h * kDk;
    const int last = min(a + 15, T - 1);
    const int klo = max(0, a - w), khi = min(T - 1, last + w);
    const int in_lo = last - w, in_hi = min(a + w, T - 1);  // every key of [in_lo, in_hi] is seen by all 16 queries
    float m = kBandFloor, l = 0.f;
    f32x4 o[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    typename F::keys cur, nxt;
    band_load(A, kbase, pbase, klo, lr, lq, cur);
    for (int k0 = klo; k0 <= khi; k0 += F::kTile) {
        band_load(A, kbase, pbase, min(k0 + F::kTile, khi), lr, lq, nxt);     // (past the walk's end: a tile nobody uses, rows clamped)
        if (k0 >= in_lo && k0 + F::kTile - 1 <= in_hi)
            band_tile<false>(A, cur, vbase, qa, qb, k0, i, lr, lq, m, l, o);
        else
            band_tile<true>(A, cur, vbase, qa, qb, k0, i, lr, lq, m, l, o);
        cur = nxt;
    }
    band_fold_padding(A, i, m, l, o);
    if (LSE && lq == 0 && a + lr < T) A.lse[(row0 + a + lr) * A.H + h] = m + logf(l);
    store_tile<ET>(A.out, A.ldo, h, row0 + a + lr, a + lr < T, lq, o, 1.f / l);
}

}  // namespace pafc

static int mha_band_launch(int dtype, int B, int T, int H, int dk, int w, int t_pad, const void *q, long ldq, const void *k,
                           const void *v, long ldkv, const void *p, long ldp, const void *pos_bias_u, const void *pos_bias_v,
                           void *out, long ldo, float *lse, bool want_lse, pafc_stream_t stream) {
    if (!q || !k || !v || !p || !pos_bias_u || !pos_bias_v || !out || (want_lse && !lse)) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (B <= 0 || T <= 0 || H <= 0 || dk <= 0 || w < 0 || t_pad < T || B > 65535 || H > 65535 || t_pad > (1 << 30))
        return PAFC_ERR_BAD_DIMS;
    if (dk != pafc::kDk) return PAFC_ERR_UNSUPPORTED;
    const long width = (long)H * dk, per16 = dtype == PAFC_F32 ? 4 : 8;
    if (ldq < width || ldkv < width || ldp < width || ldo < width || ldq % per16 || ldkv % per16 || ldp % per16 || ldo % per16)
        return PAFC_ERR_BAD_DIMS;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)p | (uintptr_t)pos_bias_u | (uintptr_t)pos_bias_v |
         (uintptr_t)out) & 15)
        return PAFC_ERR_ALIGNMENT;
    if (want_lse && ((uintptr_t)lse & 3)) return PAFC_ERR_ALIGNMENT;
    // |j - i| < t_pad for every pair: a wider band is the same band, and i + w stays far from the int range
    pafc::BandArgs a{T, H, w < t_pad ? w : t_pad, t_pad, q, ldq, k, v, ldkv, p, ldp, pos_bias_u, pos_bias_v, out, ldo, lse};
    const dim3 grid((unsigned)((T + 63) / 64), (unsigned)H, (unsigned)B), block(pafc::kBandWaves * pafc::kWave);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32) {
        if (want_lse)
            hipLaunchKernelGGL((pafc::mha_band_kernel<float, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((pafc::mha_band_kernel<float, false>), grid, block, 0, s, a);
    } else {
        if (want_lse)
            hipLaunchKernelGGL((pafc::mha_band_kernel<pafc::bf16_t, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((pafc::mha_band_kernel<pafc::bf16_t, false>), grid, block, 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_mha_band(int dtype, int B, int T, int H, int dk, int w, int t_pad, const void *q, long ldq, const void *k,
                             const void *v, long ldkv, const void *p, long ldp, const void *pos_bias_u, const void *pos_bias_v,
                             void *out, long ldo, pafc_stream_t stream) {
    return mha_band_launch(dtype, B, T, H, dk, w, t_pad, q, ldq, k, v, ldkv, p, ldp, pos_bias_u, pos_bias_v, out, ldo, nullptr,
                           false, stream);
}

extern "C" int pafc_mha_band_lse(int dtype, int B, int T, int H, int dk, int w, int t_pad, const void *q, long ldq,
                                 const void *k, const void *v, long ldkv, const void *p, long ldp, const void *pos_bias_u,
                                 const void *pos_bias_v, void *out, long ldo, float *lse, pafc_stream_t stream) {
    return mha_band_launch(dtype, B, T, H, dk, w, t_pad, q, ldq, k, v, ldkv, p, ldp, pos_bias_u, pos_bias_v, out, ldo, lse, true,
                           stream);
}
