// Backward of the Mamba-2 selective scan (SSD) on the bf16 matrix cores (C ABI: include/pafc_encoder_ops.h:
// pafc_mamba2_scan_backward).  Forward, per head (mamba2_scan.hip):  h_t = a_t h_{t-1} + dt_t B_t x_t^T,  y_t = C_t . h_t.
// With gy = dL/dy and the adjoint state G_t = C_t gy_t^T + a_{t+1} G_{t+1} (N x P, walked right to left):
//     gxu_t = B_t . G_t      g_x_t = dt_t gxu_t      g_dt_t = gxu_t . x_t
//     g_B_t = sum_heads dt_t G_t x_t                 g_C_t = sum_heads h_t gy_t
//     g_la_t = a_t <G_t, h_{t-1}> = sum_{s >= t} (gy_s . y_s - dt_s g_dt_s) = sum_{s >= t} (C_s . gC_s - B_s . gB_s)   per head
// (the last form needs neither y nor both states at once: gC_s, gB_s are the head's own terms of g_C, g_B).
// Two sweeps in blocks of 16 steps, one wave64 per (chunk, batch x head), each with one 128 x 64 fp32 state in registers:
//   h sweep, left to right, state h^T [p][n] (contraction over the head channels p):  with cum_t the block's inclusive prefix
//     of log a and H the state entering the block
//       gC_t = e^{cum_t} H gy_t + sum_{s <= t} e^{cum_t - cum_s} dt_s (x_s . gy_t) B_s
//   G sweep, right to left, state G [n][p] as the forward's; with X = a_16 G_16 the adjoint entering the block from the right
//       G_t   = sum_{s >= t} e^{cum_s - cum_t} C_s gy_s^T + e^{cum_15 - cum_t} X           X' = sum_s e^{cum_s} C_s gy_s^T + e^{cum_15} X
//       gxu_t = sum_{s >= t} e^{cum_s - cum_t} (B_t . C_s) gy_s + e^{cum_15 - cum_t} B_t . X
//       gB_t  = dt_t [ sum_{s >= t} e^{cum_s - cum_t} (gy_s . x_t) C_s + e^{cum_15 - cum_t} X x_t ]
//     (X x_t contracts over p, which lies on the lanes of the state tiles: the tiles are transposed by selection MFMAs of
//      their hi and lo halves, which are the split operands the product needs anyway).
// All exponents are <= 0.  bf16 inputs (x, B, C) enter MFMAs exactly; gy, the states and the decayed scalings enter as split
// hi + lo operands (products of two split operands keep hi hi + hi lo + lo hi).  Chunks: the forward's three passes, twice
// (chunk-local end states, scan over chunks, sweep), the adjoint's scan running right to left.  g_B / g_C: per-head fp32
// partials in the workspace, summed over heads in a fixed order and rounded to bf16 once.  Operand layouts: mamba2_scan.hip.
#include "pafc_common.h"
#include "../../include/pafc_encoder_ops.h"

namespace pafc {
namespace {

#include "mamba2_ssd.inc"

struct SsdBwdParams {
    const bf16_t *xbc;     // (B, L, ldx): [x | B | C]
    long ldx;
    const float *dt, *la;  // (B, L, H)
    const float *gy;       // (B, L, d_inner)
    bf16_t *g_xbc;         // (B, L, ldg): [g_x | g_B | g_C]
    long ldg;
    float *g_dt, *g_la;    // (B, L, H); g_la may be null
    int B, L, H, d_inner, Lc, NC, reverse;
    int c_off;             // chunk of blockIdx.x == 0 (the chunk-local pass of the adjoint skips chunk 0)
    float *ws_h, *ws_g;    // [B][H][NC][64 x 128] / [128 x 64]: state entering each chunk (h from the left, G from the right)
    float *ws_hd, *ws_gd;  // [B][H][NC]: decay product of the chunk
    float *pB, *pC;        // [B][L][H][128]: this head's terms of g_B, g_C
    float *dla;            // [B][L][H]: C . gC - B . gB
};

__device__ __forceinline__ void sel_operands(int t16, int q, u32x4 &selA, u32x4 &selB) {
    selA = u32x4{0u, 0u, 0u, 0u};
    selB = u32x4{0u, 0u, 0u, 0u};
    const int e = t16 - 4 * q;
    const unsigned one_lo = 0x3f80u, one_hi = 0x3f800000u;
    if (e == 0) { selA[0] = one_lo; selB[2] = one_lo; }
    if (e == 1) { selA[0] = one_hi; selB[2] = one_hi; }
    if (e == 2) { selA[1] = one_lo; selB[3] = one_lo; }
    if (e == 3) { selA[1] = one_hi; selB[3] = one_hi; }
}
// a uint2 of four bf16 scaled by an fp32 factor, split: two packed pairs hi, two lo
struct SSplit4 { unsigned h0, h1, l0, l1; };
__device__ __forceinline__ SSplit4 scale_split(uint2 r, float f) {
    const float b0 = bf16_bits_to_f32(r.x & 0xffffu) * f, b1 = __uint_as_float(r.x & 0xffff0000u) * f;
    const float b2 = bf16_bits_to_f32(r.y & 0xffffu) * f, b3 = __uint_as_float(r.y & 0xffff0000u) * f;
    const Bf16HiLo u0 = split_bf16_hilo(b0, b1), u1 = split_bf16_hilo(b2, b3);
    return SSplit4{u0.hi, u1.hi, u0.lo, u1.lo};
}
// two rows-by-time tiles (Lt layout, exact bf16) -> time-by-channel operands (lane = channel, slot = step)
__device__ __forceinline__ void transpose_pair(u32x4 v, u32x4 selA, u32x4 selB, u32x4 &o0, u32x4 &o1) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 t0 = mfma_bf16_packed(v, selA, zero4), t1 = mfma_bf16_packed(v, selB, zero4);
    o0 = u32x4{pack_bf16_exact(t0[0], t0[1]), pack_bf16_exact(t0[2], t0[3]), 0u, 0u};
    o1 = u32x4{pack_bf16_exact(t1[0], t1[1]), pack_bf16_exact(t1[2], t1[3]), 0u, 0u};
}
__device__ __forceinline__ float dot4(float4 a, uint2 b) {
    return a.x * bf16_bits_to_f32(b.x & 0xffffu) + a.y * __uint_as_float(b.x & 0xffff0000u)
         + a.z * bf16_bits_to_f32(b.y & 0xffffu) + a.w * __uint_as_float(b.y & 0xffff0000u);
}
__device__ __forceinline__ float sum_over_q(float v) {     // the four lanes that share t16
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// ---- h sweep: EMIT = false: chunk-local end state and decay (pass A); EMIT = true: the head's g_C terms and C . gC ---------
// State tiles T[ip][jn]: lane (i = l & 15, qq = l >> 4), reg g <-> h[n = 16 jn + i][p = 16 ip + 4 qq + g].
template <bool EMIT>
__global__ __launch_bounds__(64, 2) void mamba2_ssd_bwd_h_kernel(const SsdBwdParams p) {
    const int c = blockIdx.x + p.c_off;
    const int b = blockIdx.y / p.H, h = blockIdx.y % p.H;
    const int lane = threadIdx.x, t16 = lane & 15, q = lane >> 4;
    __shared__ float s_cum[SBL], s_dt[SBL];
    __shared__ __attribute__((aligned(16))) float s_o[EMIT ? SBL : 1][SN + 4];

    u32x4 selA, selB;
    sel_operands(t16, q, selA, selB);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    const size_t seq = (size_t)b * p.H + h;
    f32x4 T[4][8];
    {
        const float *src = (EMIT && p.NC > 1) ? p.ws_h + (seq * p.NC + c) * (size_t)(SN * SP) : nullptr;
#pragma unroll
        for (int ip = 0; ip < 4; ++ip)
#pragma unroll
            for (int jn = 0; jn < 8; ++jn)
#pragma unroll
                for (int g = 0; g < 4; ++g) T[ip][jn][g] = src ? src[(16 * ip + 4 * q + g) * SN + 16 * jn + t16] : 0.f;
    }
    float lsum = 0.f;

    const int s_begin = c * p.Lc, s_end = min(p.L, s_begin + p.Lc);
    const bf16_t *xb = p.xbc + (size_t)b * p.L * p.ldx;
    for (int s0 = s_begin; s0 < s_end; s0 += SBL) {
        const bool live = s0 + t16 < s_end;
        const int sstep = min(s0 + t16, s_end - 1);
        const int srow = p.reverse ? p.L - 1 - sstep : sstep;
        const bf16_t *row = xb + (size_t)srow * p.ldx;
        uint2 xr[4], Br[8];
        float4 gyr[EMIT ? 4 : 1];
#pragma unroll
        for (int ip = 0; ip < 4; ++ip) {
            xr[ip] = *reinterpret_cast<const uint2 *>(row + h * SP + 16 * ip + 4 * q);
            if (!live) xr[ip] = make_uint2(0u, 0u);              // padded step: x = 0, dt = 0, a = 1, gy = 0
            if constexpr (EMIT) {
                gyr[ip] = *reinterpret_cast<const float4 *>(p.gy + ((size_t)b * p.L + srow) * p.d_inner + h * SP + 16 * ip + 4 * q);
                if (!live) gyr[ip] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int jm = 0; jm < 8; ++jm) Br[jm] = *reinterpret_cast<const uint2 *>(row + p.d_inner + 16 * jm + 4 * q);
        const size_t sidx = ((size_t)b * p.L + srow) * p.H + h;
        const float dt_own = live ? p.dt[sidx] : 0.f;
        const float la_own = live ? p.la[sidx] : 0.f;
        float cum = la_own;
        cum += row_shr_zero<0x111>(cum);
        cum += row_shr_zero<0x112>(cum);
        cum += row_shr_zero<0x114>(cum);
        cum += row_shr_zero<0x118>(cum);
        __syncthreads();                                          // previous block's readers of the tables are done
        if (q == 0) { s_cum[t16] = cum; s_dt[t16] = dt_own; }
        __syncthreads();
        const float c15 = s_cum[15];
        const float4 cs4 = *reinterpret_cast<const float4 *>(&s_cum[4 * q]);
        const float4 ds4 = *reinterpret_cast<const float4 *>(&s_dt[4 * q]);
        const float cs[4] = {cs4.x, cs4.y, cs4.z, cs4.w}, ds[4] = {ds4.x, ds4.y, ds4.z, ds4.w};
        const float e15 = __expf(c15);

        u32x4 xT[4];                                             // lane (i, qq): x[s = 4 qq + g][p = 16 ip + i]
        transpose_pair(u32x4{xr[0].x, xr[0].y, xr[1].x, xr[1].y}, selA, selB, xT[0], xT[1]);
        transpose_pair(u32x4{xr[2].x, xr[2].y, xr[3].x, xr[3].y}, selA, selB, xT[2], xT[3]);

        if constexpr (EMIT) {
            u32x4 gh[2], gl[2];                                  // gy_t as a row operand over p, split
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const Bf16HiLo u0 = split_bf16_hilo(gyr[2 * kp].x, gyr[2 * kp].y), u1 = split_bf16_hilo(gyr[2 * kp].z, gyr[2 * kp].w);
                const Bf16HiLo u2 = split_bf16_hilo(gyr[2 * kp + 1].x, gyr[2 * kp + 1].y), u3 = split_bf16_hilo(gyr[2 * kp + 1].z, gyr[2 * kp + 1].w);
                gh[kp] = u32x4{u0.hi, u1.hi, u2.hi, u3.hi};
                gl[kp] = u32x4{u0.lo, u1.lo, u2.lo, u3.lo};
            }
            // (x gy^T)[s][t]: A rows = x_s (exact), B columns = gy_t, K = the 64 head channels
            f32x4 Gm = zero4;
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const u32x4 a = {xr[2 * kp].x, xr[2 * kp].y, xr[2 * kp + 1].x, xr[2 * kp + 1].y};
                Gm = mfma_bf16_packed(a, gh[kp], Gm);
                Gm = mfma_bf16_packed(a, gl[kp], Gm);
            }
            float Mv[4];                                          // this lane: t = t16, s = 4 q + g
#pragma unroll
            for (int g = 0; g < 4; ++g) Mv[g] = (4 * q + g <= t16) ? Gm[g] * __expf(cum - cs[g]) * ds[g] : 0.f;
            u32x4 Mh = {0u, 0u, 0u, 0u}, Ml = {0u, 0u, 0u, 0u};
            { const Bf16HiLo u = split_bf16_hilo(Mv[0], Mv[1]); Mh[0] = u.hi; Ml[0] = u.lo; }
            { const Bf16HiLo u = split_bf16_hilo(Mv[2], Mv[3]); Mh[1] = u.hi; Ml[1] = u.lo; }
#pragma unroll
            for (int jp = 0; jp < 8; jp += 2) {
                u32x4 BT[2];                                     // lane (i, qq): B[s = 4 qq + g][n = 16 jn + i], exact
                transpose_pair(u32x4{Br[jp].x, Br[jp].y, Br[jp + 1].x, Br[jp + 1].y}, selA, selB, BT[0], BT[1]);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int jn = jp + e;
                    f32x4 Y = zero4;
#pragma unroll
                    for (int kp = 0; kp < 2; ++kp) {
                        u32x4 sh, sl;
                        { const Bf16HiLo u = split_bf16_hilo(T[2 * kp][jn][0], T[2 * kp][jn][1]); sh[0] = u.hi; sl[0] = u.lo; }
                        { const Bf16HiLo u = split_bf16_hilo(T[2 * kp][jn][2], T[2 * kp][jn][3]); sh[1] = u.hi; sl[1] = u.lo; }
                        { const Bf16HiLo u = split_bf16_hilo(T[2 * kp + 1][jn][0], T[2 * kp + 1][jn][1]); sh[2] = u.hi; sl[2] = u.lo; }
                        { const Bf16HiLo u = split_bf16_hilo(T[2 * kp + 1][jn][2], T[2 * kp + 1][jn][3]); sh[3] = u.hi; sl[3] = u.lo; }
                        Y = mfma_bf16_packed(gh[kp], sh, Y);
                        Y = mfma_bf16_packed(gh[kp], sl, Y);
                        Y = mfma_bf16_packed(gl[kp], sh, Y);
                    }
#pragma unroll
                    for (int g = 0; g < 4; ++g) Y[g] *= __expf(cs[g]);   // rows of the C/D layout are t = 4 q + g
                    Y = mfma_bf16_packed(Mh, BT[e], Y);
                    Y = mfma_bf16_packed(Ml, BT[e], Y);
#pragma unroll
                    for (int g = 0; g < 4; ++g) s_o[4 * q + g][16 * jn + t16] = Y[g];
                }
            }
        } else {
            lsum += c15;
        }

        // ---- state: h^T <- e^{cum_15} h^T + sum_s x_s (e^{cum_15 - cum_s} dt_s B_s)^T ----------------------------------
        const float csc = __expf(c15 - cum) * dt_own;            // this lane's row s = t16
#pragma unroll
        for (int pr = 0; pr < 8; pr += 2) {
            const SSplit4 k0 = scale_split(Br[pr], csc), k1 = scale_split(Br[pr + 1], csc);
            const u32x4 kh = {k0.h0, k0.h1, k1.h0, k1.h1}, kl = {k0.l0, k0.l1, k1.l0, k1.l1};
            u32x4 ah0, ah1, al0, al1;
            transpose_pair(kh, selA, selB, ah0, ah1);
            transpose_pair(kl, selA, selB, al0, al1);
#pragma unroll
            for (int ip = 0; ip < 4; ++ip) {
                T[ip][pr] *= e15;
                T[ip][pr + 1] *= e15;
                T[ip][pr] = mfma_bf16_packed(xT[ip], ah0, T[ip][pr]);
                T[ip][pr + 1] = mfma_bf16_packed(xT[ip], ah1, T[ip][pr + 1]);
                T[ip][pr] = mfma_bf16_packed(xT[ip], al0, T[ip][pr]);
                T[ip][pr + 1] = mfma_bf16_packed(xT[ip], al1, T[ip][pr + 1]);
            }
        }

        if constexpr (EMIT) {
            __syncthreads();
            const int nvalid = min(SBL, s_end - s0);
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int tt = pass * 2 + (lane >> 5), col = (lane & 31) * 4;
                const int trow = p.reverse ? p.L - 1 - (s0 + tt) : s0 + tt;
                if (tt < nvalid)
                    *reinterpret_cast<float4 *>(p.pC + (((size_t)b * p.L + trow) * p.H + h) * SN + col) =
                        *reinterpret_cast<const float4 *>(&s_o[tt][col]);
            }
            if (p.g_la) {                                         // C_t . gC_t of this head (lane: step t16, channels 16 jm + 4 q + g)
                float acc = 0.f;
#pragma unroll
                for (int jm = 0; jm < 8; ++jm) {
                    const uint2 cr = *reinterpret_cast<const uint2 *>(row + p.d_inner + SN + 16 * jm + 4 * q);
                    acc += dot4(*reinterpret_cast<const float4 *>(&s_o[t16][16 * jm + 4 * q]), cr);
                }
                acc = sum_over_q(acc);
                if (q == 0 && live) p.dla[sidx] = acc;
            }
        }
    }

    if constexpr (!EMIT) {
        float *ws = p.ws_h + (seq * p.NC + c) * (size_t)(SN * SP);
#pragma unroll
        for (int ip = 0; ip < 4; ++ip)
#pragma unroll
            for (int jn = 0; jn < 8; ++jn)
#pragma unroll
                for (int g = 0; g < 4; ++g) ws[(16 * ip + 4 * q + g) * SN + 16 * jn + t16] = T[ip][jn][g];
        if (lane == 0) p.ws_hd[seq * p.NC + c] = __expf(lsum);
    }
}

// gy of this lane's step as a row operand over the head channels p, split (a padded step reads a valid row and gets zero)
__device__ __forceinline__ void load_gy_split(const float *gyrow, int q, bool live, u32x4 (&gh)[2], u32x4 (&gl)[2]) {
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
        float4 a = *reinterpret_cast<const float4 *>(gyrow + 32 * kp + 4 * q);
        float4 c = *reinterpret_cast<const float4 *>(gyrow + 32 * kp + 16 + 4 * q);
        if (!live) { a = make_float4(0.f, 0.f, 0.f, 0.f); c = a; }
        const Bf16HiLo u0 = split_bf16_hilo(a.x, a.y), u1 = split_bf16_hilo(a.z, a.w), u2 = split_bf16_hilo(c.x, c.y), u3 = split_bf16_hilo(c.z, c.w);
        gh[kp] = u32x4{u0.hi, u1.hi, u2.hi, u3.hi};
        gl[kp] = u32x4{u0.lo, u1.lo, u2.lo, u3.lo};
    }
}

// ---- G sweep: EMIT = false: chunk-local adjoint and decay (pass A); EMIT = true: g_x, g_dt, the head's g_B terms, B . gB ------
// State tiles S[jm][in] as the forward's: lane (i, qq), reg g <-> X[n = 16 jm + 4 qq + g][p = 16 in + i].
// EMIT keeps the block's B and C rows in LDS and reads gy twice: the 128 state registers leave room for one phase's operands,
// and the barriers between the phases keep the compiler from carrying a phase's loads through the next one.
template <bool EMIT>
__global__ __launch_bounds__(64, 2) void mamba2_ssd_bwd_g_kernel(const SsdBwdParams p) {
    const int c = blockIdx.x + p.c_off;
    const int b = blockIdx.y / p.H, h = blockIdx.y % p.H;
    const int lane = threadIdx.x, t16 = lane & 15, q = lane >> 4;
    __shared__ float s_cum[SBL], s_dt[SBL];
    __shared__ __attribute__((aligned(16))) float s_u[EMIT ? SBL : 1][SP + 4];    // gxu of the block
    __shared__ __attribute__((aligned(16))) float s_o[EMIT ? SBL : 1][SN + 4];    // gB of the block
    __shared__ __attribute__((aligned(16))) bf16_t s_b[EMIT ? SBL : 1][SN + 8], s_c[EMIT ? SBL : 1][SN + 8];   // B, C rows [step][n]
    __shared__ __attribute__((aligned(16))) bf16_t s_x[EMIT ? SBL : 1][SP + 8];                                // x rows [step][p]

    u32x4 selA, selB;
    sel_operands(t16, q, selA, selB);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    const size_t seq = (size_t)b * p.H + h;
    f32x4 S[8][4];
    {
        const float *src = (EMIT && p.NC > 1) ? p.ws_g + (seq * p.NC + c) * (size_t)(SN * SP) : nullptr;
#pragma unroll
        for (int jm = 0; jm < 8; ++jm)
#pragma unroll
            for (int in = 0; in < 4; ++in)
#pragma unroll
                for (int g = 0; g < 4; ++g) S[jm][in][g] = src ? src[(16 * jm + 4 * q + g) * SP + 16 * in + t16] : 0.f;
    }
    float lsum = 0.f;

    const int s_begin = c * p.Lc, s_end = min(p.L, s_begin + p.Lc);
    const bf16_t *xb = p.xbc + (size_t)b * p.L * p.ldx;
    for (int s0 = s_begin + (s_end - s_begin - 1) / SBL * SBL; s0 >= s_begin; s0 -= SBL) {
        const bool live = s0 + t16 < s_end;
        const int sstep = min(s0 + t16, s_end - 1);
        const int srow = p.reverse ? p.L - 1 - sstep : sstep;
        const bf16_t *row = xb + (size_t)srow * p.ldx;
        const float *gyrow = p.gy + ((size_t)b * p.L + srow) * p.d_inner + h * SP;
        uint2 Cr[8];
#pragma unroll
        for (int jm = 0; jm < 8; ++jm) Cr[jm] = *reinterpret_cast<const uint2 *>(row + p.d_inner + SN + 16 * jm + 4 * q);
        const size_t sidx = ((size_t)b * p.L + srow) * p.H + h;
        const float dt_own = live ? p.dt[sidx] : 0.f;
        const float la_own = live ? p.la[sidx] : 0.f;
        float cum = la_own;
        cum += row_shr_zero<0x111>(cum);
        cum += row_shr_zero<0x112>(cum);
        cum += row_shr_zero<0x114>(cum);
        cum += row_shr_zero<0x118>(cum);
        __syncthreads();                                          // previous block's readers of the tables are done
        if (q == 0) { s_cum[t16] = cum; s_dt[t16] = dt_own; }
        if constexpr (EMIT) {
#pragma unroll
            for (int jm = 0; jm < 8; ++jm) {
                *reinterpret_cast<uint2 *>(&s_c[t16][16 * jm + 4 * q]) = Cr[jm];
                *reinterpret_cast<uint2 *>(&s_b[t16][16 * jm + 4 * q]) = *reinterpret_cast<const uint2 *>(row + p.d_inner + 16 * jm + 4 * q);
            }
#pragma unroll
            for (int ip = 0; ip < 4; ++ip) {                      // padded step: x = 0, dt = 0, a = 1, gy = 0
                const uint2 xv = *reinterpret_cast<const uint2 *>(row + h * SP + 16 * ip + 4 * q);
                *reinterpret_cast<uint2 *>(&s_x[t16][16 * ip + 4 * q]) = live ? xv : make_uint2(0u, 0u);
            }
        }
        __syncthreads();
        const float c15 = s_cum[15];
        const float e15 = __expf(c15);
        // e^{cum_s - cum_t} for s >= t, else 0: this lane holds t = t16, s = 4 q + g of a [s][t] product
        auto decay_mask = [&](float (&d)[4]) {
            const float4 cs4 = *reinterpret_cast<const float4 *>(&s_cum[4 * q]);
            const float cs[4] = {cs4.x, cs4.y, cs4.z, cs4.w};
#pragma unroll
            for (int g = 0; g < 4; ++g) d[g] = (4 * q + g >= t16) ? __expf(cs[g] - cum) : 0.f;
        };
        // e^{cum_15 - cum_t} of the C/D layout's rows t = 4 q + g
        auto row_decay = [&](float (&er)[4]) {
            const float4 cs4 = *reinterpret_cast<const float4 *>(&s_cum[4 * q]);
            er[0] = __expf(c15 - cs4.x); er[1] = __expf(c15 - cs4.y); er[2] = __expf(c15 - cs4.z); er[3] = __expf(c15 - cs4.w);
        };
        // this lane's B / C row of the block (step t16, channels 16 jm + 4 q + g)
        auto rowB = [&](int jm) { return *reinterpret_cast<const uint2 *>(&s_b[EMIT ? t16 : 0][EMIT ? 16 * jm + 4 * q : 0]); };
        auto rowX = [&](int ip) { return *reinterpret_cast<const uint2 *>(&s_x[EMIT ? t16 : 0][EMIT ? 16 * ip + 4 * q : 0]); };
        auto rowC = [&](int jm) { return EMIT ? *reinterpret_cast<const uint2 *>(&s_c[EMIT ? t16 : 0][EMIT ? 16 * jm + 4 * q : 0]) : Cr[jm]; };

        f32x4 U[EMIT ? 4 : 1];
        if constexpr (EMIT) {
            u32x4 Vh = {0u, 0u, 0u, 0u}, Vl = {0u, 0u, 0u, 0u};
            {
                u32x4 gh[2], gl[2];
                load_gy_split(gyrow, q, live, gh, gl);
                f32x4 Vm = zero4;                                // (gy x^T)[s][t]
#pragma unroll
                for (int kp = 0; kp < 2; ++kp) {
                    const uint2 x0 = rowX(2 * kp), x1 = rowX(2 * kp + 1);
                    const u32x4 bq = {x0.x, x0.y, x1.x, x1.y};
                    Vm = mfma_bf16_packed(gh[kp], bq, Vm);
                    Vm = mfma_bf16_packed(gl[kp], bq, Vm);
                }
                float d[4];
                decay_mask(d);
                { const Bf16HiLo u = split_bf16_hilo(Vm[0] * d[0], Vm[1] * d[1]); Vh[0] = u.hi; Vl[0] = u.lo; }
                { const Bf16HiLo u = split_bf16_hilo(Vm[2] * d[2], Vm[3] * d[3]); Vh[1] = u.hi; Vl[1] = u.lo; }
            }
            float er[4];
            row_decay(er);
            __syncthreads();
            // ---- each state tile is split once and used twice: as it lies for B_t . X (-> gxu), transposed for X x_t (-> gB) ----
#pragma unroll
            for (int in = 0; in < 4; ++in) U[in] = zero4;
#pragma unroll
            for (int jp = 0; jp < 8; jp += 2) {
                const uint2 b0 = rowB(jp), b1 = rowB(jp + 1);
                const u32x4 aB = {b0.x, b0.y, b1.x, b1.y};
                f32x4 Z[2] = {zero4, zero4};                     // gB tiles jn = jp, jp + 1
#pragma unroll
                for (int kp = 0; kp < 2; ++kp) {
                    Bf16HiLo u[2][2][2];                             // [jn - jp][in - 2 kp][register pair]
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                        for (int ii = 0; ii < 2; ++ii) {
                            u[jj][ii][0] = split_bf16_hilo(S[jp + jj][2 * kp + ii][0], S[jp + jj][2 * kp + ii][1]);
                            u[jj][ii][1] = split_bf16_hilo(S[jp + jj][2 * kp + ii][2], S[jp + jj][2 * kp + ii][3]);
                        }
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii) {              // B_t . X: K = n over the tiles jp, jp + 1
                        const u32x4 sh = {u[0][ii][0].hi, u[0][ii][1].hi, u[1][ii][0].hi, u[1][ii][1].hi};
                        const u32x4 sl = {u[0][ii][0].lo, u[0][ii][1].lo, u[1][ii][0].lo, u[1][ii][1].lo};
                        U[2 * kp + ii] = mfma_bf16_packed(aB, sh, U[2 * kp + ii]);
                        U[2 * kp + ii] = mfma_bf16_packed(aB, sl, U[2 * kp + ii]);
                    }
                    const uint2 x0 = rowX(2 * kp), x1 = rowX(2 * kp + 1);
                    const u32x4 xa = {x0.x, x0.y, x1.x, x1.y};
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {              // X x_t: the tiles (jn, 2 kp), (jn, 2 kp + 1) transposed, K = p
                        const u32x4 sh = {u[jj][0][0].hi, u[jj][0][1].hi, u[jj][1][0].hi, u[jj][1][1].hi};
                        const u32x4 sl = {u[jj][0][0].lo, u[jj][0][1].lo, u[jj][1][0].lo, u[jj][1][1].lo};
                        const f32x4 h0 = mfma_bf16_packed(sh, selA, zero4), h1 = mfma_bf16_packed(sh, selB, zero4);
                        const f32x4 l0 = mfma_bf16_packed(sl, selA, zero4), l1 = mfma_bf16_packed(sl, selB, zero4);
                        const u32x4 bh = {pack_bf16_exact(h0[0], h0[1]), pack_bf16_exact(h0[2], h0[3]), pack_bf16_exact(h1[0], h1[1]), pack_bf16_exact(h1[2], h1[3])};
                        const u32x4 bl = {pack_bf16_exact(l0[0], l0[1]), pack_bf16_exact(l0[2], l0[3]), pack_bf16_exact(l1[0], l1[1]), pack_bf16_exact(l1[2], l1[3])};
                        Z[jj] = mfma_bf16_packed(xa, bh, Z[jj]);
                        Z[jj] = mfma_bf16_packed(xa, bl, Z[jj]);
                        __builtin_amdgcn_sched_barrier(0);        // (one tile group's operands at a time: the registers are full)
                    }
                }
                // gB_t = dt_t [ e^{cum_15 - cum_t} X x_t + sum_s V[s][t] C_s ]
                const uint2 c0 = rowC(jp), c1 = rowC(jp + 1);
                u32x4 CT[2];                                     // lane (i, qq): C[s = 4 qq + g][n = 16 jn + i], exact
                transpose_pair(u32x4{c0.x, c0.y, c1.x, c1.y}, selA, selB, CT[0], CT[1]);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) Z[jj][g] *= er[g];
                    Z[jj] = mfma_bf16_packed(Vh, CT[jj], Z[jj]);
                    Z[jj] = mfma_bf16_packed(Vl, CT[jj], Z[jj]);
#pragma unroll
                    for (int g = 0; g < 4; ++g) s_o[4 * q + g][16 * (jp + jj) + t16] = Z[jj][g] * s_dt[4 * q + g];
                }
            }
            __syncthreads();
        } else {
            lsum += c15;
        }

        u32x4 gTh[4], gTl[4];                                    // lane (i, qq): gy[s = 4 qq + g][p = 16 in + i], split
        {
            u32x4 gh[2], gl[2];
            load_gy_split(gyrow, q, live, gh, gl);
            transpose_pair(gh[0], selA, selB, gTh[0], gTh[1]);
            transpose_pair(gh[1], selA, selB, gTh[2], gTh[3]);
            transpose_pair(gl[0], selA, selB, gTl[0], gTl[1]);
            transpose_pair(gl[1], selA, selB, gTl[2], gTl[3]);
        }
        if constexpr (EMIT) {
            // gxu_t = e^{cum_15 - cum_t} B_t . X + sum_s W[s][t] gy_s,  W[s][t] = e^{cum_s - cum_t} (C_s . B_t), C B^T exact
            f32x4 Wm = zero4;
#pragma unroll
            for (int pr = 0; pr < 8; pr += 2) {
                const uint2 c0 = rowC(pr), c1 = rowC(pr + 1), b0 = rowB(pr), b1 = rowB(pr + 1);
                Wm = mfma_bf16_packed(u32x4{c0.x, c0.y, c1.x, c1.y}, u32x4{b0.x, b0.y, b1.x, b1.y}, Wm);
            }
            u32x4 Wh = {0u, 0u, 0u, 0u}, Wl = {0u, 0u, 0u, 0u};
            float d[4], er[4];
            decay_mask(d);
            row_decay(er);
            { const Bf16HiLo u = split_bf16_hilo(Wm[0] * d[0], Wm[1] * d[1]); Wh[0] = u.hi; Wl[0] = u.lo; }
            { const Bf16HiLo u = split_bf16_hilo(Wm[2] * d[2], Wm[3] * d[3]); Wh[1] = u.hi; Wl[1] = u.lo; }
#pragma unroll
            for (int in = 0; in < 4; ++in) {
#pragma unroll
                for (int g = 0; g < 4; ++g) U[in][g] *= er[g];
                U[in] = mfma_bf16_packed(Wh, gTh[in], U[in]);
                U[in] = mfma_bf16_packed(Wh, gTl[in], U[in]);
                U[in] = mfma_bf16_packed(Wl, gTh[in], U[in]);
#pragma unroll
                for (int g = 0; g < 4; ++g) s_u[4 * q + g][16 * in + t16] = U[in][g];
            }
        }

        // ---- state: X <- e^{cum_15} X + sum_s (e^{cum_s} C_s) gy_s^T -----------------------------------------------------
        const float csc = __expf(cum);                            // this lane's row s = t16
#pragma unroll
        for (int pr = 0; pr < 8; pr += 2) {
            const SSplit4 k0 = scale_split(rowC(pr), csc), k1 = scale_split(rowC(pr + 1), csc);
            const u32x4 kh = {k0.h0, k0.h1, k1.h0, k1.h1}, kl = {k0.l0, k0.l1, k1.l0, k1.l1};
            u32x4 ah0, ah1, al0, al1;
            transpose_pair(kh, selA, selB, ah0, ah1);
            transpose_pair(kl, selA, selB, al0, al1);
#pragma unroll
            for (int in = 0; in < 4; ++in) {
                S[pr][in] *= e15;
                S[pr + 1][in] *= e15;
                S[pr][in] = mfma_bf16_packed(ah0, gTh[in], S[pr][in]);
                S[pr + 1][in] = mfma_bf16_packed(ah1, gTh[in], S[pr + 1][in]);
                S[pr][in] = mfma_bf16_packed(ah0, gTl[in], S[pr][in]);
                S[pr + 1][in] = mfma_bf16_packed(ah1, gTl[in], S[pr + 1][in]);
                S[pr][in] = mfma_bf16_packed(al0, gTh[in], S[pr][in]);
                S[pr + 1][in] = mfma_bf16_packed(al1, gTh[in], S[pr + 1][in]);
            }
        }

        if constexpr (EMIT) {
            __syncthreads();
            const int nvalid = min(SBL, s_end - s0);
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {                // g_x = dt gxu, one rounding to bf16
                const int tt = pass * 4 + (lane >> 4), col = (lane & 15) * 4;
                const int trow = p.reverse ? p.L - 1 - (s0 + tt) : s0 + tt;
                if (tt < nvalid) {
                    const float4 v = *reinterpret_cast<const float4 *>(&s_u[tt][col]);
                    const float d = s_dt[tt];
                    *reinterpret_cast<uint2 *>(p.g_xbc + ((size_t)b * p.L + trow) * p.ldg + h * SP + col) =
                        make_uint2(pack_bf16_rne(v.x * d, v.y * d), pack_bf16_rne(v.z * d, v.w * d));
                }
            }
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int tt = pass * 2 + (lane >> 5), col = (lane & 31) * 4;
                const int trow = p.reverse ? p.L - 1 - (s0 + tt) : s0 + tt;
                if (tt < nvalid)
                    *reinterpret_cast<float4 *>(p.pB + (((size_t)b * p.L + trow) * p.H + h) * SN + col) =
                        *reinterpret_cast<const float4 *>(&s_o[tt][col]);
            }
            float gd = 0.f;                                       // g_dt_t = gxu_t . x_t (lane: step t16, channels 16 ip + 4 q + g)
#pragma unroll
            for (int ip = 0; ip < 4; ++ip) gd += dot4(*reinterpret_cast<const float4 *>(&s_u[t16][16 * ip + 4 * q]), rowX(ip));
            gd = sum_over_q(gd);
            if (q == 0 && live) p.g_dt[sidx] = gd;
            if (p.g_la) {                                         // (C . gC, left by the h sweep) - B_t . gB_t
                float acc = 0.f;
#pragma unroll
                for (int jm = 0; jm < 8; ++jm) acc += dot4(*reinterpret_cast<const float4 *>(&s_o[t16][16 * jm + 4 * q]), rowB(jm));
                acc = sum_over_q(acc);
                if (q == 0 && live) p.dla[sidx] -= acc;
            }
        }
    }

    if constexpr (!EMIT) {
        float *ws = p.ws_g + (seq * p.NC + c) * (size_t)(SN * SP);
#pragma unroll
        for (int jm = 0; jm < 8; ++jm)
#pragma unroll
            for (int in = 0; in < 4; ++in)
#pragma unroll
                for (int g = 0; g < 4; ++g) ws[(16 * jm + 4 * q + g) * SP + 16 * in + t16] = S[jm][in][g];
        if (lane == 0) p.ws_gd[seq * p.NC + c] = __expf(lsum);
    }
}

// pass B: exclusive scan of (decay, state) over the chunks of one (batch, head), in place: the states from chunk 0 upwards
// (the local end states of chunks 0 .. NC - 2 become the states entering chunks 0 .. NC - 1), the adjoints from chunk NC - 1
// downwards (the local adjoints of chunks NC - 1 .. 1 become the adjoints entering chunks NC - 1 .. 0 from the right).
__global__ __launch_bounds__(256) void mamba2_ssd_bwd_scan_kernel(const SsdBwdParams p) {
    const size_t seq = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;     // 0 .. 8191
    const bool adj = blockIdx.z != 0;
    float *ws = (adj ? p.ws_g : p.ws_h) + seq * p.NC * (size_t)(SN * SP) + e;
    const float *wd = (adj ? p.ws_gd : p.ws_hd) + seq * p.NC;
    float run = 0.f;
    for (int i = 0; i < p.NC - 1; ++i) {
        const int c = adj ? p.NC - 1 - i : i;
        const float loc = ws[(size_t)c * (SN * SP)];
        ws[(size_t)c * (SN * SP)] = run;
        run = fmaf(run, wd[c], loc);
    }
    ws[(size_t)(adj ? 0 : p.NC - 1) * (SN * SP)] = run;
}

// g_B, g_C = the heads' terms summed in head order, one rounding to bf16: a thread per (row, four columns of [g_B | g_C])
__global__ __launch_bounds__(256) void mamba2_ssd_bwd_reduce_kernel(const SsdBwdParams p) {
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);             // b * L + time index
    if (r >= (size_t)p.B * p.L) return;
    const int k = threadIdx.x & 63, col = (k & 31) * 4;
    const float *src = (k < 32 ? p.pB : p.pC) + r * p.H * SN + col;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int h = 0; h < p.H; ++h) {
        const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)h * SN);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<uint2 *>(p.g_xbc + r * p.ldg + p.d_inner + (k < 32 ? 0 : SN) + col) =
        make_uint2(pack_bf16_rne(acc.x, acc.y), pack_bf16_rne(acc.z, acc.w));
}

// g_la = suffix sum over the recurrence's steps of dla: one wave per (batch, head), 64 steps at a time from the last step
__global__ __launch_bounds__(64) void mamba2_ssd_bwd_gla_kernel(const SsdBwdParams p) {
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H, lane = threadIdx.x;
    float carry = 0.f;
    for (int base = 0; base < p.L; base += 64) {
        const int step = p.L - 1 - (base + lane);                             // lane 0 holds the latest step
        const int trow = p.reverse ? p.L - 1 - step : step;
        const size_t idx = ((size_t)b * p.L + trow) * p.H + h;
        float v = step >= 0 ? p.dla[idx] : 0.f;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float u = __shfl_up(v, d, 64);
            if (lane >= d) v += u;
        }
        if (step >= 0) p.g_la[idx] = carry + v;
        carry += __shfl(v, 63, 64);
    }
}

int bwd_chunk_len(int B, int L, int H, int chunk_len) {
    int Lc = chunk_len > 0 ? chunk_len : pafc_mamba2_scan_chunk_len(B, L, H);
    if (Lc < L) Lc = (Lc + 15) / 16 * 16;
    return Lc >= L ? L : Lc;
}

}  // namespace
}  // namespace pafc

extern "C" size_t pafc_mamba2_scan_bwd_workspace_bytes(int B, int L, int H, int chunk_len) {
    if (B <= 0 || L <= 0 || H <= 0) return 0;
    const int Lc = pafc::bwd_chunk_len(B, L, H, chunk_len);
    const size_t NC = (L + Lc - 1) / Lc, seqs = (size_t)B * H;
    size_t floats = seqs * L * (2 * pafc::SN + 1);                            // pB, pC, dla
    if (NC > 1) floats += 2 * seqs * NC * (pafc::SN * pafc::SP + 1);          // chunk states and decays, h and adjoint
    return sizeof(float) * floats;
}

extern "C" int pafc_mamba2_scan_backward(int B, int L, int H, const void *xbc, long ldx, const float *dt, const float *log_a,
                                         const float *gy, void *g_xbc, long ldg, float *g_dt, float *g_la, int reverse,
                                         int chunk_len, void *workspace, size_t workspace_bytes, pafc_stream_t stream) {
    using namespace pafc;
    if (!xbc || !dt || !log_a || !gy || !g_xbc || !g_dt) return PAFC_ERR_NULL_POINTER;
    if (B <= 0 || L <= 0 || H <= 0 || (long)B * H > 65535 || ldx < (long)H * 64 + 256 || (ldx % 4) || ldg < (long)H * 64 + 256 ||
        (ldg % 4))
        return PAFC_ERR_BAD_DIMS;
    if (((uintptr_t)xbc & 7) || ((uintptr_t)g_xbc & 7) || ((uintptr_t)gy & 15) || ((uintptr_t)workspace & 15)) return PAFC_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < pafc_mamba2_scan_bwd_workspace_bytes(B, L, H, chunk_len)) return PAFC_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    SsdBwdParams p{};
    p.xbc = (const bf16_t *)xbc; p.ldx = ldx; p.dt = dt; p.la = log_a; p.gy = gy;
    p.g_xbc = (bf16_t *)g_xbc; p.ldg = ldg; p.g_dt = g_dt; p.g_la = g_la;
    p.B = B; p.L = L; p.H = H; p.d_inner = H * 64; p.reverse = reverse ? 1 : 0;
    p.Lc = bwd_chunk_len(B, L, H, chunk_len);
    p.NC = (L + p.Lc - 1) / p.Lc;
    const size_t seqs = (size_t)B * H, tile = (size_t)SN * SP;
    float *w = (float *)workspace;
    if (p.NC > 1) {
        p.ws_h = w; w += seqs * p.NC * tile;
        p.ws_g = w; w += seqs * p.NC * tile;
    }
    p.pB = w; w += seqs * L * SN;
    p.pC = w; w += seqs * L * SN;
    p.dla = w; w += seqs * L;
    if (p.NC > 1) {
        p.ws_hd = w; w += seqs * p.NC;
        p.ws_gd = w;
        p.c_off = 0;
        hipLaunchKernelGGL((mamba2_ssd_bwd_h_kernel<false>), dim3(p.NC - 1, B * H), dim3(64), 0, s, p);
        p.c_off = 1;
        hipLaunchKernelGGL((mamba2_ssd_bwd_g_kernel<false>), dim3(p.NC - 1, B * H), dim3(64), 0, s, p);
        p.c_off = 0;
        hipLaunchKernelGGL(mamba2_ssd_bwd_scan_kernel, dim3(SN * SP / 256, B * H, 2), dim3(256), 0, s, p);
    }
    hipLaunchKernelGGL((mamba2_ssd_bwd_h_kernel<true>), dim3(p.NC, B * H), dim3(64), 0, s, p);
    hipLaunchKernelGGL((mamba2_ssd_bwd_g_kernel<true>), dim3(p.NC, B * H), dim3(64), 0, s, p);
    hipLaunchKernelGGL(mamba2_ssd_bwd_reduce_kernel, dim3((unsigned)((seqs / H * L + 3) / 4)), dim3(256), 0, s, p);
    if (g_la) hipLaunchKernelGGL(mamba2_ssd_bwd_gla_kernel, dim3(B * H), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
