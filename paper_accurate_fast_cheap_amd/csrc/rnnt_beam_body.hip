// The frame body of the CTC-fused RNN-T prefix beam search on gfx950 (C ABI: include/pafc_search.h: pafc_rnnt_beam_body).
//
// One frame for the n = B x beam slots of a batch: what PrefixBeamSearch.forward_decoder_one_step, the shallow fusion and
// topk compute with framework ops, as L + 4 launches of two kernels.  The candidate walk (rnnt_beam.hip) and the state
// selection stay what they are; this file ends at top_val / top_idx.
//
//   gemm     out[s][o] = sum_k x_s[k] W[o][k] on the matrix cores, slots as the M side.  A wave multiplies 16-slot tiles by
//            16-column tiles (v_mfma_f32_16x16x4_f32 for fp32 weights: exact products, fp32 accumulation;
//            v_mfma_f32_16x16x32_bf16 for bf16), operands straight from global memory: lane (row = l & 15, q = l >> 4) reads
//            16 bytes (fp32) or 2 x 8 bytes (bf16) of its row per k-chunk, so the k order inside a chunk is the lane's, the
//            same for both operands.  The four waves of a block split the k-chunks (chunk c to wave c mod 4) and their
//            partial tiles are added through LDS in wave order.  Four epilogues:
//              lstm    a block owns 16 hidden units = 4 gate tiles (i, f, g, o) over two operands (x: the embedding row of
//                      last_tok or the layer below's new h; h: the slot's state), then the cell update in the lane that
//                      holds all four gates of (slot, unit); 32 slots per block
//              linear  projection: + bias, rounded to the weight type; 64 slots per block
//              act     pred_ffn: P = round(. + bias), then tanh(round(E[b, t] + P)) rounded -- the joint's input
//              logits  out_w: + bias, fp32, into the workspace (n x V floats, L2-sized)
//   topk     a block per slot: max and sum of exp over its logits row in a fixed order, lse, the fused score
//            f_v = log(w_rnnt exp(z_v - lse) + w_ctc exp(ctc[b, t, v])) written over z, then `beam` rounds of a block-wide
//            arg-max in (value descending, index ascending) order, each round taking the best entry AFTER the last taken one
//            in that order -- nothing is marked, ties go to the lowest index.
//   advance  *t_dev += 1 after the walk, so that a captured frame holds no framework op
// The frame index comes from the device (t_dev) when given, clamped to T - 1.  No atomics and no communication between
// workgroups of a launch: two calls give the same bits.
#include <math.h>

#include "pafc_common.h"
#include "rnnt_net.h"

namespace pafc {
namespace {

constexpr int kWaves = 4;          // waves per gemm block: they split the k-chunks
constexpr int kMaxSlots = 4096;    // B x beam
constexpr int kMaxBeam = 16;

enum { EPI_LSTM = 0, EPI_LINEAR = 1, EPI_ACT = 2, EPI_LOGITS = 3 };

// one k-chunk of a row as MFMA operand(s); a null row, or k beyond K, reads as zero (K is a multiple of 4)
template <typename WT> struct Frag;
template <> struct Frag<float> {
    static constexpr int kChunk = 16;           // lane group q holds k0 + 4 q + (0 .. 3): four k-steps of 16x16x4
    float v[4];
    __device__ __forceinline__ void load(const float *row, int k0, int q, int K) {
        const int kk = k0 + 4 * q;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row && kk < K) t = *reinterpret_cast<const float4 *>(row + kk);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ f32x4 mma(const Frag &a, const Frag &b, f32x4 c) {
#pragma unroll
        for (int g = 0; g < 4; ++g) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[g], b.v[g], c, 0, 0, 0);
        return c;
    }
};
template <> struct Frag<bf16_t> {
    static constexpr int kChunk = 32;           // lane group q holds k0 + 8 q + (0 .. 7): one k-step of 16x16x32
    u32x4 v;
    __device__ __forceinline__ void load(const bf16_t *row, int k0, int q, int K) {
        const int kk = k0 + 8 * q;
        uint2 lo = make_uint2(0u, 0u), hi = make_uint2(0u, 0u);
        if (row && kk < K) lo = *reinterpret_cast<const uint2 *>(row + kk);
        if (row && kk + 4 < K) hi = *reinterpret_cast<const uint2 *>(row + kk + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
    }
    static __device__ __forceinline__ f32x4 mma(const Frag &a, const Frag &b, f32x4 c) {
        return mfma_bf16_packed(a.v, b.v, c);
    }
};

__device__ __forceinline__ long frame_of(int t, const int64_t *t_dev, int T) {
    long tt = t_dev ? (long)*t_dev : (long)t;
    return tt < 0 ? 0 : tt > T - 1 ? T - 1 : tt;
}

template <typename WT> struct GemmArgs {
    int n, N;                      // slots; output columns (per gate)
    int K0, K1;                    // widths of the two operands (K1 = 0: one operand)
    const WT *x0, *x1;             // (n, K0) rows -- or, with tok, the table whose row tok[s] is slot s's -- and (n, K1)
    const int64_t *tok;
    int rows0;                     // rows of the table
    const WT *w0, *w1;             // (gates * N, K0), (gates * N, K1)
    const WT *b0, *b1;             // (gates * N) or null
    const WT *c;                   // lstm: (n, N) cell state in
    WT *h_out, *c_out;             // lstm: (n, N)
    WT *out;                       // linear / act: (n, N)
    float *z;                      // logits: (n, N)
    const WT *E;                   // act: (B, T, N)
    int T, beam, t;
    const int64_t *t_dev;
};

template <typename WT, int EPI>
__global__ __launch_bounds__(256) void body_gemm_kernel(const GemmArgs<WT> p) {
    constexpr int NG = EPI == EPI_LSTM ? 4 : 1;      // column tiles per block: the four gates of 16 hidden units, or one
    constexpr int MT = EPI == EPI_LSTM ? 2 : 4;      // slot tiles per block
    constexpr int CH = Frag<WT>::kChunk;
    __shared__ float red[kWaves][MT * NG][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const int o0 = blockIdx.x * 16, s0 = blockIdx.y * (MT * 16);

    const WT *xr0[MT], *xr1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int s = s0 + mt * 16 + r16;
        xr0[mt] = nullptr; xr1[mt] = nullptr;
        if (s < p.n) {
            long row = s;
            if (p.tok) {
                const long tk = (long)p.tok[s];
                row = tk < 0 ? 0 : tk > p.rows0 - 1 ? p.rows0 - 1 : tk;
            }
            xr0[mt] = p.x0 + row * p.K0;
            if (p.K1 > 0) xr1[mt] = p.x1 + (long)s * p.K1;
        }
    }
    const WT *wr0[NG], *wr1[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int o = o0 + r16;
        wr0[g] = nullptr; wr1[g] = nullptr;
        if (o < p.N) {
            wr0[g] = p.w0 + ((long)g * p.N + o) * p.K0;
            if (p.K1 > 0) wr1[g] = p.w1 + ((long)g * p.N + o) * p.K1;
        }
    }
    f32x4 acc[MT][NG];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[mt][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto sweep = [&](const WT *const *xr, const WT *const *wr, int K) {
        const int nc = (K + CH - 1) / CH;
        for (int ci = wave; ci < nc; ci += kWaves) {
            Frag<WT> a[MT], b[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) b[g].load(wr[g], ci * CH, q, K);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt].load(xr[mt], ci * CH, q, K);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if (s0 + mt * 16 < p.n) {            // (uniform over the block)
#pragma unroll
                    for (int g = 0; g < NG; ++g) acc[mt][g] = Frag<WT>::mma(a[mt], b[g], acc[mt][g]);
                }
            }
        }
    };
    sweep(xr0, wr0, p.K0);
    if (p.K1 > 0) sweep(xr1, wr1, p.K1);

#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][mt * NG + g][r][lane] = acc[mt][g][r];
    __syncthreads();

    // C layout of the 16x16 tiles: lane (column = l & 15, q = l >> 4), register r <-> slot 4 q + r.  Thread (wave w, lane)
    // finishes register r = w of its lane position for every slot tile, adding the waves' partials in wave order.
    const int o = o0 + r16;
    long tt = 0;
    if (EPI == EPI_ACT) tt = frame_of(p.t, p.t_dev, p.T);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int s = s0 + mt * 16 + 4 * q + wave;
        if (s >= p.n || o >= p.N) continue;
        float v[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float a = red[0][mt * NG + g][wave][lane];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) a += red[w][mt * NG + g][wave][lane];
            if (p.b0) a += Elem<WT>::load(p.b0 + (long)g * p.N + o);
            if (p.b1) a += Elem<WT>::load(p.b1 + (long)g * p.N + o);
            v[g] = a;
        }
        const long at = (long)s * p.N + o;
        if (EPI == EPI_LSTM) {
            const float c0 = Elem<WT>::load(p.c + at);
            const float c1 = sigm(v[NG > 1 ? 1 : 0]) * c0 + sigm(v[0]) * tanhf(v[NG > 2 ? 2 : 0]);
            const float h1 = sigm(v[NG > 3 ? 3 : 0]) * tanhf(c1);
            Elem<WT>::store(p.c_out + at, c1);
            Elem<WT>::store(p.h_out + at, h1);
        } else if (EPI == EPI_LINEAR) {
            Elem<WT>::store(p.out + at, v[0]);
        } else if (EPI == EPI_ACT) {
            const float P = Elem<WT>::round(v[0]);
            const float e = Elem<WT>::load(p.E + ((long)(s / p.beam) * p.T + tt) * p.N + o);
            const float a = Elem<WT>::round(e + P);
            Elem<WT>::store(p.out + at, tanhf(a));
        } else {
            p.z[at] = v[0];
        }
    }
}

// (value descending, index ascending): is (a, ia) before (b, ib)?
__device__ __forceinline__ bool before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

template <typename CT>
__global__ __launch_bounds__(256) void body_topk_kernel(float *z, int V, const CT *ctc, long ldc, int T, int beam, int t,
                                                         const int64_t *t_dev, float w_rnnt, float w_ctc, float *top_val,
                                                         int64_t *top_idx) {
    __shared__ float sv[kWaves];
    __shared__ int si[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    const long tt = frame_of(t, t_dev, T);
    float *zr = z + (long)s * V;
    const CT *cr = ctc + ((long)(s / beam) * T + tt) * ldc;

    float m = -INFINITY;
    for (int v = tid; v < V; v += 256) m = fmaxf(m, zr[v]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) sv[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
    __syncthreads();
    float sum = 0.f;
    for (int v = tid; v < V; v += 256) sum += expf(zr[v] - m);
    sum = wave_sum(sum);
    if (lane == 0) sv[wave] = sum;
    __syncthreads();
    const float lse = m + logf(((sv[0] + sv[1]) + sv[2]) + sv[3]);
    // a thread only ever re-reads the entries it wrote itself
    for (int v = tid; v < V; v += 256) zr[v] = logf(w_rnnt * expf(zr[v] - lse) + w_ctc * expf(Elem<CT>::load(cr + v)));

    float lv = INFINITY;          // the last entry taken: everything still to take lies after it
    int li = -1;
    for (int r = 0; r < beam; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;      // (none found: only when fewer than `beam` entries compare at all, i.e. NaN scores)
        for (int v = tid; v < V; v += 256) {
            const float f = zr[v];
            if (before(lv, li, f, v) && before(f, v, bv, bi)) { bv = f; bi = v; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        __syncthreads();          // the previous round's sv / si have been read
        if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (before(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        lv = bv; li = bi;
        if (tid == 0) {
            top_val[(long)s * beam + r] = bv;
            top_idx[(long)s * beam + r] = bi < V ? bi : 0;     // never an id outside the vocabulary
        }
    }
}

// the frame counter of a captured loop: *t_dev += 1
__global__ void body_advance_kernel(int64_t *t_dev) { t_dev[0] += 1; }

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

struct BodyWs { void *pred, *hj; float *z; };

BodyWs body_layout(void *ws, const pafc_rnnt_greedy_net *n, long slots, size_t *bytes) {
    const size_t el = n->dtype == PAFC_F32 ? 4 : 2;
    char *p = (char *)ws;
    size_t o = 0;
    auto take = [&](size_t b) { char *r = p ? p + o : nullptr; o += al256(b); return r; };
    BodyWs w;
    w.pred = take((size_t)slots * n->pred_dim * el);
    w.hj = take((size_t)slots * n->join_dim * el);
    w.z = (float *)take((size_t)slots * n->vocab * sizeof(float));
    *bytes = o;
    return w;
}

// beam / slot limits; the net's own are rnnt_check_net's
int body_dims(const pafc_rnnt_greedy_net *n, int B, int T, int beam) {
    if (B <= 0 || T <= 0 || beam <= 0) return PAFC_ERR_BAD_DIMS;
    if (beam > kMaxBeam || n->vocab < beam || (long)B * beam > kMaxSlots) return PAFC_ERR_UNSUPPORTED;
    return PAFC_OK;
}

template <typename WT, int EPI>
void launch_gemm(const GemmArgs<WT> &a, hipStream_t st) {
    constexpr int MT = EPI == EPI_LSTM ? 2 : 4;
    const dim3 grid((unsigned)((a.N + 15) / 16), (unsigned)((a.n + MT * 16 - 1) / (MT * 16)));
    hipLaunchKernelGGL((body_gemm_kernel<WT, EPI>), grid, dim3(256), 0, st, a);
}

template <typename WT>
void launch_body(const pafc_rnnt_greedy_net *net, int B, int T, int beam, int t, const int64_t *t_dev, const void *E, int ctc_dtype,
                 const void *ctc, long ldc, float w_rnnt, float w_ctc, const int64_t *last_tok, const void *h, const void *c,
                 void *h_new, void *c_new, float *top_val, int64_t *top_idx, const BodyWs &ws, hipStream_t st) {
    const int n = B * beam, L = net->num_layers, H = net->hidden;
    const long lay = (long)n * H;
    for (int l = 0; l < L; ++l) {
        GemmArgs<WT> a{};
        a.n = n; a.N = H; a.K1 = H;
        if (l == 0) { a.K0 = net->embed_dim; a.x0 = (const WT *)net->embed; a.tok = last_tok; a.rows0 = net->embed_rows; }
        else { a.K0 = H; a.x0 = (const WT *)h_new + (l - 1) * lay; }
        a.x1 = (const WT *)h + l * lay;
        a.w0 = (const WT *)net->w_ih[l]; a.w1 = (const WT *)net->w_hh[l];
        a.b0 = net->b_ih ? (const WT *)net->b_ih[l] : nullptr; a.b1 = net->b_hh ? (const WT *)net->b_hh[l] : nullptr;
        a.c = (const WT *)c + l * lay; a.h_out = (WT *)h_new + l * lay; a.c_out = (WT *)c_new + l * lay;
        launch_gemm<WT, EPI_LSTM>(a, st);
    }
    {
        GemmArgs<WT> a{};
        a.n = n; a.N = net->pred_dim; a.K0 = H; a.x0 = (const WT *)h_new + (L - 1) * lay;
        a.w0 = (const WT *)net->proj_w; a.b0 = (const WT *)net->proj_b; a.out = (WT *)ws.pred;
        launch_gemm<WT, EPI_LINEAR>(a, st);
    }
    {
        GemmArgs<WT> a{};
        a.n = n; a.N = net->join_dim; a.K0 = net->pred_dim; a.x0 = (const WT *)ws.pred;
        a.w0 = (const WT *)net->pred_ffn_w; a.b0 = (const WT *)net->pred_ffn_b; a.out = (WT *)ws.hj;
        a.E = (const WT *)E; a.T = T; a.beam = beam; a.t = t; a.t_dev = t_dev;
        launch_gemm<WT, EPI_ACT>(a, st);
    }
    {
        GemmArgs<WT> a{};
        a.n = n; a.N = net->vocab; a.K0 = net->join_dim; a.x0 = (const WT *)ws.hj;
        a.w0 = (const WT *)net->out_w; a.b0 = (const WT *)net->out_b; a.z = ws.z;
        launch_gemm<WT, EPI_LOGITS>(a, st);
    }
    if (ctc_dtype == PAFC_F32)
        hipLaunchKernelGGL(body_topk_kernel<float>, dim3((unsigned)n), dim3(256), 0, st, ws.z, net->vocab, (const float *)ctc, ldc, T,
                           beam, t, t_dev, w_rnnt, w_ctc, top_val, top_idx);
    else
        hipLaunchKernelGGL(body_topk_kernel<bf16_t>, dim3((unsigned)n), dim3(256), 0, st, ws.z, net->vocab, (const bf16_t *)ctc, ldc,
                           T, beam, t, t_dev, w_rnnt, w_ctc, top_val, top_idx);
}

}  // namespace
}  // namespace pafc

extern "C" {

size_t pafc_rnnt_beam_body_workspace_bytes(const pafc_rnnt_greedy_net *net, int B, int beam) {
    if (!net || (net->dtype != PAFC_F32 && net->dtype != PAFC_BF16)) return 0;
    if (net->num_layers <= 0 || net->embed_dim <= 0 || net->hidden <= 0 || net->pred_dim <= 0 || net->join_dim <= 0 || net->vocab <= 0)
        return 0;
    if (net->embed_dim % 4 || net->hidden % 4 || net->pred_dim % 4 || net->join_dim % 4 || net->join_dim > pafc::kRnntMaxJ) return 0;
    if (pafc::body_dims(net, B, 1, beam) != PAFC_OK) return 0;
    size_t bytes = 0;
    pafc::body_layout(nullptr, net, (long)B * beam, &bytes);
    return bytes;
}

int pafc_rnnt_beam_body(const pafc_rnnt_greedy_net *net, int B, int T, int beam, int t, const int64_t *t_dev, const void *E,
                        int ctc_dtype, const void *ctc, long ldc, float w_rnnt, float w_ctc, const int64_t *last_tok, const void *h,
                        const void *c, void *h_new, void *c_new, float *top_val, int64_t *top_idx, void *workspace,
                        size_t workspace_bytes, pafc_stream_t stream) {
    int rc = pafc::rnnt_check_net(net);
    if (rc != PAFC_OK) return rc;
    if (!E || !ctc || !last_tok || !h || !c || !h_new || !c_new || !top_val || !top_idx || !workspace) return PAFC_ERR_NULL_POINTER;
    rc = pafc::body_dims(net, B, T, beam);
    if (rc != PAFC_OK) return rc;
    if (ctc_dtype != PAFC_F32 && ctc_dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (ldc < net->vocab) return PAFC_ERR_BAD_DIMS;
    if (workspace_bytes < pafc_rnnt_beam_body_workspace_bytes(net, B, beam)) return PAFC_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 255) != 0 || !pafc::aligned16(h) || !pafc::aligned16(c) || !pafc::aligned16(h_new) ||
        !pafc::aligned16(c_new))
        return PAFC_ERR_ALIGNMENT;
    size_t bytes = 0;
    const pafc::BodyWs ws = pafc::body_layout(workspace, net, (long)B * beam, &bytes);
    hipStream_t st = (hipStream_t)stream;
    if (net->dtype == PAFC_F32)
        pafc::launch_body<float>(net, B, T, beam, t, t_dev, E, ctc_dtype, ctc, ldc, w_rnnt, w_ctc, last_tok, h, c, h_new, c_new, top_val,
                                 top_idx, ws, st);
    else
        pafc::launch_body<pafc::bf16_t>(net, B, T, beam, t, t_dev, E, ctc_dtype, ctc, ldc, w_rnnt, w_ctc, last_tok, h, c, h_new, c_new,
                                        top_val, top_idx, ws, st);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

int pafc_rnnt_beam_body_advance(int64_t *t_dev, pafc_stream_t stream) {
    if (!t_dev) return PAFC_ERR_NULL_POINTER;
    hipLaunchKernelGGL(pafc::body_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t_dev);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

}  // extern "C"
