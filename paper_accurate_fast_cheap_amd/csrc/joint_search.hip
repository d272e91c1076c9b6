// joint_search.hip -- the kernels of joint CTC/attention decoding, the time-synchronous beam search
// (include/pafc_joint_search.h).
//
// mha_step_paths_kernel: pafc_mha_step's body (mha_step_body.h), one wave per (row, head), with a per-row length and a
// per-row table of cache rows.
//
// candidates_kernel: one block per (frame, utterance): the C largest CTC log-probabilities by C passes of an arg-max over the
// elements that come after the previous winner in the order (value descending, index ascending), sorted by token.
//
// frame_kernel: one block of 256 per utterance.  The reference loops over (beam prefix, candidate) and accumulates into
// dictionaries; here every scored prefix of the frame is one ITEM owned by one lane, and its table entry is gathered, not
// accumulated.  Why that is the same: an entry (p_nb, p_b) of the frame's table receives
//   p_nb: the expansion of its parent (one parent, one token: once), and either the prefix's own repeat (it is on the beam
//         and its last token is a candidate) or the "considered before" term (it is not on the beam) -- never both;
//   p_b:  the prefix's own blank branch (on the beam) or the "considered before" term (not on the beam);
// so at most two terms meet in one log-add, which is symmetric and returns x for (-inf, x): no order of arrival exists.
// The only order that matters is the reference's loop order for the snapshots a new node takes of its parent's live (end frame,
// ctc confidence): the parent's live pair changes at most once within the frame, to (t + 1, max(old, p_ctc[last token])), at the
// earlier of (its own parent's expansion by its last token, its own repeat branch); a child is formed before or after that
// moment by its place in the loop, which the lane knows (see `sees_update`).
#include "pafc_joint_search.h"
#include "mha_step_body.h"

#include <math.h>

namespace pafc {
namespace {

constexpr int kMaxN = 16;
constexpr int kMaxC = 24;
constexpr int kItems = kMaxN * kMaxC;
constexpr double kNegInf = -__builtin_huge_val();
constexpr unsigned long long kEmpty = ~0ull;

__device__ __forceinline__ double logadd(double a, double b) {
    if (a == kNegInf && b == kNegInf) return kNegInf;
    const double m = a > b ? a : b;
    return m + log(exp(a - m) + exp(b - m));
}

// ---- self-attention through per-row paths ----

struct PathArgs {
    int R, H, rows, W;
    const void *qkv;
    long ldqkv;
    void *cache;
    const int32_t *path;
    long ldpath;
    const int32_t *length, *new_row, *need;
    void *out;
    long ldo;
};

template <typename ET> __global__ __launch_bounds__(kStepWaves * kWave) void mha_step_paths_kernel(PathArgs a) {
    const int r = blockIdx.x, lane = threadIdx.x & (kWave - 1);
    const int h = blockIdx.y * kStepWaves + (threadIdx.x >> 6);
    if (h >= a.H) return;                                              // (wave-uniform)
    const int p = min(max(a.length[r], 1), a.W + 1) - 1;                // keys [0, p]: p table entries and the row itself
    const long d = (long)a.H * kStepDk;
    const ET *qkv = static_cast<const ET *>(a.qkv) + (long)r * a.ldqkv;
    ET *cache = static_cast<ET *>(a.cache);
    const int32_t *path = a.path + (long)r * a.ldpath;
    const int nr = a.new_row[r], rows = a.rows;
    ET *slot = (a.need[r] != 0 && nr >= 0 && nr < rows) ? cache + (long)nr * 2 * d : nullptr;
    mha_step_row<ET>(qkv, cache, d, h, lane, p, slot, [=](int j) { return min(max(path[j], 0), rows - 1); },
                     static_cast<ET *>(a.out) + (long)r * a.ldo);
}

// ---- candidates ----

__device__ __forceinline__ bool after_f(float v, int i, float pv, int pi) { return v < pv || (v == pv && i > pi); }
__device__ __forceinline__ bool better_f(float v, int i, float bv, int bi) { return bi < 0 || v > bv || (v == bv && i < bi); }

template <typename ET>
__global__ __launch_bounds__(256) void candidates_kernel(int T, int V, int C, int blank, float log_threshold, const ET *ctc,
                                                         const int32_t *lens, int32_t *cand_tok, float *cand_p, float *p_blank,
                                                         int32_t *skip) {
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (t >= lens[b]) return;
    const ET *row = ctc + ((long)b * T + t) * V;
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float selv[kMaxC];
    __shared__ int seli[kMaxC];
    float pv = INFINITY;
    int pi = -1;
    for (int k = 0; k < C; ++k) {
        float bv = 0.f;
        int bi = -1;
        for (int v = tid; v < V; v += 256) {
            const float x = Elem<ET>::load(row + v);
            if ((k == 0 ? x == x : after_f(x, v, pv, pi)) && better_f(x, v, bv, bi)) {
                bv = x;
                bi = v;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, kWave);
            const int oi = __shfl_xor(bi, off, kWave);
            if (oi >= 0 && better_f(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            sv[tid >> 6] = bv;
            si[tid >> 6] = bi;
        }
        __syncthreads();
        bv = sv[0];
        bi = si[0];
        for (int w = 1; w < 4; ++w)
            if (si[w] >= 0 && better_f(sv[w], si[w], bv, bi)) {
                bv = sv[w];
                bi = si[w];
            }
        __syncthreads();
        if (tid == 0) {
            selv[k] = bv;
            seli[k] = bi;                                  // -1: fewer than C selectable values (NaNs)
        }
        if (bi < 0) {
            pv = -INFINITY;
            pi = V;                                        // nothing comes after this
        } else {
            pv = bv;
            pi = bi;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const long o = ((long)b * T + t) * C;
        skip[(long)b * T + t] = seli[0] == blank && selv[0] >= log_threshold;
        p_blank[(long)b * T + t] = Elem<ET>::load(row + blank);
        // ascending token order (missing entries, -1, last)
        for (int k = 1; k < C; ++k) {
            const int ti = seli[k];
            const float tv = selv[k];
            int j = k - 1;
            while (j >= 0 && (ti >= 0 && (seli[j] < 0 || seli[j] > ti))) {
                seli[j + 1] = seli[j];
                selv[j + 1] = selv[j];
                --j;
            }
            seli[j + 1] = ti;
            selv[j + 1] = tv;
        }
        for (int k = 0; k < C; ++k) {
            cand_tok[o + k] = seli[k];
            cand_p[o + k] = selv[k];
        }
    }
}

// ---- the frame ----

__device__ __forceinline__ unsigned hash_slot(unsigned long long key, int HS) {
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & (unsigned)(HS - 1);
}

__device__ __forceinline__ void lse_merge(double &m, double &s, double m2, double s2) {
    const double M = fmax(m, m2);
    const double x = (m == kNegInf) ? 0.0 : s * exp(m - M);
    const double y = (m2 == kNegInf) ? 0.0 : s2 * exp(m2 - M);
    m = M;
    s = x + y;
}

struct FrameArgs {
    pafc_joint_state st;
    int t, V, blank;
    const void *logits;
    long ldl;
    const int32_t *lens;
    double ctc_w, dec_w, bonus;
};

template <typename ET> __global__ __launch_bounds__(256) void frame_kernel(FrameArgs a) {
    const pafc_joint_state &st = a.st;
    const int b = blockIdx.x, tid = threadIdx.x, N = st.N, C = st.C, T = st.T, R = st.B * st.N, t = a.t;
    const long M = st.M;
    const int r0 = b * N;
    const bool use_dec = a.dec_w > 0.0;
    if (t >= a.lens[b] || st.skip[(long)b * T + t] != 0) {             // (block-uniform)
        if (tid < N) {
            const int r = r0 + tid;
            st.need[r] = 0;
            st.store_row[r] = (T + 1) * R;
            if (t < a.lens[b]) {
                st.trace_node[(long)t * R + r] = st.node[r];
                st.trace_score[(long)t * R + r] = st.score[r];
            }
        }
        if (tid == 0 && t < a.lens[b]) st.trace_exec[(long)t * st.B + b] = 0;
        return;
    }
    const int e = st.executed[b] + 1, cur = e & 1, prv = cur ^ 1;
    const int nl = min(max(st.nlive[b], 0), N);
    int32_t *parent = st.parent + b * M, *token = st.token + b * M, *length = st.length + b * M, *start = st.start + b * M,
            *end = st.end + b * M, *snap_end = st.snap_end + b * M, *row = st.row + b * M;
    float *ctc_conf = st.ctc_conf + b * M, *snap_ctc = st.snap_ctc_conf + b * M;
    double *att_conf = st.att_conf + b * M, *att_sum = st.att_sum + b * M, *lse = st.lse + b * M;
    double *nb_prev = st.p_nb + ((long)prv * st.B + b) * M, *b_prev = st.p_b + ((long)prv * st.B + b) * M;
    double *nb_cur = st.p_nb + ((long)cur * st.B + b) * M, *b_cur = st.p_b + ((long)cur * st.B + b) * M;
    const int32_t *stamp_prev = st.stamp + ((long)prv * st.B + b) * M;
    int32_t *stamp_cur = st.stamp + ((long)cur * st.B + b) * M;
    unsigned long long *hkey = st.hash_key + (long)b * st.HS;
    int32_t *hnode = st.hash_node + (long)b * st.HS;

    __shared__ int ctok[kMaxC];
    __shared__ float cp[kMaxC];
    __shared__ int blank_ci;
    __shared__ int hn[kMaxN], hlast[kMaxN], hlen[kMaxN], hpar[kMaxN], hrow[kMaxN], pj[kMaxN], lc[kMaxN], old_end[kMaxN];
    __shared__ float old_ctc[kMaxN];
    __shared__ double hnb[kMaxN], hb[kMaxN], htot[kMaxN], hatt[kMaxN], hlse[kMaxN];
    __shared__ int cid[kItems], isnew[kItems], ikey[kItems];
    __shared__ double isc[kItems];
    __shared__ int sel[kMaxN];
    __shared__ int nsel, n_nodes_s;
    __shared__ double dm[4], ds[4];

    const long co = ((long)b * T + t) * C;
    if (tid < C) {
        ctok[tid] = st.cand_tok[co + tid];
        cp[tid] = st.cand_p[co + tid];
    }
    if (tid < nl) {
        const int n = min(max(st.node[r0 + tid], 0), (int)M - 1);
        hn[tid] = n;
        hlast[tid] = token[n];
        hlen[tid] = length[n];
        hpar[tid] = parent[n];
        hrow[tid] = row[n];
        const bool ok = stamp_prev[n] == e - 1;                        // (a beam prefix was scored by the previous executed frame)
        hnb[tid] = ok ? nb_prev[n] : kNegInf;
        hb[tid] = ok ? b_prev[n] : kNegInf;
        htot[tid] = logadd(hnb[tid], hb[tid]);
        hatt[tid] = att_sum[n];
        old_end[tid] = end[n];
        old_ctc[tid] = ctc_conf[n];
    }
    if (tid == 0) n_nodes_s = st.n_nodes[b];
    __syncthreads();
    if (tid == 0) {
        int bc = -1;
        for (int c = 0; c < C; ++c)
            if (ctok[c] == a.blank) bc = c;
        blank_ci = bc;
    }
    if (tid < nl) {
        int p = -1, l = -1;
        for (int j = 0; j < nl; ++j)
            if (j != tid && hn[j] == hpar[tid]) p = j;
        for (int c = 0; c < C; ++c)                                    // ([sos] counts: the reference compares c with hyp[-1])
            if (ctok[c] == hlast[tid] && ctok[c] != a.blank) l = c;
        pj[tid] = p;
        lc[tid] = l;
    }
    // the logsumexp of every beam prefix's logits row, taken once per node
    for (int i = 0; i < nl; ++i) {
        if (!use_dec) break;
        const int n = min(max(st.node[r0 + i], 0), (int)M - 1);
        double v = lse[n];                                             // (block-uniform)
        if (v != v) {
            const ET *lrow = static_cast<const ET *>(a.logits) + (long)(r0 + i) * a.ldl;
            double m = kNegInf, s = 0.0;
            for (int x = tid; x < a.V; x += 256) {
                const double y = (double)Elem<ET>::load(lrow + x);
                if (y > m) {
                    s = s * exp(m - y) + 1.0;
                    m = y;
                } else if (y > kNegInf) {
                    s += exp(y - m);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) lse_merge(m, s, __shfl_xor(m, off, kWave), __shfl_xor(s, off, kWave));
            __syncthreads();                                           // (dm / ds of the previous row were read)
            if ((tid & 63) == 0) {
                dm[tid >> 6] = m;
                ds[tid >> 6] = s;
            }
            __syncthreads();
            m = dm[0];
            s = ds[0];
            for (int w = 1; w < 4; ++w) lse_merge(m, s, dm[w], ds[w]);
            v = m + log(s);
            __syncthreads();                                           // (every thread has read lse[n] before it changes)
            if (tid == 0) lse[n] = v;
        }
        if (tid == 0) hlse[i] = v;
    }
    __syncthreads();
    const int bci = blank_ci;
    const bool has_blank = bci >= 0;
    const float pblank = st.p_blank[(long)b * T + t];
    const int nitems = nl * C;

    // A: look every child up
    for (int k = tid; k < nitems; k += 256) {
        const int i = k / C, ci = k % C, c = ctok[ci];
        int found = -1;
        isnew[k] = 0;
        if (c < 0) {
            found = -2;                                                // no such candidate
        } else if (ci == bci) {
            found = hn[i];
        } else {
            const unsigned long long key = ((unsigned long long)(unsigned)hn[i] << 32) | (unsigned)c;
            unsigned s = hash_slot(key, st.HS);
            for (int probe = 0; probe < st.HS; ++probe) {
                const unsigned long long kk = hkey[s];
                if (kk == key) {
                    found = hnode[s];
                    break;
                }
                if (kk == kEmpty) break;
                s = (s + 1) & (unsigned)(st.HS - 1);
            }
        }
        cid[k] = found;
    }
    __syncthreads();
    // B: number the new nodes in the loop's order
    if (tid == 0) {
        int nn = n_nodes_s;
        for (int k = 0; k < nitems; ++k)
            if (cid[k] == -1) {
                if (nn < (int)M) {
                    cid[k] = nn++;
                    isnew[k] = 1;
                } else {
                    cid[k] = -2;                                       // (cannot happen: the pool holds N * C nodes per frame)
                }
            }
        n_nodes_s = nn;
    }
    __syncthreads();
    // C: one lane per item
    for (int k = tid; k < nitems; k += 256) {
        const int i = k / C, ci = k % C, c = ctok[ci], child = cid[k];
        double score = __builtin_nan("");
        int key = k;
        if (child >= 0 && ci == bci) {
            // the prefix itself, through the blank branch -- unless it is also the child of another beam prefix this frame:
            // then that pair's lane owns it
            if (!(pj[i] >= 0 && lc[i] >= 0)) {
                const double nb = lc[i] >= 0 ? (double)cp[lc[i]] + hnb[i] : kNegInf;
                const double bb = (double)pblank + htot[i];
                nb_cur[child] = nb;
                b_cur[child] = bb;
                stamp_cur[child] = e;
                if (lc[i] >= 0) {
                    end[child] = t + 1;
                    ctc_conf[child] = fmaxf(old_ctc[i], cp[lc[i]]);
                }
                score = a.ctc_w * logadd(nb, bb);
                if (hlen[i] > 1 && use_dec) score += hatt[i] * a.dec_w;
                score += a.bonus * (double)(hlen[i] - 1);
            }
        } else if (child >= 0) {
            const double pc = (double)cp[ci];
            const bool fresh = isnew[k] != 0;
            int j = -1;                                                // the child's slot if it is on the beam
            if (!fresh)
                for (int q = 0; q < nl; ++q)
                    if (hn[q] == child) j = q;
            if (fresh) {
                const unsigned long long hk = ((unsigned long long)(unsigned)hn[i] << 32) | (unsigned)c;
                unsigned s = hash_slot(hk, st.HS);
                for (int probe = 0; probe < st.HS; ++probe) {
                    const unsigned long long was = atomicCAS(&hkey[s], kEmpty, hk);
                    if (was == kEmpty || was == hk) {
                        hnode[s] = child;
                        break;
                    }
                    s = (s + 1) & (unsigned)(st.HS - 1);
                }
                parent[child] = hn[i];
                token[child] = c;
                length[child] = hlen[i] + 1;
                start[child] = t;
                end[child] = t + 1;
                ctc_conf[child] = cp[ci];
                // has the parent's live (end, ctc_conf) changed by the time the loop forms this child?
                const bool sees_update = lc[i] >= 0 && ((pj[i] >= 0 && pj[i] < i) || c > hlast[i]);
                snap_end[child] = sees_update ? t + 1 : old_end[i];
                snap_ctc[child] = sees_update ? fmaxf(old_ctc[i], cp[lc[i]]) : old_ctc[i];
            } else {
                end[child] = t + 1;
                ctc_conf[child] = fmaxf(j >= 0 ? old_ctc[j] : ctc_conf[child], cp[ci]);
            }
            double nb = pc + (c == hlast[i] ? hb[i] : htot[i]);
            double bb = kNegInf;
            if (j >= 0) {
                nb = logadd(nb, pc + hnb[j]);
                if (has_blank) {
                    bb = (double)pblank + htot[j];
                    key = min(k, j * C + bci);
                }
            } else if (!fresh && stamp_prev[child] == e - 1) {
                const double pnb = nb_prev[child], pb = b_prev[child];
                bb = (double)pblank + logadd(pnb, pb);
                nb = logadd(nb, pc + pnb);
            }
            nb_cur[child] = nb;
            b_cur[child] = bb;
            stamp_cur[child] = e;
            double att = 0.0;
            if (use_dec) {
                if (fresh) {
                    const ET *lrow = static_cast<const ET *>(a.logits) + (long)(r0 + i) * a.ldl;
                    const double step = (double)Elem<ET>::load(lrow + c) - hlse[i];
                    att = hatt[i] + step;
                    att_conf[child] = step;
                    att_sum[child] = att;
                } else {
                    att = att_sum[child];
                }
            }
            score = a.ctc_w * logadd(nb, bb);
            if (use_dec) score += att * a.dec_w;
            score += a.bonus * (double)hlen[i];
        }
        isc[k] = score;
        ikey[k] = key;
    }
    // beam prefixes that no item covers (no blank candidate, not a child of the beam) still enter the table through their
    // own repeat
    if (tid < nl && !has_blank && lc[tid] >= 0 && pj[tid] < 0) {
        const int n = hn[tid];
        nb_cur[n] = (double)cp[lc[tid]] + hnb[tid];
        b_cur[n] = kNegInf;
        stamp_cur[n] = e;
        end[n] = t + 1;
        ctc_conf[n] = fmaxf(old_ctc[tid], cp[lc[tid]]);
    }
    __syncthreads();
    // D: the N best items: score descending, the reference's listing order ascending; a NaN is never taken
    if (tid < kWave) {
        double pv = __builtin_huge_val();
        int pk = -1, cnt = 0;
        for (int s = 0; s < N; ++s) {
            double bv = 0.0;
            int bk = -1, bi = -1;
            for (int k = tid; k < nitems; k += kWave) {
                const double v = isc[k];
                const int kk = ikey[k];
                if (v != v) continue;
                if (s > 0 && !(v < pv || (v == pv && kk > pk))) continue;
                if (bi < 0 || v > bv || (v == bv && kk < bk)) {
                    bv = v;
                    bk = kk;
                    bi = k;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(bv, off, kWave);
                const int ok = __shfl_xor(bk, off, kWave), oi = __shfl_xor(bi, off, kWave);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && ok < bk))) {
                    bv = ov;
                    bk = ok;
                    bi = oi;
                }
            }
            if (bi < 0) break;                                         // (wave-uniform)
            if (tid == 0) sel[s] = bi;
            pv = bv;
            pk = bk;
            ++cnt;
        }
        if (tid == 0) nsel = cnt;
    }
    __syncthreads();
    // E: the new beam.  The paths first: column by column, every read of a round before its writes
    const int ns = nsel;
    int32_t *path = st.path + (long)r0 * (T + 1);
    {
        const int s = tid & 15, jj = tid >> 4;
        const bool live = s < ns;
        const int k = live ? sel[s] : 0, i = k / C;
        const bool is_child = live && (k % C) != bci;
        const int keep = live ? hlen[i] - 1 : 0;                       // entries of the source slot's path
        int maxlen = 0;
        for (int q = 0; q < nl; ++q) maxlen = max(maxlen, hlen[q]);
        for (int j0 = 0; j0 < maxlen; j0 += 16) {
            const int j = j0 + jj;
            int v = 0;
            bool w = false;
            if (live && j <= T) {
                if (j < keep) {
                    v = path[(long)i * (T + 1) + j];
                    w = true;
                } else if (j == keep && is_child) {
                    v = hrow[i];
                    w = true;
                }
            }
            __syncthreads();
            if (w) path[(long)s * (T + 1) + j] = v;
            __syncthreads();
        }
    }
    if (tid < N) {
        const int s = tid, r = r0 + s;
        int nd = -1, need = 0, tok = 0, len = 1, rw = 0, store = (T + 1) * R;
        double sc = 0.0;
        if (s < ns) {
            const int k = sel[s];
            nd = cid[k];
            sc = isc[k];
            tok = token[nd];
            len = length[nd];
            int have = row[nd];
            if (use_dec && have < 0 && t + 1 < a.lens[b]) {
                have = e * R + r;
                row[nd] = have;
                need = 1;
                store = have;
            }
            rw = have >= 0 ? have : 0;
        }
        st.node[r] = nd;
        st.need[r] = need;
        st.in_token[r] = tok;
        st.in_pos[r] = len - 1;
        st.in_len[r] = len;
        st.new_row[r] = need ? store : 0;
        st.store_row[r] = store;
        st.row_of_slot[r] = rw;
        st.score[r] = sc;
        st.trace_node[(long)t * R + r] = nd;
        st.trace_score[(long)t * R + r] = sc;
    }
    if (tid == 0) {
        st.executed[b] = e;
        st.nlive[b] = ns;
        st.n_nodes[b] = n_nodes_s;
        st.trace_exec[(long)t * st.B + b] = 1;
    }
    if (tid < N) {
        // decoder evaluations: one per slot that asks for one
        const int mine = st.need[r0 + tid];
        if (mine) atomicAdd(&st.evals[b], 1);
    }
}

__global__ __launch_bounds__(64) void collect_kernel(pafc_joint_state st, int32_t *out_len, int32_t *out_tok, int32_t *out_start,
                                                     int32_t *out_end, float *out_ctc, double *out_att) {
    const int r = blockIdx.x * 64 + threadIdx.x, R = st.B * st.N, W = st.T + 1;
    if (r >= R) return;
    const int b = r / st.N;
    const long M = st.M;
    const int nd = st.node[r];
    if (nd < 0 || nd >= M) {
        out_len[r] = -1;
        return;
    }
    const int32_t *parent = st.parent + b * M;
    const int len = min(max(st.length[b * M + nd] - 1, 0), W);
    out_len[r] = len;
    int n = nd, pos = len - 1;
    bool first = true;
    int c_end = 0;
    float c_ctc = 0.f;
    while (n > 0 && pos >= 0) {
        const long o = (long)r * W + pos, q = b * M + n;
        out_tok[o] = st.token[q];
        out_start[o] = st.start[q];
        out_end[o] = first ? st.end[q] : c_end;
        out_ctc[o] = first ? st.ctc_conf[q] : c_ctc;
        out_att[o] = st.att_conf[q];
        c_end = st.snap_end[q];
        c_ctc = st.snap_ctc_conf[q];
        first = false;
        n = parent[n];
        --pos;
    }
}

int state_check(const pafc_joint_state *s) {
    if (!s) return PAFC_ERR_NULL_POINTER;
    if (s->B <= 0 || s->N <= 0 || s->C <= 0 || s->T <= 0 || s->M <= 1 || s->HS <= 0 || (s->HS & (s->HS - 1)) ||
        (long)s->HS < 2 * (long)s->M)                                  // (the hash stays at most half full)
        return PAFC_ERR_BAD_DIMS;
    if (s->N > kMaxN || s->C > kMaxC) return PAFC_ERR_UNSUPPORTED;
    if ((long)s->M < 1 + (long)s->T * s->N * s->C || (long)(s->T + 2) * s->B * s->N > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    const void *ptrs[] = {s->parent, s->token, s->length, s->start, s->end, s->snap_end, s->ctc_conf, s->snap_ctc_conf,
                          s->att_conf, s->att_sum, s->lse, s->row, s->p_nb, s->p_b, s->stamp, s->hash_key, s->hash_node,
                          s->n_nodes, s->executed, s->nlive, s->evals, s->node, s->need, s->in_token, s->in_pos, s->in_len,
                          s->new_row, s->row_of_slot, s->store_row, s->score, s->path, s->cand_tok, s->cand_p, s->p_blank,
                          s->skip, s->trace_node, s->trace_score, s->trace_exec};
    for (const void *p : ptrs)
        if (!p) return PAFC_ERR_NULL_POINTER;
    return PAFC_OK;
}

}  // namespace
}  // namespace pafc

extern "C" int pafc_mha_step_paths(int dtype, int R, int H, int dk, int rows, int W, const void *qkv, long ldqkv, void *cache,
                                   const int32_t *path, long ldpath, const int32_t *length, const int32_t *new_row,
                                   const int32_t *need, void *out, long ldo, pafc_stream_t stream) {
    if (!qkv || !cache || !path || !length || !new_row || !need || !out) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (R <= 0 || H <= 0 || dk <= 0 || rows <= 0 || W <= 0 || ldpath < W || H > 65535 * pafc::kStepWaves) return PAFC_ERR_BAD_DIMS;
    if (dk != pafc::kStepDk) return PAFC_ERR_UNSUPPORTED;
    const long width = (long)H * dk, per16 = dtype == PAFC_F32 ? 4 : 8;
    if (ldqkv < 3 * width || ldo < width || ldqkv % per16 || ldo % per16) return PAFC_ERR_BAD_DIMS;
    if (((uintptr_t)qkv | (uintptr_t)cache | (uintptr_t)out) & 15) return PAFC_ERR_ALIGNMENT;
    pafc::PathArgs a{R, H, rows, W, qkv, ldqkv, cache, path, ldpath, length, new_row, need, out, ldo};
    const dim3 grid((unsigned)R, (unsigned)((H + pafc::kStepWaves - 1) / pafc::kStepWaves)), block(pafc::kStepWaves * pafc::kWave);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::mha_step_paths_kernel<float>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((pafc::mha_step_paths_kernel<pafc::bf16_t>), grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_joint_candidates(int dtype, int B, int T, int V, int C, int blank, float log_threshold, const void *ctc,
                                     const int32_t *lens, int32_t *cand_tok, float *cand_p, float *p_blank, int32_t *skip,
                                     pafc_stream_t stream) {
    if (!ctc || !lens || !cand_tok || !cand_p || !p_blank || !skip) return PAFC_ERR_NULL_POINTER;
    if (dtype != PAFC_F32 && dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (B <= 0 || T <= 0 || V <= 0 || C <= 0 || blank < 0 || blank >= V || B > 65535) return PAFC_ERR_BAD_DIMS;
    if (C > pafc::kMaxC || C > V) return PAFC_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)T, (unsigned)B), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::candidates_kernel<float>), grid, block, 0, s, T, V, C, blank, log_threshold, (const float *)ctc,
                           lens, cand_tok, cand_p, p_blank, skip);
    else
        hipLaunchKernelGGL((pafc::candidates_kernel<pafc::bf16_t>), grid, block, 0, s, T, V, C, blank, log_threshold,
                           (const pafc::bf16_t *)ctc, lens, cand_tok, cand_p, p_blank, skip);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_joint_frame(const pafc_joint_state *state, int t, int logits_dtype, int V, const void *logits, long ldl,
                                const int32_t *lens, const double *weights, int blank, pafc_stream_t stream) {
    const int rc = pafc::state_check(state);
    if (rc != PAFC_OK) return rc;
    if (!lens || !weights) return PAFC_ERR_NULL_POINTER;
    if (logits_dtype != PAFC_F32 && logits_dtype != PAFC_BF16) return PAFC_ERR_DTYPE;
    if (t < 0 || t >= state->T || V <= 0 || blank < 0 || blank >= V || state->C > V) return PAFC_ERR_BAD_DIMS;
    const double ctc_w = weights[0], dec_w = weights[1], bonus = weights[2];
    if (dec_w > 0.0 && (!logits || ldl < V)) return logits ? PAFC_ERR_BAD_DIMS : PAFC_ERR_NULL_POINTER;
    pafc::FrameArgs a{*state, t, V, blank, logits, ldl, lens, ctc_w, dec_w, bonus};
    hipStream_t s = (hipStream_t)stream;
    if (logits_dtype == PAFC_F32)
        hipLaunchKernelGGL((pafc::frame_kernel<float>), dim3((unsigned)state->B), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((pafc::frame_kernel<pafc::bf16_t>), dim3((unsigned)state->B), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

extern "C" int pafc_joint_collect(const pafc_joint_state *state, int32_t *out_len, int32_t *out_tok, int32_t *out_start,
                                  int32_t *out_end, float *out_ctc_conf, double *out_att_conf, pafc_stream_t stream) {
    const int rc = pafc::state_check(state);
    if (rc != PAFC_OK) return rc;
    if (!out_len || !out_tok || !out_start || !out_end || !out_ctc_conf || !out_att_conf) return PAFC_ERR_NULL_POINTER;
    const int R = state->B * state->N;
    hipLaunchKernelGGL(pafc::collect_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *state, out_len,
                       out_tok, out_start, out_end, out_ctc_conf, out_att_conf);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}
