// What the four prefix beam searches (ctc_beam.hip, ctc_beam_stream.hip, rnnt_beam.hip, rnnt_beam_stream.hip) share: the
// beam limit, the float64 log-add, the dimension check of their entry points and the walks over the hypothesis trie.
//
// A hypothesis is a node of a per-row trie kept as two int32 pools: parent[n] and token[n]; node 0 is the empty prefix.
// A frame list (the CTC search's token times) is the same shape: prev[n] and frame[n], node 0 the empty list.
#ifndef PAFC_BEAM_TRIE_H
#define PAFC_BEAM_TRIE_H

#include "pafc_common.h"
#include "../../include/pafc_search.h"

namespace pafc {
namespace {

constexpr int BEAM_MAX = 16;               // beam size and top-k limit
constexpr double NEG_INF = -__builtin_huge_val();

__device__ __forceinline__ double log_add2(double a, double b) {
    if (a == NEG_INF && b == NEG_INF) return NEG_INF;
    const double m = a > b ? a : b;
    return m + log(exp(a - m) + exp(b - m));
}

// B rows, node pools sized for T frames: a node index 1 + t * beam + rank must fit an int32
inline int beam_dims_check(int B, int T, int beam) {
    if (B <= 0 || T <= 0 || beam <= 0) return PAFC_ERR_BAD_DIMS;
    if (beam > BEAM_MAX || (long)T * beam >= 0x7fffffffL) return PAFC_ERR_UNSUPPORTED;
    return PAFC_OK;
}

// the frames a row takes of a chunk of Tmax
__device__ __forceinline__ int clamp_frames(int64_t nf, int Tmax) { return (int)(nf < 0 ? 0 : (nf > Tmax ? Tmax : nf)); }

// The list that ends in `head` along the chain n = prev[n] (until n <= 0), oldest entry first: counts it, then writes
// value[n] to its position in `out` wherever that position is below cap.  Returns the count.
__device__ __forceinline__ int trie_list_back(int head, const int32_t *prev, const int32_t *value, int32_t *out, int cap) {
    int cnt = 0;
    for (int n = head; n > 0; n = prev[n]) ++cnt;
    int pos = cnt;
    for (int n = head; n > 0; n = prev[n]) {
        --pos;
        if (pos < cap) out[pos] = value[n];
    }
    return cnt;
}

// The n-best of one row as if its stream ended here, called by one wave of 64: lane < nb (`active`) holds the member's
// trie node and its token count len.  Returns committed = the length of the longest common prefix of the members' token
// lists; every hypothesis of a later frame is a member or extends one, so those tokens never change again.  The same token
// list can own two trie nodes (it left the beam and was formed again), so the walk compares tokens, not node ids; two
// members on ONE node do agree below it, which ends the walk early.  It also stops at `from`, the count the caller already
// holds as final (clamped to the shortest member): all members agree below it.  The token copy stops at `from` too:
// out_tokens, the member's own row, receives tokens [from, from + ld).  Work and bytes follow the uncommitted tail, not the
// length of the stream.
__device__ __forceinline__ int trie_drain(bool active, int node, int len, int nb, const int32_t *pparent,
                                          const int32_t *ptoken, int from, int ld, int32_t *out_tokens) {
    int dmin = active ? len : 0x7fffffff;                         // the shortest member
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dmin = min(dmin, __shfl_xor(dmin, off, 64));
    if (nb == 0) dmin = 0;
    from = min(max(from, 0), dmin);

    // ---- committed: looked for in [from, dmin] ----------------------------------------------------------------------
    int n = node, d = active ? len : dmin;
    while (d > dmin) { n = pparent[n]; --d; }                     // every member at depth dmin
    int committed = dmin;
    while (d > from) {                                            // (d is wave-uniform from here on)
        const int n0 = __shfl(n, 0, 64);
        if (__all(!active || n == n0)) break;                     // one node: the lists agree below d
        const int tk = active ? ptoken[n] : -1;
        const int tk0 = __shfl(tk, 0, 64);
        if (!__all(!active || tk == tk0)) committed = d - 1;      // position d - 1 differs
        if (active) n = pparent[n];
        --d;
    }

    // ---- the member's tokens [from, from + ld) ------------------------------------------------------------------------
    if (active) {
        int m = node;
        for (int dd = len; dd > from; --dd) {
            const int pos = dd - 1 - from;
            if (pos < ld) out_tokens[pos] = ptoken[m];
            m = pparent[m];
        }
    }
    return committed;
}

}  // namespace
}  // namespace pafc
#endif
