// What the offline CTC-fused RNN-T prefix beam search (rnnt_beam.hip) and the streaming one (rnnt_beam_stream.hip) share
// outside the kernel body, beyond beam_trie.h: the layout of the beam state.  The per-frame candidate walk itself is
// rnnt_beam_frame.inc; both step kernels include the same text, so their arithmetic cannot drift apart.
#ifndef PAFC_RNNT_BEAM_COMMON_H
#define PAFC_RNNT_BEAM_COMMON_H

#include "beam_trie.h"

namespace pafc {
namespace {

struct RnntState {
    int32_t *nb;                                   // (B) live beams
    int32_t *node, *parent, *last;                 // (B, beam)
    double *score;                                 // (B, beam)
    int32_t *pool_parent, *pool_token;             // (B, 1 + T * beam)
};

__host__ __device__ __forceinline__ RnntState carve(void *ws, int B, int T, int beam) {
    RnntState s;
    char *p = (char *)ws;
    s.score = (double *)p; p += sizeof(double) * (size_t)B * beam;
    s.nb = (int32_t *)p; p += sizeof(int32_t) * (size_t)((B + 1) & ~1);
    s.node = (int32_t *)p; p += sizeof(int32_t) * (size_t)B * beam;
    s.parent = (int32_t *)p; p += sizeof(int32_t) * (size_t)B * beam;
    s.last = (int32_t *)p; p += sizeof(int32_t) * (size_t)B * beam;
    s.pool_parent = (int32_t *)p; p += sizeof(int32_t) * (size_t)B * (1 + (size_t)T * beam);
    s.pool_token = (int32_t *)p;
    return s;
}

// bytes of the state carve() lays out
__host__ __device__ inline size_t rnnt_state_bytes(int B, int T, int beam) {
    return sizeof(double) * (size_t)B * beam + sizeof(int32_t) * ((size_t)((B + 1) & ~1) + 3 * (size_t)B * beam +
                                                                   2 * (size_t)B * (1 + (size_t)T * beam));
}

}  // namespace
}  // namespace pafc
#endif
