// One frame of the CTC-fused RNN-T prefix beam search for one utterance: the text both step kernels include (rnnt_beam.hip
// offline, rnnt_beam_stream.hip chunk by chunk), so that they run the same arithmetic.  A block of 64 lanes per utterance.
// Reads, from the including kernel: s (RnntState), B, T (the frames the node pools are sized for), beam, blank, b, lane,
// base = b * beam, t (the frame that numbers new nodes: 1 + t * beam + rank; the caller keeps t < T), top_val / top_idx
// (B, beam, beam), next_idx / last_tok (B * beam).  Steps: candidates = float32(beam score) + log-prob; sorted descending,
// equal values in flat order; walked best first, equal hypotheses merged with log_add, stopped at `beam` distinct ones;
// the collected ones sorted stably by score; written back by rank.  Leaves in LDS for the includer: m_* (the beam before
// the frame), a_src / a_new / a_rank per collected hypothesis and cnt, their number.
    __shared__ float c_val[BEAM_MAX * BEAM_MAX];
    __shared__ int c_tok[BEAM_MAX * BEAM_MAX], c_order[BEAM_MAX * BEAM_MAX];
    __shared__ int m_node[BEAM_MAX], m_parent[BEAM_MAX], m_last[BEAM_MAX];
    __shared__ double m_score[BEAM_MAX];
    // collected hypotheses (beam_A of the reference), in first-seen order
    __shared__ double a_score[BEAM_MAX];
    __shared__ int a_node[BEAM_MAX], a_parent[BEAM_MAX], a_tok[BEAM_MAX], a_last[BEAM_MAX];
    __shared__ int a_src[BEAM_MAX], a_new[BEAM_MAX], a_rank[BEAM_MAX];
    __shared__ int a_count;

    const int nbm = s.nb[b];
    if (lane < beam) {
        m_node[lane] = s.node[base + lane]; m_parent[lane] = s.parent[base + lane]; m_last[lane] = s.last[base + lane];
        m_score[lane] = s.score[base + lane];
    }
    __syncthreads();
    const int ncand = nbm * beam;
    for (int c = lane; c < ncand; c += 64) {
        const int m = c / beam, k = c % beam;
        // float32(beam score) + float32 log-prob, added in float32 (prefix_beam_search.py:515-520)
        c_val[c] = (float)m_score[m] + top_val[((size_t)base + m) * beam + k];
        c_tok[c] = (int)top_idx[((size_t)base + m) * beam + k];
    }
    __syncthreads();
    for (int c = lane; c < ncand; c += 64) {        // descending by value; equal values keep their flat order
        const float v = c_val[c];
        int r = 0;
        for (int j = 0; j < ncand; ++j) r += (c_val[j] > v || (c_val[j] == v && j < c)) ? 1 : 0;
        c_order[r] = c;
    }
    __syncthreads();
    if (lane == 0) {
        int cnt = 0;
        for (int r = 0; r < ncand && cnt < beam; ++r) {
            const int c = c_order[r], m = c / beam, tk = c_tok[c];
            const double v = (double)c_val[c];
            int node = -1, par = -1, tok = -1, lastt;
            if (tk == blank) {
                node = m_node[m]; par = m_parent[m]; tok = m_last[m]; lastt = m_last[m];
            } else {
                par = m_node[m]; tok = tk; lastt = tk;
                for (int qm = 0; qm < nbm; ++qm)
                    if (m_parent[qm] == par && m_last[qm] == tk && m_node[qm] != 0) node = m_node[qm];   // already a member
            }
            int hit = -1;
            for (int e = 0; e < cnt; ++e) {
                const bool same = node >= 0 ? a_node[e] == node : (a_node[e] < 0 && a_parent[e] == par && a_tok[e] == tok);
                if (same) { hit = e; break; }
            }
            if (hit >= 0) {
                a_score[hit] = log_add2(a_score[hit], v);
            } else {
                a_score[cnt] = v; a_node[cnt] = node; a_parent[cnt] = par; a_tok[cnt] = tok; a_last[cnt] = lastt;
                a_src[cnt] = m; a_new[cnt] = tk != blank;
                ++cnt;
            }
        }
        a_count = cnt;
    }
    __syncthreads();
    const int cnt = a_count;
    if (lane < cnt) {                               // stable sort by score, descending (Python's list.sort, :556)
        int r = 0;
        for (int e = 0; e < cnt; ++e) r += (a_score[e] > a_score[lane] || (a_score[e] == a_score[lane] && e < lane)) ? 1 : 0;
        a_rank[lane] = r;
    }
    __syncthreads();
    const size_t pstride = 1 + (size_t)T * beam;
    if (lane < cnt) {
        const int p = a_rank[lane];
        int node = a_node[lane];
        if (node < 0) {
            node = 1 + t * beam + p;
            s.pool_parent[b * pstride + node] = a_parent[lane];
            s.pool_token[b * pstride + node] = a_tok[lane];
        }
        s.node[base + p] = node;
        s.parent[base + p] = a_node[lane] < 0 ? a_parent[lane] : (a_new[lane] ? a_parent[lane] : m_parent[a_src[lane]]);
        s.last[base + p] = a_last[lane];
        s.score[base + p] = a_score[lane];
        next_idx[base + p] = (int64_t)(base + a_src[lane]) + (a_new[lane] ? (int64_t)B * beam : 0);
        last_tok[base + p] = a_last[lane];
    } else if (lane < beam) {                       // unused slot: inert
        s.score[base + lane] = NEG_INF; s.node[base + lane] = 0; s.parent[base + lane] = -1; s.last[base + lane] = blank;
        next_idx[base + lane] = base + lane;
        last_tok[base + lane] = blank;
    }
    if (lane == 0) s.nb[b] = cnt;
