// One frame of the CTC prefix beam search: the body of the frame loop of ctc_prefix_beam_kernel (ctc_beam.hip, which
// explains the slots, the tie order, TIMES and CTX) and of ctc_beam_stream_feed_kernel (ctc_beam_stream.hip).  The
// including scope provides the arrays of ctc_beam_lds.inc and
//   p (top_logp, top_idx, blank, g), b, lane, K, beam, UNTOUCHED, pparent / ptoken / tframe / tprev (the row's pools),
//   tin     the frame's index in this launch's top_logp / top_idx (B, p.T, K),
//   t       the frame's index since the start of the utterance: it numbers the new nodes (1 + t * beam + rank) and is
//           the frame that the frame lists record,
//   STREAM  constexpr bool: also carry each member's token count (c_len).
    const int nb = s_nb;
    if (lane < K) {
        tok[lane] = p.top_idx[((long)b * p.T + tin) * K + lane];
        lp[lane] = (double)p.top_logp[((long)b * p.T + tin) * K + lane];
    }
    __syncthreads();
    // rank of the blank token in the top-k (or -1)
    int rblank = -1;
    for (int r = 0; r < K; ++r) if (tok[r] == p.blank) rblank = r;

    // ---- S slots: lane m < nb gathers what lands on member m itself ---------------------------------------
    if (lane < nb) {
        const int m = lane;
        double s = NEG_INF, ns = NEG_INF;
        int order = UNTOUCHED;
        if (rblank >= 0) { s = c_sc[m] + lp[rblank]; order = min(order, (rblank * nb + m) * 2); }
        int rq = -1;                                            // rank of the member's own last token
        if (c_last[m] >= 0) for (int r = 0; r < K; ++r) if (tok[r] == c_last[m]) rq = r;
        if (rq >= 0 && c_last[m] != p.blank) {
            ns = c_ns[m] + lp[rq];                             // *uu -> *u
            order = min(order, (rq * nb + m) * 2);
            // the same prefix reached by extending its parent, if the parent is in the beam too
            for (int pb = 0; pb < nb; ++pb) {
                if (c_node[pb] == c_parent[m]) {
                    const bool rep = c_last[pb] == c_last[m];   // parent ends in the same token: only its blank path
                    ns = log_add2(ns, (rep ? c_s[pb] : c_sc[pb]) + lp[rq]);
                    order = min(order, (rq * nb + pb) * 2 + (rep ? 1 : 0));
                }
            }
        }
        s_s[m] = s; s_ns[m] = ns; s_order[m] = order; s_node[m] = c_node[m]; s_tok[m] = c_last[m]; s_par[m] = c_parent[m];
        if constexpr (TIMES) {
            // the contributions in the reference's loop order: 0 blank of m, 1 *uu -> *u of m, 2 *u-u -> *uu of
            // the parent, 3 extension of the parent
            int ko[3], kk[3], ks[3], nc = 0;
            if (rblank >= 0) { ko[nc] = (rblank * nb + m) * 2; kk[nc] = 0; ks[nc] = m; ++nc; }
            if (rq >= 0 && c_last[m] != p.blank) {
                ko[nc] = (rq * nb + m) * 2; kk[nc] = 1; ks[nc] = m; ++nc;
                for (int pb = 0; pb < nb; ++pb) {
                    if (c_node[pb] == c_parent[m]) {
                        const bool rep = c_last[pb] == c_last[m];
                        ko[nc] = (rq * nb + pb) * 2 + (rep ? 1 : 0); kk[nc] = rep ? 2 : 3; ks[nc] = pb; ++nc;
                    }
                }
            }
            for (int i = 1; i < nc; ++i)
                for (int j = i; j > 0 && ko[j - 1] > ko[j]; --j) {
                    int x = ko[j]; ko[j] = ko[j - 1]; ko[j - 1] = x;
                    x = kk[j]; kk[j] = kk[j - 1]; kk[j - 1] = x;
                    x = ks[j]; ks[j] = ks[j - 1]; ks[j - 1] = x;
                }
            double vs = NEG_INF, vns = NEG_INF, ctp = NEG_INF;
            int ts = 0, top = T_NONE, tbase = 0;
            for (int i = 0; i < nc; ++i) {
                const int q = ks[i];
                const bool sbest = c_vs[q] > c_vns[q];
                const double vit = sbest ? c_vs[q] : c_vns[q];
                const int qtimes = sbest ? c_ts[q] : c_tns[q];
                if (kk[i] == 0) {
                    vs = vit + lp[rblank]; ts = qtimes;
                } else if (kk[i] == 1) {
                    const double prob = lp[rq];
                    if (vns < c_vns[q] + prob && ctp < prob) { ctp = prob; top = T_REPLACE; tbase = c_tns[q]; }
                } else {
                    const double prob = lp[rq];
                    const double x = (kk[i] == 2 ? c_vs[q] : vit) + prob;
                    if (vns < x) { vns = x; ctp = prob; top = T_APPEND; tbase = kk[i] == 2 ? c_ts[q] : qtimes; }
                }
            }
            s_vs[m] = vs; s_vns[m] = vns; s_ts[m] = ts; s_top[m] = top; s_tbase[m] = tbase;
        }
        if constexpr (CTX) { s_ctx[m] = c_ctx[m]; s_cs[m] = c_cs[m]; }
    } else if (lane < BEAM_MAX) {
        s_order[lane] = UNTOUCHED;
    }
    // ---- E slots: (member m, token rank r) -> a new prefix, unless it already is a member ---------------
    for (int e = lane; e < BEAM_MAX * BEAM_MAX; e += 64) {
        const int m = e / BEAM_MAX, r = e % BEAM_MAX;
        int order = UNTOUCHED;
        double ns = NEG_INF;
        double vns = NEG_INF, cs = 0.0;
        int top = T_NONE, tbase = 0, cn = 0;
        if (m < nb && r < K && tok[r] != p.blank) {
            bool is_member = false;
            for (int qm = 0; qm < nb; ++qm) is_member |= (c_parent[qm] == c_node[m] && c_last[qm] == tok[r]);
            if (!is_member) {
                const bool rep = tok[r] == c_last[m];
                ns = (rep ? c_s[m] : c_sc[m]) + lp[r];
                order = (r * nb + m) * 2 + (rep ? 1 : 0);
                if constexpr (TIMES) {        // the slot's only contribution: v_ns and the frame list of the path
                    const bool sbest = c_vs[m] > c_vns[m];
                    const double x = (rep ? c_vs[m] : (sbest ? c_vs[m] : c_vns[m])) + lp[r];
                    vns = NEG_INF; top = T_NONE; tbase = 0;
                    if (NEG_INF < x) { vns = x; top = T_APPEND; tbase = (rep || sbest) ? c_ts[m] : c_tns[m]; }
                }
                if constexpr (CTX) { int nx; const double sc = ctx_step(p.g, c_ctx[m], tok[r], nx); cn = nx; cs = c_cs[m] + sc; }
            }
        }
        const int si = BEAM_MAX + e;
        if constexpr (TIMES) { s_vs[si] = NEG_INF; s_vns[si] = vns; s_ts[si] = 0; s_top[si] = top; s_tbase[si] = tbase; }
        if constexpr (CTX) { s_ctx[si] = cn; s_cs[si] = cs; }
        s_s[si] = NEG_INF; s_ns[si] = ns; s_order[si] = order; s_node[si] = -1;
        s_tok[si] = (r < K) ? tok[r] : -1; s_par[si] = (m < nb) ? c_node[m] : -1;
    }
    __syncthreads();
    for (int i = lane; i < NSLOT; i += 64) {
        if constexpr (CTX) {                // rank on score() + context_score, keep score() for the next frame
            const double ac = s_order[i] == UNTOUCHED ? NEG_INF : log_add2(s_s[i], s_ns[i]);
            s_ac[i] = ac;
            s_tot[i] = s_order[i] == UNTOUCHED ? NEG_INF : ac + s_cs[i];
        } else {
            s_tot[i] = s_order[i] == UNTOUCHED ? NEG_INF : log_add2(s_s[i], s_ns[i]);
        }
    }
    __syncthreads();
    // ---- rank the touched slots: score descending, first-touch order ascending -----------------------------
    for (int i = lane; i < NSLOT; i += 64) {
        if (s_order[i] == UNTOUCHED) continue;
        int rank = 0;
        const double sc = s_tot[i];
        const int oi = s_order[i];
        for (int j = 0; j < NSLOT; ++j) {
            if (s_order[j] == UNTOUCHED) continue;
            rank += (s_tot[j] > sc || (s_tot[j] == sc && s_order[j] < oi)) ? 1 : 0;
        }
        if (rank < beam) {
            int node = s_node[i];
            if (node < 0) {                                     // a new prefix: its node id is fixed by (t, rank)
                node = 1 + t * beam + rank;
                pparent[node] = s_par[i];
                ptoken[node] = s_tok[i];
            }
            n_node[rank] = node; n_last[rank] = s_tok[i]; n_parent[rank] = s_par[i];
            n_bs[rank] = s_s[i]; n_bns[rank] = s_ns[i]; n_bsc[rank] = CTX ? s_ac[i] : sc;
            if constexpr (TIMES) {
                int tns = 0;
                if (s_top[i] != T_NONE) {                      // a survivor materialises its pending frame list
                    tns = 1 + t * beam + rank;
                    tframe[tns] = t;
                    tprev[tns] = s_top[i] == T_APPEND ? s_tbase[i] : tprev[s_tbase[i]];
                }
                n_vs[rank] = s_vs[i]; n_vns[rank] = s_vns[i]; n_ts[rank] = s_ts[i]; n_tns[rank] = tns;
            }
            if constexpr (CTX) { n_ctx[rank] = s_ctx[i]; n_cs[rank] = s_cs[i]; }
            if constexpr (STREAM) n_len[rank] = i < BEAM_MAX ? c_len[i] : c_len[(i - BEAM_MAX) / BEAM_MAX] + 1;   // an E slot is a new prefix
        }
    }
    __syncthreads();
    if (lane == 0) {
        int cnt = 0;
        for (int i = 0; i < NSLOT; ++i) cnt += s_order[i] != UNTOUCHED;
        s_nb = min(cnt, beam);
    }
    __syncthreads();
    if (lane < s_nb) {
        c_node[lane] = n_node[lane]; c_last[lane] = n_last[lane]; c_parent[lane] = n_parent[lane];
        c_s[lane] = n_bs[lane]; c_ns[lane] = n_bns[lane]; c_sc[lane] = n_bsc[lane];
        if constexpr (TIMES) { c_vs[lane] = n_vs[lane]; c_vns[lane] = n_vns[lane]; c_ts[lane] = n_ts[lane]; c_tns[lane] = n_tns[lane]; }
        if constexpr (CTX) { c_ctx[lane] = n_ctx[lane]; c_cs[lane] = n_cs[lane]; }
        if constexpr (STREAM) c_len[lane] = n_len[lane];
    }
    __syncthreads();
