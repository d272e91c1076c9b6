// LDS arrays of the CTC prefix beam search kernels (see ctc_beam_frame.inc); included inside the kernel body.
    __shared__ double c_s[MAXB], c_ns[MAXB], c_sc[MAXB];          // current beam: blank-ending, non-blank-ending, total
    __shared__ int c_node[MAXB], c_last[MAXB], c_parent[MAXB];
    __shared__ double s_s[NSLOT], s_ns[NSLOT], s_tot[NSLOT];
    __shared__ int s_order[NSLOT], s_node[NSLOT], s_tok[NSLOT], s_par[NSLOT];
    __shared__ int tok[MAXB];
    __shared__ double lp[MAXB];
    __shared__ int n_node[MAXB], n_last[MAXB], n_parent[MAXB];              // next beam staging
    __shared__ double n_bs[MAXB], n_bns[MAXB], n_bsc[MAXB];
    __shared__ int s_nb;
    // TIMES: viterbi scores and frame-list handles of the members / slots / next members
    __shared__ double c_vs[MAXB], c_vns[MAXB], s_vs[NSLOT], s_vns[NSLOT], n_vs[MAXB], n_vns[MAXB];
    __shared__ int c_ts[MAXB], c_tns[MAXB], s_ts[NSLOT], s_top[NSLOT], s_tbase[NSLOT], n_ts[MAXB], n_tns[MAXB];
    // CTX: context node and bonus; s_ac = the acoustic score of a slot (s_tot adds the bonus)
    __shared__ int c_ctx[MAXB], s_ctx[NSLOT], n_ctx[MAXB];
    __shared__ double c_cs[MAXB], s_cs[NSLOT], n_cs[MAXB], s_ac[NSLOT];
    __shared__ int c_len[MAXB], n_len[MAXB];                                // STREAM: token count of each member
