// LDS arrays of the CTC prefix beam search kernels (see ctc_beam_frame.inc); included inside the kernel body.
    __shared__ double c_s[BEAM_MAX], c_ns[BEAM_MAX], c_sc[BEAM_MAX];          // current beam: blank-ending, non-blank-ending, total
    __shared__ int c_node[BEAM_MAX], c_last[BEAM_MAX], c_parent[BEAM_MAX];
    __shared__ double s_s[NSLOT], s_ns[NSLOT], s_tot[NSLOT];
    __shared__ int s_order[NSLOT], s_node[NSLOT], s_tok[NSLOT], s_par[NSLOT];
    __shared__ int tok[BEAM_MAX];
    __shared__ double lp[BEAM_MAX];
    __shared__ int n_node[BEAM_MAX], n_last[BEAM_MAX], n_parent[BEAM_MAX];              // next beam staging
    __shared__ double n_bs[BEAM_MAX], n_bns[BEAM_MAX], n_bsc[BEAM_MAX];
    __shared__ int s_nb;
    // TIMES: viterbi scores and frame-list handles of the members / slots / next members
    __shared__ double c_vs[BEAM_MAX], c_vns[BEAM_MAX], s_vs[NSLOT], s_vns[NSLOT], n_vs[BEAM_MAX], n_vns[BEAM_MAX];
    __shared__ int c_ts[BEAM_MAX], c_tns[BEAM_MAX], s_ts[NSLOT], s_top[NSLOT], s_tbase[NSLOT], n_ts[BEAM_MAX], n_tns[BEAM_MAX];
    // CTX: context node and bonus; s_ac = the acoustic score of a slot (s_tot adds the bonus)
    __shared__ int c_ctx[BEAM_MAX], s_ctx[NSLOT], n_ctx[BEAM_MAX];
    __shared__ double c_cs[BEAM_MAX], s_cs[NSLOT], n_cs[BEAM_MAX], s_ac[NSLOT];
    __shared__ int c_len[BEAM_MAX], n_len[BEAM_MAX];                                // STREAM: token count of each member
