"""Transducer container around the accelerated encoder (reference: wenet/transducer/transducer.py): encoder + CTC +
RNN predictor + joint, `decode(methods=[...,'rnnt_beam_search', 'rnnt_greedy_search'])` (:695-813), `beam_search_decode`
(:644-693), `greedy_search` (:427-472), the runtime step API (:474-505) and `stream_greedy_search` /
`stream_beam_search`: the streaming encoder and the greedy / CTC-fused prefix beam search chunk by chunk with carried
decoder state.  Two-pass decoding (transducer_attention_rescoring, :288-425): `score_hypotheses` is the full-sum transducer
score log p(y | x) of n-best lists (`_cal_transducer_score`, :185-210), and the decode modes "ctc_beam_td_rescoring" /
"rnnt_beam_td_rescoring" re-rank a first pass with it (search/rescoring.py); with an attention decoder attached
(`attention_decoder=`, held as `self.decoder`) "attention_rescoring", "ctc_beam_td_attn_rescoring" and
"rnnt_beam_attn_rescoring" add the attention term of ASRModel.score_attention (transformer/attn_rescore.py).

Training objective (forward, :105-175): transducer_weight * RNN-T loss + ctc_weight * CTC loss over the accelerated
encoder.  The reference's RNN-T loss is the third-party `optimized_transducer.transducer_loss` (transducer.py:506-523;
Rev fork, unpinned): restated from the published definition in `loss.py` -- PARITY UNPINNED.  Its attention decoder was
not released (decoder.py is swallowed by .gitignore:44): the decoder here is the published WeNet one (transformer/decoder.py),
used by the second pass and, when it is built trainable (init_model: args.train_attention_decoder), by the attention term of
the objective, attention_decoder_weight * loss_att (transformer/attn_train.py)."""
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ..transformer.asr_model import ASRModel
from ..transformer.search import DecodeResult
from .loss import transducer_loss
from .search.greedy_search import GreedyStreamer, batch_greedy_search
from .search.prefix_beam_search import BeamStreamer, PrefixBeamSearch
from ..transformer.attn_rescore import ATTN_RESCORING_MODES, attention_rescore
from .search.rescoring import RESCORING_MODES, build_arc_tables, check_hypotheses, check_score_backend, rescore

IGNORE_ID = -1
FUSED_JOINT = "fused_joint"


def add_blank(ys_pad: torch.Tensor, blank: int, ignore_id: int) -> torch.Tensor:
    """wenet/utils/common.py:78-107: prepend <blank>, padding (ignore_id) -> blank: (B, L) -> (B, L + 1)."""
    bs = ys_pad.size(0)
    _blank = torch.full((bs, 1), blank, dtype=ys_pad.dtype, device=ys_pad.device)
    out = torch.cat([_blank, ys_pad], dim=1)
    return torch.where(out == ignore_id, blank, out)


class Transducer(ASRModel):
    def __init__(self, vocab_size: int, blank: int, encoder: torch.nn.Module, predictor: torch.nn.Module,
                 joint: torch.nn.Module, ctc=None, special_tokens: Optional[dict] = None, attention_decoder=None,
                 ctc_weight: float = 0.0, transducer_weight: float = 1.0, attention_weight: float = 0.0,
                 transducer_type: Optional[str] = None, reverse_weight: float = 0.0, lsm_weight: float = 0.0,
                 length_normalized_loss: bool = False, **_unused_model_conf):
        super().__init__(vocab_size, encoder, ctc, ctc_weight, special_tokens, decoder=attention_decoder,
                         reverse_weight=reverse_weight, lsm_weight=lsm_weight, length_normalized_loss=length_normalized_loss)
        # model_conf.transducer_type (the reference's key, default "optimized_transducer"): every value but "fused_joint" keeps the
        # restated path below; "fused_joint" asks for the fused joint + loss kernels (hip_ops.rnnt_joint_loss) and never falls back
        self.fused_joint = transducer_type == FUSED_JOINT
        self.blank = blank
        self.predictor = predictor
        self.joint = joint
        self.transducer_weight = transducer_weight
        self.attention_decoder_weight = attention_weight
        self.bs: Optional[PrefixBeamSearch] = None

    def forward(self, batch: dict, device: torch.device) -> Dict[str, Optional[torch.Tensor]]:
        """transducer.py:105-175: encoder -> RNN-T loss (+ ctc_weight * CTC) (+ attention_decoder_weight * attention loss when
        the model has an attention decoder with trainable parameters and that weight is not 0)."""
        speech = batch["feats"].to(device)
        speech_lengths = batch["feats_lengths"].to(device)
        text = batch["target"].to(device)
        text_lengths = batch["target_lengths"].to(device)
        assert speech.shape[0] == speech_lengths.shape[0] == text.shape[0] == text_lengths.shape[0]
        encoder_out, encoder_mask = self.encoder(speech, speech_lengths)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        loss_rnnt = self._compute_loss(encoder_out, encoder_out_lens, text, text_lengths)
        loss = self.transducer_weight * loss_rnnt
        loss_ctc = None
        if self.ctc_weight != 0.0 and self.ctc is not None:
            loss_ctc = self.ctc.loss(encoder_out.float(), encoder_out_lens, text, text_lengths)
            loss = loss + self.ctc_weight * loss_ctc.sum()
        loss_att, acc_att = None, -1.0
        if self.attention_decoder_weight != 0.0 and self._trains_attention():
            loss_att, acc_att = self._calc_att_loss(encoder_out, encoder_mask, text, batch["target_lengths"])
            loss = loss + self.attention_decoder_weight * loss_att.sum()
        return {"loss": loss, "loss_att": loss_att, "loss_ctc": loss_ctc, "loss_rnnt": loss_rnnt, "th_accuracy": acc_att}

    def _compute_loss(self, encoder_out, encoder_out_lens, text, text_lengths) -> torch.Tensor:
        """transducer.py:525-561 (optimized_transducer branch): predictor over blank-prepended targets, joint on the
        valid lattices only, loss with reduction "mean"."""
        ys_in_pad = add_blank(text, self.blank, IGNORE_ID)
        predictor_out = self.predictor(ys_in_pad)
        rnnt_text = torch.where(text == IGNORE_ID, 0, text.to(torch.int64)).to(torch.int32)
        if self.fused_joint:
            return self._fused_joint_loss(encoder_out, encoder_out_lens, predictor_out, rnnt_text, text_lengths)
        joint_out = self.joint.forward_optimized(encoder_out.to(predictor_out.dtype), predictor_out,
                                                 encoder_out_lens.to(torch.int32), text_lengths.to(torch.int32))
        return transducer_loss(joint_out, rnnt_text, encoder_out_lens, text_lengths, self.blank, reduction="mean",
                               from_log_softmax=False)

    def _fused_joint_loss(self, encoder_out, encoder_out_lens, predictor_out, rnnt_text, text_lengths) -> torch.Tensor:
        """transducer_type "fused_joint": the same "mean" (sum_n nll_n / sum_n T_n) from E = enc_ffn(encoder_out) over the padded
        (B, T) and P = pred_ffn(predictor_out), without the joint's (rows, V) output (hip_ops.rnnt_joint_loss)."""
        from .. import hip_ops
        from .._lib import PafcError
        j = self.joint
        unmet = self._joint_unmet_for_kernels()
        E = P = None
        if unmet is None:
            E = j.enc_ffn(encoder_out.to(predictor_out.dtype))
            P = j.pred_ffn(predictor_out)
            unmet = hip_ops.rnnt_joint_loss_unmet(E, P, j.ffn_out.weight)
        if unmet is not None:
            raise PafcError(f"transducer_type {FUSED_JOINT!r}: {unmet}")
        nll = hip_ops.rnnt_joint_loss(E, P, j.ffn_out.weight, j.ffn_out.bias, encoder_out_lens, rnnt_text, text_lengths,
                                      self.blank)
        return nll.sum() / encoder_out_lens.sum()

    def _joint_unmet_for_kernels(self) -> Optional[str]:
        """The condition of the joint the fused kernels do not take (pre-join projections, no post-join, tanh, no hat_joint)."""
        j = self.joint
        if not getattr(j, "prejoin_linear", False) or j.enc_ffn is None or j.pred_ffn is None:
            return "the joint has no pre-join projections (prejoin_linear: false)"
        if j.postjoin_linear:
            return "the joint has a post-join projection (postjoin_linear: true)"
        if not isinstance(j.activatoin, torch.nn.Tanh):
            return "the joint's activation is not tanh"
        if getattr(j, "hat_joint", False):
            return "hat_joint"
        return None

    @torch.no_grad()
    def score_hypotheses(self, encoder_out: torch.Tensor, encoder_lens, hyps: List[List[List[int]]],
                         backend: Optional[str] = None) -> List[List[float]]:
        """The full-sum transducer score log p(y | x) of every hypothesis: hyps[b] is a list of token lists for utterance b of
        encoder_out (B, T, D); the result has the same shape.  encoder_lens: (B) tensor or list; lengths on the host spare
        the kernels backend one read of the device.
        backend "framework": `_cal_transducer_score` restated (transducer.py:185-210): the encoder rows repeated per hypothesis,
          predictor(add_blank(...)), joint, transducer_loss(reduction="none") times -1; on the CPU and the GPU.
        backend "kernels": the prefix trie of every n-best list through hip_ops.rnnt_score_hypotheses -- enc_ffn once per
          utterance, the predictor teacher-forced once over the padded hypotheses (the reference's own call), one joint row per
          (frame, trie arc) instead of one per (hypothesis, frame, label count), no logits stored.  It scores with the bf16 joint,
          the training kernel's contract, also for an fp32 model.  It needs the joint _fused_joint_loss takes (pre-join
          projections, no post-join projection, tanh, no hat_joint); an unmet condition raises PafcError, never a fallback.
        None: kernels on the GPU, framework on the CPU.
        ValueError for a blank inside a hypothesis, a token outside the vocabulary or more than 2558 tokens."""
        backend = check_score_backend(backend, encoder_out.is_cuda)
        lens = [int(v) for v in (encoder_lens.tolist() if isinstance(encoder_lens, torch.Tensor) else encoder_lens)]
        if len(hyps) != encoder_out.size(0) or len(lens) != encoder_out.size(0):
            raise ValueError(f"{encoder_out.size(0)} utterances, {len(hyps)} n-best lists, {len(lens)} lengths")
        flat = [h for nbest in hyps for h in nbest]
        if backend == "framework":
            check_hypotheses(hyps, self.vocab_size, self.blank)
            td = self._score_framework(encoder_out, lens, hyps) if flat else []
        else:
            td = self._score_kernels(encoder_out, encoder_lens, lens, hyps) if flat else []
        out, at = [], 0
        for nbest in hyps:
            out.append(td[at:at + len(nbest)])
            at += len(nbest)
        return out

    def _hyps_pad(self, flat: List[List[int]], device) -> torch.Tensor:
        umax = max(len(h) for h in flat)
        pad = torch.full((len(flat), umax), IGNORE_ID, dtype=torch.int64)
        for n, h in enumerate(flat):
            pad[n, :len(h)] = torch.tensor(h, dtype=torch.int64)
        return pad.to(device, non_blocking=True)

    def _score_framework(self, encoder_out, lens: List[int], hyps) -> List[float]:
        td: List[float] = []
        for b, nbest in enumerate(hyps):              # one utterance at a time: its hypotheses are the reference's batch
            if not nbest:
                continue
            hyps_pad = self._hyps_pad(nbest, encoder_out.device)
            predictor_out = self.predictor(add_blank(hyps_pad, self.blank, IGNORE_ID))
            enc = encoder_out[b:b + 1, :lens[b]].to(predictor_out.dtype).repeat(len(nbest), 1, 1)
            joint_out = self.joint(enc, predictor_out)                                   # (m, T_b, U + 1, V)
            us = [len(h) for h in nbest]
            logits = torch.cat([joint_out[i, :, :u + 1].reshape(-1, joint_out.size(-1)) for i, u in enumerate(us)])
            rnnt_text = torch.where(hyps_pad == IGNORE_ID, 0, hyps_pad).to(torch.int32)
            nll = transducer_loss(logits, rnnt_text, torch.tensor([lens[b]] * len(nbest)), torch.tensor(us), self.blank,
                                  reduction="none")
            td += (nll * -1).tolist()
        return td

    def _score_kernels(self, encoder_out, encoder_lens, lens: List[int], hyps) -> List[float]:
        from .. import hip_ops
        from .._lib import PafcError
        j = self.joint
        unmet = self._joint_unmet_for_kernels()
        if unmet is None and not encoder_out.is_cuda:
            unmet = "the operands are not on the GPU"
        if unmet is not None:
            raise PafcError(f"score_hypotheses(backend='kernels'): {unmet}")
        tables = build_arc_tables(hyps, lens, self.vocab_size, self.blank)
        flat = [h for nbest in hyps for h in nbest]
        predictor_out = self.predictor(add_blank(self._hyps_pad(flat, encoder_out.device), self.blank, IGNORE_ID))
        E = j.enc_ffn(encoder_out.to(predictor_out.dtype))
        P = j.pred_ffn(predictor_out)                                                    # (N, Umax + 1, J): tables.pred_stride
        unmet = hip_ops.rnnt_score_unmet(E, P, j.ffn_out.weight)
        if unmet is not None:
            raise PafcError(f"score_hypotheses(backend='kernels'): {unmet}")
        hl = encoder_lens if isinstance(encoder_lens, torch.Tensor) and encoder_lens.is_cuda else None
        score = hip_ops.rnnt_score_hypotheses(E, P, j.ffn_out.weight, j.ffn_out.bias, hl, tables, self.blank)
        return score.tolist()                                                            # the one read of the device

    def init_bs(self):
        if self.bs is None:
            self.bs = PrefixBeamSearch(self.encoder, self.predictor, self.joint, self.ctc, self.blank)

    def beam_search_decode(self, encoder_outs, encoder_lens, ctc_probs, decoding_chunk_size: int = -1,
                           beam_size: int = 5, num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                           ctc_weight: float = 0.3, transducer_weight: float = 0.7, cat_embs=None,
                           frame_body: Optional[str] = None) -> List[DecodeResult]:
        """frame_body: None (the PrefixBeamSearch's own, "framework" by default) or "framework" / "kernels" for this call: the
        per-frame body of the device-resident search as framework ops or as the library's kernels (never a fallback)."""
        self.init_bs()
        return self.bs.prefix_beam_search_decode(encoder_outs, encoder_lens, ctc_probs, decoding_chunk_size, beam_size,
                                                 num_decoding_left_chunks, simulate_streaming, ctc_weight,
                                                 transducer_weight, cat_embs, frame_body)

    @torch.no_grad()
    def greedy_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                      num_decoding_left_chunks: int = -1, simulate_streaming: bool = False, n_steps: int = 64
                      ) -> List[List[int]]:
        """transducer.py:427-472 for B >= 1 (the reference asserts B = 1): the encoder, then the greedy search of every
        utterance (search/greedy_search.py: on the GPU the lockstep kernels, on the CPU the reference's loop).
        simulate_streaming is ignored, as in the reference."""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        encoder_out, encoder_mask = self._forward_encoder(speech, speech_lengths, decoding_chunk_size,
                                                          num_decoding_left_chunks)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        return [r.tokens for r in batch_greedy_search(self, encoder_out, encoder_out_lens, n_steps)]

    @torch.no_grad()
    def stream_greedy_search(self, speech: torch.Tensor, decoding_chunk_size: int, n_steps: int = 64,
                             on_tokens: Optional[Callable[[int, List[List[int]]], None]] = None) -> List[DecodeResult]:
        """Streaming greedy search of B equal-length streams (B, T, F): the window walk of ASRModel._stream_windows (the
        encoder with carried state, drained after the last window) and each window's output frames into one
        GreedyStreamer.  on_tokens(window_index, new_tokens_per_row) is called after every window.  Returns per stream the tokens, their absolute frames and the path score.  Over the stream the
        decisions equal batch_greedy_search of the concatenated encoder outputs of the same steps."""
        windows = self._stream_windows(speech, decoding_chunk_size, "stream_greedy_search")
        streamer = GreedyStreamer(self, speech.size(0), decoding_chunk_size, n_steps)
        for i, y in windows:
            new: List[List[int]] = [[] for _ in range(speech.size(0))]
            for a in range(0, y.size(1), decoding_chunk_size):      # (the final drain of the look-ahead emits more frames)
                for b, tk in enumerate(streamer.feed(y[:, a:a + decoding_chunk_size])):
                    new[b] += tk
            if on_tokens is not None:
                on_tokens(i, new)
        return streamer.results()

    @torch.no_grad()
    def stream_beam_search(self, speech: torch.Tensor, decoding_chunk_size: int, beam_size: int = 10, ctc_weight: float = 0.3,
                           transducer_weight: float = 0.7, blank_penalty: float = 0.0,
                           on_partial: Optional[Callable[[int, List[DecodeResult], List[List[int]]], None]] = None,
                           max_total_frames: Optional[int] = None, frame_body: Optional[str] = None) -> List[DecodeResult]:
        """Streaming CTC-fused RNN-T prefix beam search of B equal-length streams (B, T, F): the window walk of
        ASRModel._stream_windows, each window's frames and their ctc_logprobs into one BeamStreamer.
        on_partial(window_index, partial_results, committed_tokens_per_row) is called once per window.  Returns per stream
        the n-best DecodeResult.  Over the stream the result equals the offline rnnt_beam_search of the concatenated encoder
        outputs of the same steps.  max_total_frames (default: what the speech can produce) sizes the trie pools.
        frame_body: BeamStreamer's ("framework" / "kernels"; None: the default)."""
        windows = self._stream_windows(speech, decoding_chunk_size, "stream_beam_search")
        if max_total_frames is None:
            max_total_frames = speech.size(1) // self.encoder.embed.subsampling_rate + decoding_chunk_size
        streamer = BeamStreamer(self, speech.size(0), decoding_chunk_size, beam_size, ctc_weight, transducer_weight,
                                max_total_frames, frame_body=frame_body)
        for i, y in windows:
            partial = None                                      # (a window may come without output frames)
            for a in range(0, y.size(1), decoding_chunk_size):      # (the final drain of the look-ahead emits more frames)
                yc = y[:, a:a + decoding_chunk_size]
                partial = streamer.feed(yc, self.ctc_logprobs(yc, blank_penalty, self.blank))
            if on_partial is not None:
                on_partial(i, partial if partial is not None else streamer.partials(), [list(c) for c in streamer.committed])
        return streamer.results()

    # ---- the reference's runtime step API (transducer.py:474-505), for runtimes that drive their own loop ----
    def forward_encoder_chunk(self, xs: torch.Tensor, offset: int, required_cache_size: int,
                              att_cache: torch.Tensor = torch.zeros(0, 0, 0, 0), cnn_cache: torch.Tensor = torch.zeros(0, 0, 0, 0)
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.encoder.forward_chunk(xs, offset, required_cache_size, att_cache, cnn_cache)

    def forward_predictor_step(self, xs: torch.Tensor, cache: List[torch.Tensor]) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """B = 1: the reference's fake (1, 1) padding, in the predictor's dtype (bf16 models)."""
        assert len(cache) == 2
        padding = torch.zeros(1, 1, dtype=self.predictor.embed.weight.dtype, device=xs.device)
        return self.predictor.forward_step(xs, padding, cache)

    def forward_joint_step(self, enc_out: torch.Tensor, pred_out: torch.Tensor) -> torch.Tensor:
        return self.joint(enc_out, pred_out)

    def forward_predictor_init_state(self) -> List[torch.Tensor]:
        """The zero state of one stream, on the predictor's device and in its dtype."""
        w = self.predictor.embed.weight
        return [c.to(w.dtype) for c in self.predictor.init_state(1, device=w.device)]

    @torch.no_grad()
    def decode(self, methods: List[str], speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int = 10,
               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0,
               transducer_weight: float = 0.0, simulate_streaming: bool = False, reverse_weight: float = 0.0,
               context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0, cat_embs=None,
               frame_body: Optional[str] = None, attn_weight: float = 0.0, search_ctc_weight: float = 0.3,
               search_transducer_weight: float = 0.7, score_backend: Optional[str] = None, length_penalty: float = 0.0,
               **_ignored) -> Dict[str, List[DecodeResult]]:
        """frame_body: for rnnt_beam_search and rnnt_beam_td_rescoring, the per-frame body of beam_search_decode ("framework" /
        "kernels").
        Two-pass modes with the attention term (a model with an attention decoder; NotImplementedError without one):
          "attention_rescoring": first pass ctc_prefix_beam_search, final_i = attn_i + ctc_weight * first_pass_score_i;
          "ctc_beam_td_attn_rescoring" / "rnnt_beam_attn_rescoring": the first passes of the two modes below,
            final_i = attn_weight * attn_i + ctc_weight * first_pass_score_i + transducer_weight * td_i (transducer.py:401-420);
          attn_i = score_attention's l2r_i, or (1 - reverse_weight) * l2r_i + reverse_weight * r2l_i; results as
          attn_rescore.attention_rescore builds them (nbest_attn_scores, confidence, tokens_confidence).
        "attention_beam_search" (likewise a model with an attention decoder): the decoder's own autoregressive beam search with
          length_penalty (attn_search.attention_beam_search, backend: score_backend); the reference's spelling "attention" is
          still refused.
        "joint_decoding" (likewise): the time-synchronous joint CTC/attention beam search (joint_search.joint_decoding) with
          ctc_weight, beam_size and length_bonus = length_penalty; backend: score_backend; cat_embs must be None for it.
        Two-pass modes without it (a non-zero reverse_weight or attn_weight with them is a ValueError):
          "ctc_beam_td_rescoring": first pass ctc_prefix_beam_search (computed once when that mode is requested too);
          "rnnt_beam_td_rescoring": first pass beam_search_decode with search_ctc_weight / search_transducer_weight -- the
            reference's names, but beam_search_decode's defaults 0.3 / 0.7: the reference's 1.0 / 0.0 switch the transducer off.
        Second pass: final_i = ctc_weight * first_pass_score_i + transducer_weight * td_i, td_i = score_hypotheses (backend:
        score_backend), ties to the earlier first-pass rank; nbest / nbest_scores / nbest_times re-ordered by final,
        nbest_td_scores the raw td_i (search/rescoring.py: rescore)."""
        td_only = [m for m in methods if m in RESCORING_MODES]
        if td_only and (reverse_weight != 0.0 or attn_weight != 0.0):
            raise ValueError(f"decode mode {td_only[0]!r} with reverse_weight = {reverse_weight} / attn_weight = {attn_weight}: "
                             "the attention decoder was not released with the reference, so this mode has no attention term to "
                             "weigh; ctc_beam_td_attn_rescoring / rnnt_beam_attn_rescoring of a model built with an attention "
                             "decoder have one")
        with_attn = [m for m in methods if m in ATTN_RESCORING_MODES + ("attention_beam_search", "joint_decoding")]
        if with_attn and self.decoder is None:
            raise NotImplementedError(f"decode mode {with_attn[0]!r} needs an attention decoder (init_model builds one with "
                                      "args.attention_decoder)")
        two_pass = [m for m in methods if m in RESCORING_MODES + ATTN_RESCORING_MODES]
        rest = [m for m in methods if m not in ("rnnt_beam_search", "rnnt_greedy_search") + RESCORING_MODES + ATTN_RESCORING_MODES]
        encoder_out, encoder_mask = self._forward_encoder(speech, speech_lengths, decoding_chunk_size,
                                                          num_decoding_left_chunks, simulate_streaming, cat_embs)
        encoder_lens = encoder_mask.squeeze(1).sum(1)
        ctc_probs = self.ctc_logprobs(encoder_out, blank_penalty, blank_id)
        results = {}
        ctc_first = ("ctc_beam_td_rescoring", "attention_rescoring", "ctc_beam_td_attn_rescoring")
        if any(m in ctc_first for m in two_pass) and "ctc_prefix_beam_search" not in rest:
            rest = rest + ["ctc_prefix_beam_search"]          # the first pass, not reported under its own name
        for m in rest:
            if m == "ctc_greedy_search":
                from ..transformer.search import ctc_greedy_search
                results[m] = ctc_greedy_search(ctc_probs, encoder_lens, blank_id)
            elif m == "ctc_prefix_beam_search":
                from ..transformer.search import ctc_prefix_beam_search
                results[m] = ctc_prefix_beam_search(ctc_probs, encoder_lens, beam_size, context_graph, blank_id)
            elif m == "attention_beam_search":
                from ..transformer.attn_search import attention_beam_search
                results[m] = attention_beam_search(self, encoder_out, encoder_mask, beam_size, length_penalty, score_backend)
            elif m == "joint_decoding":
                from ..transformer.joint_search import joint_decoding
                results[m] = joint_decoding(self, encoder_out, encoder_lens, ctc_probs, ctc_weight, beam_size,
                                            length_bonus=length_penalty, blank_id=blank_id, backend=score_backend,
                                            cat_embs=cat_embs)
            elif m == "attention":
                raise NotImplementedError("decode mode 'attention' is not accepted under the reference's name: the attention "
                                          "decoder's beam search is the mode 'attention_beam_search'")
            else:
                raise NotImplementedError(f"decode mode {m!r} is outside the accelerated path")
        if "rnnt_beam_search" in methods:
            results["rnnt_beam_search"] = self.beam_search_decode(
                encoder_outs=encoder_out, encoder_lens=encoder_lens, ctc_probs=ctc_probs, beam_size=beam_size,
                ctc_weight=ctc_weight, transducer_weight=transducer_weight, cat_embs=cat_embs, frame_body=frame_body)
        if "rnnt_greedy_search" in methods:
            results["rnnt_greedy_search"] = batch_greedy_search(self, encoder_out, encoder_lens)
        if two_pass:
            lens_host = encoder_lens.tolist()
            firsts, tds, attns = {}, {}, {}                   # per first pass: computed once, shared by the modes that rest on it
            for m in two_pass:
                kind = "ctc" if m in ctc_first else "rnnt"
                if kind not in firsts:
                    firsts[kind] = results["ctc_prefix_beam_search"] if kind == "ctc" else self.beam_search_decode(
                        encoder_outs=encoder_out, encoder_lens=encoder_lens, ctc_probs=ctc_probs, beam_size=beam_size,
                        ctc_weight=search_ctc_weight, transducer_weight=search_transducer_weight, cat_embs=cat_embs,
                        frame_body=frame_body)
                first = firsts[kind]
                hyps = [r.nbest if r.nbest is not None else [r.tokens] for r in first]
                if m != "attention_rescoring" and kind not in tds:
                    tds[kind] = self.score_hypotheses(encoder_out, lens_host, hyps, backend=score_backend)
                if m in ATTN_RESCORING_MODES and kind not in attns:
                    attns[kind] = self.score_attention(encoder_out, lens_host, hyps, reverse_weight, score_backend)
                if m in RESCORING_MODES:
                    results[m] = rescore(first, tds[kind], ctc_weight, transducer_weight)
                elif m == "attention_rescoring":
                    results[m] = attention_rescore(first, attns[kind], reverse_weight, ctc_weight)
                else:
                    results[m] = attention_rescore(first, attns[kind], reverse_weight, ctc_weight, attn_weight, tds[kind],
                                                   transducer_weight)
            if "ctc_prefix_beam_search" not in methods:
                results.pop("ctc_prefix_beam_search", None)
        return results
