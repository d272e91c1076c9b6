"""Encoder + CTC container exposing what the hot path's callers use on the reference's ASRModel / Transducer:
`.encoder`, `.ctc`, `_forward_encoder` (asr_model.py:294-321), `ctc_logprobs` (:324-335) and `decode` for the
CTC modes (:337-440).  The RNN-T predictor/joint and the losses are containers around the path, not the path; transducer
decoding joins in paper_accurate_fast_cheap_amd/transducer.  An attention decoder (`decoder=`,
transformer/decoder.py) serves the second pass: `score_attention` and the "attention_rescoring" mode
(transformer/attn_rescore.py)."""
from typing import Callable, Dict, Iterator, List, Optional, Tuple

import torch

from ..utils.graph_step import chunk_windows
from .ctc import CTC
from .search import DecodeResult, ctc_greedy_search


class ASRModel(torch.nn.Module):
    def __init__(self, vocab_size: int, encoder: torch.nn.Module, ctc: CTC, ctc_weight: float = 1.0,
                 special_tokens: Optional[dict] = None, decoder: Optional[torch.nn.Module] = None, reverse_weight: float = 0.0,
                 lsm_weight: float = 0.0, length_normalized_loss: bool = False, **_unused_model_conf):
        super().__init__()
        self.vocab_size = vocab_size
        self.encoder = encoder
        self.ctc = ctc
        self.decoder = decoder          # the attention decoder of the second pass (transformer/decoder.py), or None
        self.ctc_weight = ctc_weight
        # the attention term of the training objective (transformer/attn_train.py): the right decoder's share of it, the label
        # smoothing and the loss' denominator (the reference's keys and defaults, asr_model.py:66-68)
        self.reverse_weight = reverse_weight
        self.lsm_weight = lsm_weight
        self.length_normalized_loss = length_normalized_loss
        self.special_tokens = special_tokens
        self.sos = (vocab_size - 1) if special_tokens is None else special_tokens.get("<sos>", vocab_size - 1)
        self.eos = (vocab_size - 1) if special_tokens is None else special_tokens.get("<eos>", vocab_size - 1)

    def forward(self, batch: dict, device: torch.device) -> Dict[str, Optional[torch.Tensor]]:
        """The training objective over the accelerated encoder: the CTC loss, and with an attention decoder that has trainable
        parameters and ctc_weight != 1 the hybrid ctc_weight * ctc + (1 - ctc_weight) * att of asr_model.py:199-205 (adding the
        keys loss_att and th_accuracy).  Without a decoder, or with the frozen one of the second pass, CTC only."""
        speech = batch["feats"].to(device)
        speech_lengths = batch["feats_lengths"].to(device)
        text = batch["target"].to(device)
        text_lengths = batch["target_lengths"].to(device)
        encoder_out, encoder_mask = self.encoder(speech, speech_lengths)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        loss_ctc = self.ctc.loss(encoder_out.float(), encoder_out_lens, text, text_lengths)
        if self.ctc_weight != 1.0 and self._trains_attention():
            loss_att, acc_att = self._calc_att_loss(encoder_out, encoder_mask, text, batch["target_lengths"])
            loss = self.ctc_weight * loss_ctc + (1 - self.ctc_weight) * loss_att
            return {"loss": loss, "loss_att": loss_att, "loss_ctc": loss_ctc, "th_accuracy": acc_att}
        return {"loss": loss_ctc, "loss_ctc": loss_ctc}

    def _trains_attention(self) -> bool:
        from .attn_train import trainable_decoder
        return trainable_decoder(self)

    def _calc_att_loss(self, encoder_out: torch.Tensor, encoder_mask: torch.Tensor, text: torch.Tensor,
                       text_lengths: torch.Tensor, backend: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loss_att, acc_att) of asr_model.py:251-292 (transformer/attn_train.att_loss); text_lengths as the batch holds them
        (on the host: the packed rows are then planned without reading the device)."""
        from .attn_train import att_loss
        return att_loss(self, encoder_out, encoder_mask, text, text_lengths, backend)

    def _forward_encoder(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                         num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                         cat_embs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if simulate_streaming and decoding_chunk_size > 0:
            return self.encoder.forward_chunk_by_chunk(speech, decoding_chunk_size=decoding_chunk_size,
                                                       num_decoding_left_chunks=num_decoding_left_chunks)
        return self.encoder(speech, speech_lengths, decoding_chunk_size=decoding_chunk_size,
                            num_decoding_left_chunks=num_decoding_left_chunks, cat_embs=cat_embs)

    def ctc_logprobs(self, encoder_out: torch.Tensor, blank_penalty: float = 0.0, blank_id: int = 0) -> torch.Tensor:
        if blank_penalty > 0.0:
            logits = self.ctc.ctc_lo(encoder_out)
            logits[:, :, blank_id] -= blank_penalty
            return logits.log_softmax(dim=2)
        return self.ctc.log_softmax(encoder_out)

    def is_bidirectional_decoder(self) -> bool:
        return self.decoder is not None and hasattr(self.decoder, "right_decoder")

    def score_attention(self, encoder_out: torch.Tensor, encoder_lens, hyps: List[List[List[int]]],
                        reverse_weight: float = 0.0, backend: Optional[str] = None):
        """The attention decoder's scores of n-best lists: hyps[b] is a list of token lists for utterance b of encoder_out
        (B, T', D); encoder_lens a (B) tensor or list (lengths on the host spare one read of the device).  Returns an
        attn_rescore.AttentionScores: per utterance and hypothesis l2r = sum_j log p(y_j | y_<j, x) + log p(eos | y, x) and its
        L + 1 terms l2r_logp; with reverse_weight > 0 also r2l / r2l_logp of the right decoder over the reversed hypothesis.
        The empty hypothesis is legal and scores log p(eos | sos).
        backend "framework": the reference's recipe as framework ops (memory repeated per hypothesis, padding, masks, full
          log-softmax, gather), on the CPU and the GPU.
        backend "kernels": packed rows on the library's GEMMs and the kernels of include/pafc_attention.h, GPU only, never a
          fallback: PafcError naming what is unmet.
        None: kernels on the GPU, framework on the CPU.
        NotImplementedError without a decoder; ValueError for reverse_weight > 0 without a right_decoder or a token outside the
        vocabulary.  The result's `stats` holds what the kernels backend counted (rows, chunks, logits_peak_bytes)."""
        from .attn_rescore import score_attention
        return score_attention(self, encoder_out, encoder_lens, hyps, reverse_weight, backend)

    def _attention_rescoring(self, first: List[DecodeResult], encoder_out, encoder_lens, ctc_weight: float, reverse_weight: float,
                             score_backend: Optional[str]) -> List[DecodeResult]:
        """search.py:364-448 over a CTC prefix beam search: final_i = attn_i + ctc_weight * ctc_score_i."""
        from .attn_rescore import attention_rescore
        hyps = [r.nbest if r.nbest is not None else [r.tokens] for r in first]
        scores = self.score_attention(encoder_out, encoder_lens.tolist(), hyps, reverse_weight, score_backend)
        return attention_rescore(first, scores, reverse_weight, ctc_weight)

    @torch.no_grad()
    def decode(self, methods: List[str], speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int = 10,
               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0,
               simulate_streaming: bool = False, reverse_weight: float = 0.0, blank_id: int = 0,
               blank_penalty: float = 0.0, cat_embs: Optional[torch.Tensor] = None, context_graph=None,
               score_backend: Optional[str] = None, length_penalty: float = 0.0, **_ignored
               ) -> Dict[str, List[DecodeResult]]:
        """"attention_rescoring" (a model with an attention decoder): first pass ctc_prefix_beam_search (computed once when that
        mode is requested too), final_i = attn_i + ctc_weight * ctc_score_i with attn_i of score_attention (backend:
        score_backend) and reverse_weight; the n-best lists come back re-ordered by final (attn_rescore.attention_rescore).
        "attention_beam_search" (likewise): the decoder's own autoregressive beam search with length_penalty
        (attn_search.attention_beam_search, backend: score_backend) -- the reference's mode "attention", a spelling that is still
        refused here.
        "joint_decoding" (likewise): the time-synchronous joint CTC/attention beam search (joint_search.joint_decoding) with
        ctc_weight, beam_size and length_bonus = length_penalty, as the reference maps them; backend: score_backend; cat_embs
        must be None for it."""
        assert speech.shape[0] == speech_lengths.shape[0]
        rescoring = "attention_rescoring" in methods
        for m in ("attention_rescoring", "attention_beam_search", "joint_decoding"):
            if m in methods and self.decoder is None:
                raise NotImplementedError(f"decode mode {m!r} needs an attention decoder (init_model builds one "
                                          "with args.attention_decoder)")
        encoder_out, encoder_mask = self._forward_encoder(speech, speech_lengths, decoding_chunk_size,
                                                          num_decoding_left_chunks, simulate_streaming, cat_embs)
        encoder_lens = encoder_mask.squeeze(1).sum(1)
        ctc_probs = self.ctc_logprobs(encoder_out, blank_penalty, blank_id)
        results = {}
        todo = [m for m in methods if m != "attention_rescoring"]
        if rescoring and "ctc_prefix_beam_search" not in todo:
            todo.append("ctc_prefix_beam_search")                 # the first pass, not reported under its own name
        for m in todo:
            if m == "ctc_greedy_search":
                results[m] = ctc_greedy_search(ctc_probs, encoder_lens, blank_id)
            elif m == "ctc_prefix_beam_search":
                from .search import ctc_prefix_beam_search
                results[m] = ctc_prefix_beam_search(ctc_probs, encoder_lens, beam_size, context_graph, blank_id)
            elif m == "attention_beam_search":
                from .attn_search import attention_beam_search
                results[m] = attention_beam_search(self, encoder_out, encoder_mask, beam_size, length_penalty, score_backend)
            elif m == "joint_decoding":
                from .joint_search import joint_decoding
                results[m] = joint_decoding(self, encoder_out, encoder_lens, ctc_probs, ctc_weight, beam_size,
                                            length_bonus=length_penalty, blank_id=blank_id, backend=score_backend,
                                            cat_embs=cat_embs)
            elif m == "attention":
                raise NotImplementedError("decode mode 'attention' is not accepted under the reference's name: the attention "
                                          "decoder's beam search is the mode 'attention_beam_search'")
            else:
                raise NotImplementedError(f"decode mode {m!r} is outside the accelerated path")
        if rescoring:
            results["attention_rescoring"] = self._attention_rescoring(results["ctc_prefix_beam_search"], encoder_out,
                                                                       encoder_lens, ctc_weight, reverse_weight, score_backend)
            if "ctc_prefix_beam_search" not in methods:
                del results["ctc_prefix_beam_search"]
        return results

    @torch.no_grad()
    def align(self, speech: torch.Tensor, speech_lengths: torch.Tensor, text: torch.Tensor, text_lengths: torch.Tensor,
              blank_id: int = 0, blank_penalty: float = 0.0, tokens_info: bool = False) -> List[DecodeResult]:
        """Forced alignment of the transcripts text[b, :text_lengths[b]] to the audio (the reference's Model.align,
        wenet/cli/model.py:92-104,148, for a batch): encoder -> CTC log-probabilities -> search.ctc_forced_align.  Each result
        carries the tokens handed in, the path score and the first / last encoder frame of every token (times / end_times).
        tokens_info: also (start, end) seconds per token from gen_timestamps_from_peak with the encoder's frame period
        (subsampling rate x 0.01 s) and max_token_duration 1.0, as cli/model.py:113-118."""
        from ..utils.ctc_utils import gen_timestamps_from_peak
        from .search import ctc_forced_align
        assert speech.shape[0] == speech_lengths.shape[0] == text.shape[0] == text_lengths.shape[0]
        encoder_out, encoder_mask = self._forward_encoder(speech, speech_lengths)
        encoder_lens = encoder_mask.squeeze(1).sum(1)
        ctc_probs = self.ctc_logprobs(encoder_out, blank_penalty, blank_id)
        results = ctc_forced_align(ctc_probs, encoder_lens, text, text_lengths, blank_id)
        if tokens_info:
            frame_rate = self.encoder.embed.subsampling_rate * 0.01
            max_duration = encoder_out.size(1) * frame_rate
            for r in results:
                r.tokens_info = gen_timestamps_from_peak(r.times, max_duration, frame_rate, 1.0)
        return results

    def _stream_windows(self, speech: torch.Tensor, decoding_chunk_size: int, who: str) -> Iterator[Tuple[int, torch.Tensor]]:
        """The window walk of a chunked stream, the contract of encoder.stream_chunks: the windows of forward_chunk_by_chunk
        through the encoder with carried state -- forward_chunk_carry for a causal conv module (or none),
        forward_chunk_lookahead for the shipped non-causal one, drained with final=True after the last window.  Yields
        (window index, the window's output frames (B, n, D)); the final drain of the look-ahead emits more frames than
        decoding_chunk_size."""
        if decoding_chunk_size <= 0:
            raise ValueError(f"{who}: decoding_chunk_size must be > 0 (a chunked stream)")
        from .encoder_layer import streamable_slot
        enc = self.encoder
        layers = list(getattr(enc, "encoders", []))
        if not layers or any(not streamable_slot(l.self_attn) for l in layers) or not enc.normalize_before:
            raise ValueError(f"{who}: the encoder must be a pre-norm uni-directional model (rwkv_tmix60 slot, or mamba_att with "
                             "rnn_att_direction: uni); a bidirectional encoder needs the whole utterance")
        lookahead = any(l.conv_module is not None and l.conv_module.lorder == 0 for l in layers)
        T = speech.size(1)
        starts, window, _ = chunk_windows(enc.embed, decoding_chunk_size, T)

        def walk():
            state = None
            for i, c in enumerate(starts):
                xs = speech[:, c:min(c + window, T)]
                if lookahead:
                    y, state = enc.forward_chunk_lookahead(xs, state, final=(i == len(starts) - 1))
                else:
                    y, state = enc.forward_chunk_carry(xs, 0, state)
                yield i, y
        return walk()

    @torch.no_grad()
    def stream_ctc_search(self, speech: torch.Tensor, decoding_chunk_size: int, mode: str = "ctc_prefix_beam_search",
                          beam_size: int = 10, context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0,
                          on_partial: Optional[Callable[[int, List[DecodeResult], List[List[int]]], None]] = None,
                          max_total_frames: Optional[int] = None) -> List[DecodeResult]:
        """Streaming CTC search (mode: ctc_prefix_beam_search or ctc_greedy_search) of B equal-length streams (B, T, F):
        the window walk of _stream_windows, each window's frames through ctc_logprobs into one search.CtcStreamer.
        on_partial(window_index, partial_results, committed_tokens_per_row) is called once per window.  Returns per
        stream the full DecodeResult (times included).  Over the stream the result equals the offline search of
        ctc_logprobs of the concatenated encoder outputs of the same steps.  max_total_frames (default: what the speech
        can produce) sizes the beam search's pools."""
        from .search import CtcStreamer
        windows = self._stream_windows(speech, decoding_chunk_size, "stream_ctc_search")
        if max_total_frames is None:
            max_total_frames = speech.size(1) // self.encoder.embed.subsampling_rate + decoding_chunk_size
        streamer = CtcStreamer(speech.size(0), decoding_chunk_size, mode, beam_size, context_graph, blank_id, max_total_frames)
        for i, y in windows:
            partial = None                                      # (a window may come without output frames)
            for a in range(0, y.size(1), decoding_chunk_size):
                partial = streamer.feed(self.ctc_logprobs(y[:, a:a + decoding_chunk_size], blank_penalty, blank_id))
            if on_partial is not None:
                on_partial(i, partial if partial is not None else streamer.partials(), [list(c) for c in streamer.committed])
        return streamer.results()
