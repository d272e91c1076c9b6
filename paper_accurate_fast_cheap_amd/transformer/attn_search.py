"""Autoregressive beam search with the attention decoder (reference: attention_beam_search, wenet/transformer/search.py:251-360,
the decode mode "attention" of its ASRModel.decode; here the mode is "attention_beam_search").

backend "framework" is the reference's loop, step for step, on TransformerDecoder.forward_one_step: the memory repeated once per
beam, an (i, i) mask per step, the (B*N, V) log-softmax, two topk, an index_select of every cache and a read of the device
(`end_flag.sum() == running_size`) per step.

backend "kernels" keeps the R = B*N running rows on the device.  Per layer the source attention's K | V of an utterance is ONE
projection of its memory rows, made before the loop and shared by its beams; the self-attention keeps a key/value cache whose
rows are written once and never moved -- a beam finds its ancestors through a small index table -- and the two prunings read the
logits directly (include/pafc_attn_search.h: pafc_mha_step, pafc_attn_beam_select).  Every nn.Linear runs on the library's GEMMs
through decoder_rows.proj, every LayerNorm on hip_ops.add_layernorm, the source attention on hip_ops.mha_rows with one group per
utterance: the layer body is decoder_rows.decoder_layers on the set-up of decoder_rows.SearchEngine; this module supplies the
self-attention and the selection.  A step's shapes do not depend on the step and nothing in it reads the device: the position
and the `done` flag live in device memory, a step that finds `done` set (or the cap reached) changes nothing, and the host looks
at (done, pos) once per STEPS_PER_READ steps.  After the loop one read brings the trace (parent, token, score of every slot and
step) and the scores; the backtrace and the length penalty run on the host in float64.  step_graph=True replays a block of steps
as one captured graph instead of issuing its launches one by one."""
from typing import List, Optional

import numpy as np
import torch

from .decoder import subsequent_mask
from .decoder_rows import SearchEngine, kernels_unmet, pass_launches
from .search import DecodeResult
from ..utils import graph_step

STEPS_PER_READ = 8                 # steps issued between two looks at (done, pos)
CACHE_CAP_BYTES = 1 << 30          # the self-attention caches of one call, all layers: 3 x 251 x 80 rows of 2 x 512 fp32 are 247 MB
MAX_BEAM = 16                      # pafc_attn_beam_select's candidates of an utterance fit one wave: N * N <= 256


def mask_finished_scores(score: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """wenet/utils/common.py: an ended beam keeps one candidate, at 0; its others get -inf.  score (R, N), flag (R, 1)."""
    n = score.size(-1)
    zero = torch.zeros_like(flag, dtype=torch.bool)
    if n > 1:
        unfinished = torch.cat((zero, flag.repeat([1, n - 1])), dim=1)
        finished = torch.cat((flag, zero.repeat([1, n - 1])), dim=1)
    else:
        unfinished, finished = zero, flag
    score.masked_fill_(unfinished, -float("inf"))
    score.masked_fill_(finished, 0)
    return score


def mask_finished_preds(pred: torch.Tensor, flag: torch.Tensor, eos: int) -> torch.Tensor:
    """wenet/utils/common.py: every candidate of an ended beam is eos."""
    return pred.masked_fill_(flag.repeat([1, pred.size(-1)]), eos)


def _results(hyps: List[List[int]], final: List[float], B: int, N: int, eos: int, stats, trace) -> List[DecodeResult]:
    """hyps: the R rows without their sos; final: their penalised scores.  Per utterance the N beams in final-score order
    (stable: ties to the lower slot, which is where the reference's max lands), eos stripped."""
    out = []
    for b in range(B):
        order = sorted(range(N), key=lambda i: -final[b * N + i])
        nbest = [[t for t in hyps[b * N + i] if t != eos] for i in order]
        scores = [final[b * N + i] for i in order]
        out.append(DecodeResult(tokens=nbest[0], score=scores[0], nbest=nbest, nbest_scores=scores, stats=stats,
                                trace=trace if b == 0 else None))
    return out


@torch.no_grad()
def attention_beam_search(model, encoder_out: torch.Tensor, encoder_mask: torch.Tensor, beam_size: int = 10,
                          length_penalty: float = 0.0, backend: Optional[str] = None, max_len: Optional[int] = None,
                          return_trace: bool = False, step_graph: bool = False) -> List[DecodeResult]:
    """encoder_out (B, T', d), encoder_mask (B, 1, T') bool, True on an utterance's frames (its first T'_b) -> one DecodeResult
    per utterance: tokens of the best beam without eos, score its penalised score score / length ** length_penalty, nbest /
    nbest_scores all beam_size beams in that order, stats what the kernels backend counted (steps, host_reads,
    launches_per_step, cache_bytes; None from the framework backend).  The search runs at most T' steps (the padded length, as in
    the reference), or max_len if that is lower.
    backend: "framework" | "kernels" | None (kernels on the GPU, framework on the CPU); "kernels" is never a fallback: PafcError
    names what it cannot take.
    step_graph (kernels backend): capture one block of STEPS_PER_READ steps into a hipGraph (utils.graph_step.capture) and
    replay it; a capture the runtime refuses leaves the call eager (stats["step_graph"] says which).
    return_trace: results[0].trace = dict(parent, token, score), (steps, B * beam_size) arrays: slot r's parent slot within its
    utterance, its token and its unpenalised score after every step."""
    from ..transducer.search.rescoring import check_score_backend
    decoder = getattr(model, "decoder", None)
    if decoder is None:
        raise NotImplementedError("attention_beam_search needs an attention decoder (init_model builds one with "
                                  "args.attention_decoder)")
    backend = check_score_backend(backend, encoder_out.is_cuda)
    B, T = encoder_out.size(0), encoder_out.size(1)
    if encoder_mask.shape != (B, 1, T):
        raise ValueError(f"encoder_mask {tuple(encoder_mask.shape)} for encoder_out {tuple(encoder_out.shape)}")
    if max_len is not None and max_len < 1:
        raise ValueError(f"max_len = {max_len}")
    cap = T if max_len is None else min(T, int(max_len))
    V = model.vocab_size
    if backend == "kernels":
        from .._lib import PafcError
        if not 1 <= beam_size <= MAX_BEAM:
            raise PafcError(f"attention_beam_search(backend='kernels'): a beam of {beam_size} (the selection kernel takes 1.."
                            f"{MAX_BEAM})")
        if V < beam_size:
            raise PafcError(f"attention_beam_search(backend='kernels'): a vocabulary of {V} for a beam of {beam_size}")
        unmet = kernels_unmet(model, encoder_out, False)
        if unmet is not None:
            raise PafcError(f"attention_beam_search(backend='kernels'): {unmet}")
        return _search_kernels(model, encoder_out, encoder_mask, beam_size, length_penalty, cap, return_trace, step_graph)
    if step_graph:
        raise ValueError("step_graph replays the kernels backend's step; the framework backend has none")
    if beam_size < 1 or V < beam_size:
        raise ValueError(f"a beam of {beam_size} for a vocabulary of {V}")
    return _search_framework(model, encoder_out, encoder_mask, beam_size, length_penalty, cap, return_trace)


def _search_framework(model, encoder_out, encoder_mask, beam_size, length_penalty, cap, return_trace):
    device = encoder_out.device
    batch_size, maxlen, encoder_dim = encoder_out.shape
    running_size = batch_size * beam_size
    dtype = next(model.decoder.parameters()).dtype
    encoder_out = encoder_out.to(dtype).unsqueeze(1).repeat(1, beam_size, 1, 1).view(running_size, maxlen, encoder_dim)
    encoder_mask = encoder_mask.unsqueeze(1).repeat(1, beam_size, 1, 1).view(running_size, 1, maxlen)
    hyps = torch.ones([running_size, 1], dtype=torch.long, device=device).fill_(model.sos)
    prefix_len = hyps.size(1)
    scores = torch.tensor([0.0] + [-float("inf")] * (beam_size - 1), dtype=torch.float)
    scores = scores.to(device).repeat([batch_size]).unsqueeze(1).to(device)
    end_flag = torch.zeros_like(scores, dtype=torch.bool, device=device)
    cache = None
    trace = dict(parent=[], token=[], score=[])
    for i in range(prefix_len, cap + 1):
        if end_flag.sum() == running_size:
            break
        hyps_mask = subsequent_mask(i).unsqueeze(0).repeat(running_size, 1, 1).to(device)
        logp, cache = model.decoder.forward_one_step(encoder_out, encoder_mask, hyps, hyps_mask, cache)
        top_k_logp, top_k_index = logp.topk(beam_size)
        top_k_logp = mask_finished_scores(top_k_logp, end_flag)
        top_k_index = mask_finished_preds(top_k_index, end_flag, model.eos)
        scores = scores + top_k_logp
        scores = scores.view(batch_size, beam_size * beam_size)
        scores, offset_k_index = scores.topk(k=beam_size)
        cache_index = (offset_k_index // beam_size).view(-1)
        base_cache_index = (torch.arange(batch_size, device=device).view(-1, 1).repeat([1, beam_size]) * beam_size).view(-1)
        cache_index = base_cache_index + cache_index
        cache = [torch.index_select(c, dim=0, index=cache_index) for c in cache]
        scores = scores.view(-1, 1)
        base_k_index = torch.arange(batch_size, device=device).view(-1, 1).repeat([1, beam_size])
        base_k_index = base_k_index * beam_size * beam_size
        best_k_index = base_k_index.view(-1) + offset_k_index.view(-1)
        best_k_pred = torch.index_select(top_k_index.view(-1), dim=-1, index=best_k_index)
        best_hyps_index = best_k_index // beam_size
        last_best_k_hyps = torch.index_select(hyps, dim=0, index=best_hyps_index)
        hyps = torch.cat((last_best_k_hyps, best_k_pred.view(-1, 1)), dim=1)
        end_flag = torch.eq(hyps[:, -1], model.eos).view(-1, 1)
        if return_trace:
            trace["parent"].append((offset_k_index // beam_size).view(-1).tolist())
            trace["token"].append(best_k_pred.tolist())
            trace["score"].append(scores.view(-1).tolist())
    scores = scores.view(batch_size, beam_size)
    lengths = hyps.ne(model.eos).sum(dim=1).view(batch_size, beam_size).float()
    scores = scores / lengths.pow(length_penalty)
    if return_trace:
        trace = dict(parent=np.asarray(trace["parent"], dtype=np.int64).reshape(-1, running_size),
                     token=np.asarray(trace["token"], dtype=np.int64).reshape(-1, running_size),
                     score=np.asarray(trace["score"], dtype=np.float64).reshape(-1, running_size))
    return _results(hyps[:, prefix_len:].tolist(), scores.view(-1).tolist(), batch_size, beam_size, model.eos, None,
                    trace if return_trace else None)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels backend
# ---------------------------------------------------------------------------------------------------------------------------

class _Engine(SearchEngine):
    """The device state of one call and its step.  Nothing here reads the device."""

    def __init__(self, model, encoder_out, encoder_mask, N: int, cap: int):
        from .._lib import PafcError
        self.bind_decoder(model, "attention_beam_search")
        dec, dtype = self.dec, self.dtype
        self.N, self.cap, self.eos = N, cap, int(model.eos)
        dev = encoder_out.device
        B, T, d = encoder_out.shape
        self.B, self.R, self.P = B, B * N, cap + 1
        R, P = self.R, self.P
        self.cache_bytes = self.cache_bytes_of(P * R, d)
        if self.cache_bytes > CACHE_CAP_BYTES:
            raise PafcError(f"attention_beam_search(backend='kernels'): the key/value caches of {len(dec.decoders)} layers x "
                            f"{P} positions x {R} rows need {self.cache_bytes} bytes, above CACHE_CAP_BYTES = {CACHE_CAP_BYTES}: "
                            "set max_len (or decode fewer utterances per call)")
        self.project_memory(encoder_out, encoder_mask.reshape(B, T).sum(1).to(torch.int32), N, P)
        # the state
        self.caches = [torch.empty(P, R, 2 * d, dtype=dtype, device=dev) for _ in dec.decoders]
        self.anc = torch.zeros(2, R, P, dtype=torch.int32, device=dev)
        self.state = torch.zeros(2, dtype=torch.int32, device=dev)              # pos, done
        self.pos, self.done = self.state[0:1], self.state[1:2]
        self.score = torch.full((B, N), -float("inf"), dtype=torch.float32, device=dev)
        self.score[:, 0] = 0.0
        self.score = self.score.reshape(R)
        self.ended = torch.zeros(R, dtype=torch.int32, device=dev)
        self.token = torch.full((R,), int(model.sos), dtype=torch.int32, device=dev)
        self.trace_parent = torch.zeros(P, R, dtype=torch.int32, device=dev)
        self.trace_token = torch.zeros(P, R, dtype=torch.int32, device=dev)
        self.trace_score = torch.zeros(P, R, dtype=torch.float32, device=dev)
        self.workspace = self.ops.attn_beam_select_workspace(B, N, dev)
        self.launches = pass_launches(dec) + 3                  # the decoder pass, output_layer, the selection's two

    def self_attention(self, i, layer, qkv):
        return self.ops.mha_step(qkv, self.caches[i], self.anc, self.pos, self.done, self.N, self.H)

    def step(self):
        dec = self.dec
        logits = self.proj(self.decoder_pass(self.token, self.pos), dec.output_layer.weight, dec.output_layer.bias)
        self.ops.attn_beam_select(logits, self.N, self.eos, self.cap, self.score, self.ended, self.token, self.anc,
                                  self.trace_parent, self.trace_token, self.trace_score, self.pos, self.done, self.workspace)


def backtrace(parent: np.ndarray, token: np.ndarray, N: int) -> List[List[int]]:
    """The rows' token lists (without sos) from a trace: parent / token (steps, R)."""
    steps, R = parent.shape
    hyps = []
    for r in range(R):
        base, cur, toks = (r // N) * N, r, []
        for s in range(steps - 1, -1, -1):
            toks.append(int(token[s, cur]))
            cur = base + int(parent[s, cur])
        hyps.append(toks[::-1])
    return hyps


def penalised(scores: np.ndarray, hyps: List[List[int]], sos: int, eos: int, length_penalty: float) -> List[float]:
    """score / length ** length_penalty in float64, length the tokens of [sos] + hyp that are not eos (search.py:347-348: with
    sos == eos the prefix is not counted, and a length of 0 divides by 0 unless length_penalty is 0)."""
    lengths = np.array([sum(t != eos for t in [sos] + h) for h in hyps], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (scores.astype(np.float64) / np.power(lengths, np.float64(length_penalty))).tolist()


def _search_kernels(model, encoder_out, encoder_mask, N, length_penalty, cap, return_trace, step_graph=False):
    eng = _Engine(model, encoder_out, encoder_mask, N, cap)
    R, P = eng.R, eng.P
    issued = reads = 0
    dev = encoder_out.device

    def block(n=STEPS_PER_READ):
        for _ in range(n):
            eng.step()

    graph, mode = None, "eager"
    while issued < cap:
        n = min(STEPS_PER_READ, cap - issued)
        if not step_graph or mode == "eager (capture refused)":
            block(n)
        else:
            # whole blocks: the steps past the cap are frozen.  The first block runs eagerly on the side stream (it warms every
            # kernel up where a capture wants them, and its steps count), the second is captured -- nothing runs during a
            # capture -- and replayed from then on: a plain chain on one stream.
            n = STEPS_PER_READ
            if issued == 0:
                graph_step.on_side_stream(dev, block)
            else:
                if graph is None:
                    graph, _ = graph_step.capture(block, dev)
                if graph is None:
                    mode = "eager (capture refused)"
                    block(n)
                else:
                    mode = "replayed"
                    graph.replay()
        issued += n
        if issued < cap:
            pos, done = eng.state.tolist()                    # the one look per block
            reads += 1
            if done or pos >= cap:
                break
    # one read: the trace, the scores and the state
    packed = torch.cat([eng.trace_parent.reshape(-1), eng.trace_token.reshape(-1), eng.trace_score.view(torch.int32).reshape(-1),
                        eng.score.view(torch.int32), eng.state]).cpu().numpy()
    reads += 1
    steps = int(packed[-2])
    parent = packed[:P * R].reshape(P, R)[:steps].astype(np.int64)
    token = packed[P * R:2 * P * R].reshape(P, R)[:steps].astype(np.int64)
    tscore = packed[2 * P * R:3 * P * R].view(np.float32).reshape(P, R)[:steps]
    score = packed[3 * P * R:3 * P * R + R].view(np.float32)
    hyps = backtrace(parent, token, N)
    final = penalised(score, hyps, int(model.sos), int(model.eos), length_penalty)
    stats = dict(steps=steps, steps_issued=issued, host_reads=reads, launches_per_step=eng.launches,
                 cache_bytes=eng.cache_bytes, rows=R, memory_rows=encoder_out.size(0) * encoder_out.size(1), step_graph=mode)
    trace = dict(parent=parent, token=token, score=tscore.astype(np.float64)) if return_trace else None
    return _results(hyps, final, eng.B, N, int(model.eos), stats, trace)
