"""The attention decoder's beam search on the GPU: the two kernels of include/pafc_attn_search.h against float64, and
attention_beam_search(backend="kernels") verified step by step through its trace against the float64 restatement
(tests/attn_search_ref.py) on the models of tests/test_attn_search.py.

Bounds.  pafc_mha_step, as tests/test_mha_rows_gpu.py derives its own: fp32, max |err| against float64 <= 4 x the max |err| of
the same formula run in float32 on the CPU; bf16, 4 x the error of the float32 CPU run on operands rounded to bf16 against
float64 on the unrounded ones (the kernel adds one bf16 rounding of its output).  A case whose CPU error is exactly zero
(position 0: one key, the softmax is 1) joins the next non-zero yardstick.  pafc_attn_beam_select: the inputs keep every kept
candidate 1e-3 from its neighbours and from every dropped one in float64 (asserted here, on the CPU), so parents, tokens, flags
and tables must equal the float64 selection exactly; scores within 4 x the float32 CPU error of the same sums.  The engine: a
search is a chain of near-ties, so a run is not compared with one float64 search but checked step by step along its own path:
every selected (parent, token) has a float64 candidate score of at least the float64 N-th best - eps_i, and the kernel's
score is within eps_i of the float64 score of its own path, eps_i = 8 (i + 1) e32 with e32 the largest per-token
log-probability error of this project's decoder run in float32 on the CPU against float64 on the case's own prefixes (the
8 x float32-CPU convention of tests/test_attn_rescore_gpu.py, accumulated over the steps).  For the bf16 decoder the float32
CPU run uses weights and memory rounded to bf16 and is compared with float64 on the unrounded ones: the error the operands'
rounding alone causes."""
import math

import numpy as np
import pytest
import torch

from tests import attn_rescore_cases as C
from tests import attn_search_ref as SR
from tests import parity_log
from tests.test_attn_search import T, batch_mask, case_inputs, search_model

pytestmark = pytest.mark.gpu

H, DK = 2, 64
D = H * DK
INF = float("inf")


# ---- pafc_mha_step -----------------------------------------------------------------------------------------------------------

def _gather_attention(qkv, cache, anc, N, pos):
    """out[r, h] = softmax_j(q . k_j / 8) v_j over the ancestors' cache rows j < pos and the row's own k, v, in qkv's dtype."""
    R = qkv.shape[0]
    base = (torch.arange(R) // N) * N
    out = torch.zeros(R, D, dtype=qkv.dtype)
    rows = base[:, None] + anc[:, :pos]                                             # (R, pos)
    past = cache[torch.arange(pos)[None, :], rows]                                  # (R, pos, 2 D)
    for h in range(H):
        cs = slice(h * DK, (h + 1) * DK)
        k = torch.cat([past[:, :, cs], qkv[:, None, D:2 * D][:, :, cs]], dim=1)
        v = torch.cat([past[:, :, D:][:, :, cs], qkv[:, None, 2 * D:][:, :, cs]], dim=1)
        s = torch.einsum("rd,rjd->rj", qkv[:, cs], k) / math.sqrt(DK)
        out[:, cs] = torch.einsum("rj,rjd->rd", torch.softmax(s, dim=-1), v)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mha_step_against_float64(hip, dtype):
    from paper_accurate_fast_cheap_amd import hip_ops
    P = 132
    g = torch.Generator().manual_seed(13)
    tag = "fp32" if dtype == torch.float32 else "bf16"
    pending = []
    for R, N in ((15, 5), (1, 1)):
        for pos in (0, 1, 63, 64, 65, 130):
            qkv = torch.randn(R, 3 * D, generator=g, dtype=torch.float64)
            cache = torch.randn(P, R, 2 * D, generator=g, dtype=torch.float64)
            anc = torch.randint(0, N, (R, P), generator=g)                          # beams share and swap ancestors at random
            if N > 1 and pos > 1:
                assert (anc[:, :pos] != (torch.arange(R) % N)[:, None]).any()       # not the identity
                assert any(len(set(anc[b * N:(b + 1) * N, j].tolist())) < N for b in range(R // N) for j in range(pos))
            want = _gather_attention(qkv, cache, anc, N, pos)
            if dtype == torch.float32:
                cpu = _gather_attention(qkv.float(), cache.float(), anc, N, pos)
            else:
                cpu = _gather_attention(qkv.bfloat16().float(), cache.bfloat16().float(), anc, N, pos)
            dev = "cuda"
            qbuf = torch.full((R, 3 * D + 8), float("nan"), dtype=dtype, device=dev)      # a pitch wider than 3 D
            qbuf[:, :3 * D] = qkv.to(dtype)
            cbuf = torch.full((P, R, 2 * D), float("nan"), dtype=dtype, device=dev)       # NaN beyond what is owned
            cbuf[:pos] = cache[:pos].to(dtype)
            abuf = torch.full((2, R, P), 9999, dtype=torch.int32, device=dev)
            abuf[pos & 1, :, :pos] = anc[:, :pos].to(torch.int32)
            pos_t = torch.tensor([pos], dtype=torch.int32, device=dev)
            done_t = torch.zeros(1, dtype=torch.int32, device=dev)
            before = _bits(cbuf)
            out = torch.full((R, D), float("nan"), dtype=dtype, device=dev)
            hip_ops.mha_step(qbuf[:, :3 * D], cbuf, abuf, pos_t, done_t, N, H, out=out)
            again = torch.full((R, D), float("nan"), dtype=dtype, device=dev)
            hip_ops.mha_step(qbuf[:, :3 * D], cbuf, abuf, pos_t, done_t, N, H, out=again)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all() and torch.equal(_bits(out), _bits(again))    # owned, and the same bits twice
            after = _bits(cbuf)
            assert torch.equal(after[pos], _bits(qkv[:, D:].to(dtype)))                   # the row's own slot: its k | v
            keep = torch.ones(P, dtype=torch.bool)
            keep[pos] = False
            assert torch.equal(after[keep], before[keep])                                 # every other position untouched
            got = out.double().cpu()
            ek, ec = (got - want).abs().max().item(), (cpu.double() - want).abs().max().item()
            print(f"mha_step {tag} R={R} pos={pos}: max|err| kernel {ek:.3e}, cpu yardstick {ec:.3e}")
            parity_log.record(f"mha_step_{tag}_R{R}_pos{pos}", max_abs_err=ek, cpu_yardstick_err=ec)
            pending.append(ek)
            if ec > 0:
                assert max(pending) <= 4 * ec, (R, pos, pending, ec)
                pending = []
            # pos = P, a negative pos, or done set: nothing at all is written
            for p_bad, d_bad in ((P, 0), (-1, 0), (pos, 1)):
                out.fill_(float("nan"))
                frozen = _bits(cbuf)
                hip_ops.mha_step(qbuf[:, :3 * D], cbuf, abuf, torch.tensor([p_bad], dtype=torch.int32, device=dev),
                                 torch.tensor([d_bad], dtype=torch.int32, device=dev), N, H, out=out)
                torch.cuda.synchronize()
                assert torch.isnan(out).all() and torch.equal(_bits(cbuf), frozen)
    assert not pending


# ---- pafc_attn_beam_select ---------------------------------------------------------------------------------------------------

def _select(logits, score, ended, N, eos, dtype=torch.float64):
    """The reference's two prunings in `dtype`: per utterance the chosen (parent, token, total) in order, and the sorted totals
    of all N * N candidates (kept first)."""
    R, V = logits.shape
    logp = torch.log_softmax(logits.to(dtype), dim=-1)
    out, totals = [], []
    for b in range(R // N):
        cands = []
        for i in range(N):
            r = b * N + i
            if ended[r]:
                row = [(eos, 0.0)] + [(eos, -INF)] * (N - 1)
            else:
                vals, idx = torch.sort(logp[r], descending=True, stable=True)
                row = [(int(idx[k]), vals[k].item()) for k in range(N)]
            for k, (tok, lp) in enumerate(row):
                total = (score[r].to(dtype) + torch.tensor(lp, dtype=dtype)).item()
                cands.append((-total if total > -INF else INF, i * N + k, i, tok, total))
        cands.sort()
        out.append([(c[2], c[3], c[4]) for c in cands[:N]])
        totals.append([c[4] for c in cands])
    return out, totals


def _select_inputs(B, N, V, kind, seed):
    """float32-representable logits and scores whose float64 selection has every kept candidate >= 1e-3 from its neighbours and
    from every dropped one (the first seed of seed, seed + 1000, ... for which that holds; the caller asserts it again)."""
    R, eos = B * N, V - 1
    while True:
        g = torch.Generator().manual_seed(seed)
        logits = (torch.randn(R, V, generator=g) * 2).double()
        for r in range(R):                                                           # the N + 1 largest of a row: well apart
            idx = torch.randperm(V, generator=g)[:min(N + 1, V)]
            gaps = torch.rand(len(idx), generator=g) * 0.3 + 0.01
            logits[r, idx] = (logits[r].max() + 0.5 + torch.cumsum(gaps, 0)).float().double()
        if kind == "first":
            score = torch.tensor([0.0] + [-INF] * (N - 1), dtype=torch.float64).repeat(B)
            ended = torch.zeros(R, dtype=torch.bool)
        else:
            score = -(torch.cumsum(torch.rand(R, generator=g) * 0.5 + 0.01, 0))[torch.randperm(R, generator=g)].float().double()
            ended = torch.ones(R, dtype=torch.bool) if kind == "all_ended" else torch.rand(R, generator=g) < 0.35
            if kind == "mid" and N > 1:
                ended[0], ended[1] = True, False                                       # ended and live beams side by side
        if _gaps_ok(_select(logits, score, ended, N, eos)[1], N):
            return logits, score, ended, eos
        seed += 1000


def _gaps_ok(totals, N):
    for t in totals:
        kept, dropped = t[:N], [x for x in t[N:] if x > -INF]
        if any(not math.isfinite(x) for x in kept):
            return False
        if any(a - b < 1e-3 for a, b in zip(kept, kept[1:])) or (dropped and kept[-1] - max(dropped) < 1e-3):
            return False
    return True


class _State:
    def __init__(self, B, N, P, pos, score, ended, seed):
        R, dev = B * N, "cuda"
        g = torch.Generator().manual_seed(seed)
        self.anc = torch.randint(0, N, (2, R, P), generator=g).to(torch.int32).to(dev)
        self.score, self.ended = score.float().to(dev), ended.to(torch.int32).to(dev)
        self.token = torch.full((R,), -5, dtype=torch.int32, device=dev)
        self.tp, self.tt = (torch.full((P, R), -1, dtype=torch.int32, device=dev) for _ in range(2))
        self.ts = torch.full((P, R), float("nan"), device=dev)
        self.pos = torch.tensor([pos], dtype=torch.int32, device=dev)
        self.done = torch.zeros(1, dtype=torch.int32, device=dev)

    def tensors(self):
        return [self.anc, self.score, self.ended, self.token, self.tp, self.tt, self.ts, self.pos, self.done]

    def snapshot(self):
        torch.cuda.synchronize()
        return [_bits(t).clone() for t in self.tensors()]

    def run(self, logits_dev, N, eos, cap):
        from paper_accurate_fast_cheap_amd import hip_ops
        hip_ops.attn_beam_select(logits_dev, N, eos, cap, self.score, self.ended, self.token, self.anc, self.tp, self.tt, self.ts,
                                 self.pos, self.done)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 4, 10, 16])
@pytest.mark.parametrize("V", [53, 5000])
def test_attn_beam_select_against_float64(hip, V, N, B):
    R, P, cap = B * N, 8, 6
    worst = 0.0
    for kind, pos in (("first", 0), ("mid", 3), ("all_ended", 5)):
        logits, score, ended, eos = _select_inputs(B, N, V, kind, seed=7 + V + 31 * N + B)
        want, totals = _select(logits, score, ended, N, eos)
        assert _gaps_ok(totals, N)                                                    # the inputs separate the candidates
        st = _State(B, N, P, pos, score, ended, seed=3)
        anc_before = st.anc.cpu().clone()
        buf = torch.full((R, V + 3), float("nan"), device="cuda")                     # a row pitch wider than V
        buf[:, :V] = logits.float()
        st.run(buf[:, :V], N, eos, cap)
        torch.cuda.synchronize()
        tp, tt, ts, anc = st.tp.cpu(), st.tt.cpu(), st.ts.cpu(), st.anc.cpu()
        logp32 = torch.log_softmax(logits.float(), dim=-1)
        ek = ec = 0.0
        for b in range(B):
            for s, (par, tok, total) in enumerate(want[b]):
                r = b * N + s
                assert (int(tp[pos, r]), int(tt[pos, r])) == (par, tok), (kind, b, s)
                assert int(st.token[r]) == tok and int(st.ended[r]) == int(tok == eos)
                assert anc[(pos + 1) & 1, r, :pos].tolist() == anc_before[pos & 1, b * N + par, :pos].tolist()
                assert int(anc[(pos + 1) & 1, r, pos]) == par
                assert st.score[r].item() == ts[pos, r].item()
                ek = max(ek, abs(st.score[r].item() - total))
                pr = b * N + par
                cpu32 = (score.float()[pr] + (0.0 if ended[pr] else logp32[pr, tok])).item()
                ec = max(ec, abs(cpu32 - total))
        assert torch.equal(anc[pos & 1], anc_before[pos & 1])                         # the half that was read is left alone
        rest = torch.ones(P, dtype=torch.bool)
        rest[pos] = False
        assert (tp[rest] == -1).all() and (tt[rest] == -1).all() and torch.isnan(ts[rest]).all()
        all_eos = all(tok == eos for u in want for _, tok, _ in u)
        assert int(st.pos) == pos + 1 and int(st.done) == int(all_eos) and (kind != "all_ended" or all_eos)
        print(f"attn_beam_select V={V} N={N} B={B} {kind}: max|err| kernel {ek:.3e}, float32 CPU {ec:.3e}")
        parity_log.record(f"attn_beam_select_V{V}_N{N}_B{B}_{kind}", max_abs_err=ek, cpu_float32_err=ec)
        assert ek <= 4 * ec if ec > 0 else ek == 0.0, (kind, ek, ec)
        worst = max(worst, ek)
        if kind == "all_ended":
            # done is set: further steps change nothing, whatever the logits
            frozen = st.snapshot()
            st.run(buf[:, :V].flip(1).contiguous(), N, eos, cap)
            assert all(torch.equal(a, b) for a, b in zip(st.snapshot(), frozen))
        if kind == "mid":
            # the cap is reached (pos = cap) without done: frozen too
            st.pos.fill_(cap)
            st.done.zero_()
            frozen = st.snapshot()
            st.run(buf[:, :V], N, eos, cap)
            assert all(torch.equal(a, b) for a, b in zip(st.snapshot(), frozen))
    assert math.isfinite(worst)


# ---- the engine, through its trace -------------------------------------------------------------------------------------------

def _verify_engine(tag, results, sd64, conf, enc64, mask, N, cap, sos, eos, model32, enc32, lp):
    """Every step of the returned trace against the float64 restatement along the run's own path (the module docstring)."""
    from paper_accurate_fast_cheap_amd.transformer.attn_search import STEPS_PER_READ, penalised
    tr, stats = results[0].trace, results[0].stats
    B = enc64.size(0)
    R = B * N
    steps = tr["parent"].shape[0]
    assert stats["steps"] == steps and 1 <= steps <= cap
    assert stats["host_reads"] - 1 <= stats["steps_issued"] / STEPS_PER_READ and stats["steps_issued"] < steps + STEPS_PER_READ
    sd = {k: v.detach().double() for k, v in sd64.items()}
    prefix = "left_decoder." if conf["bidirectional"] else ""
    Tm = enc64.size(1)
    memory = enc64.unsqueeze(1).repeat(1, N, 1, 1).view(R, Tm, -1)
    mmask = mask.unsqueeze(1).repeat(1, N, 1, 1).view(R, 1, Tm)
    mem32 = enc32.unsqueeze(1).repeat(1, N, 1, 1).view(R, Tm, -1)
    left32 = model32.decoder.left_decoder
    hyps = torch.full((R, 1), sos, dtype=torch.long)
    score = torch.tensor([0.0] + [-INF] * (N - 1), dtype=torch.float64).repeat(B)
    ended = torch.zeros(R, dtype=torch.bool)
    e32, slack, drift = 0.0, [], []
    for i in range(steps):
        assert not ended.all(), (tag, i)                                              # the search went on: some beam was live
        logp = SR.step_logp(sd, prefix, conf, memory, mmask, hyps)
        with torch.no_grad():
            l32 = left32(mem32, mmask, hyps, torch.full((R,), hyps.size(1)))[0][:, -1]
        e32 = max(e32, (torch.log_softmax(l32, dim=-1).double() - logp).abs().max().item())
        new_score, rows = torch.empty(R, dtype=torch.float64), []
        for b in range(B):
            cands = []
            for j in range(N):
                r = b * N + j
                if ended[r]:
                    cands.append(score[r].item())
                else:
                    cands += (score[r] + logp[r].topk(N).values).tolist()
            nth = sorted(cands, reverse=True)[N - 1]
            pairs = set()
            for s in range(N):
                r = b * N + s
                par, tok = int(tr["parent"][i, r]), int(tr["token"][i, r])
                assert 0 <= par < N and 0 <= tok < logp.size(1)
                pr = b * N + par
                assert tok == eos or not ended[pr], (tag, i, r)                       # mask_finished_preds
                mine = score[pr].item() + (0.0 if ended[pr] else logp[pr, tok].item())
                pairs.add((par, tok))
                slack.append((i, nth - mine))
                drift.append((i, abs(tr["score"][i, r] - mine)))
                new_score[r] = mine
                rows.append(pr)
            assert len(pairs) == N, (tag, i, b)                                       # distinct candidates
        toks = torch.from_numpy(tr["token"][i]).long()
        hyps = torch.cat([hyps[torch.tensor(rows)], toks[:, None]], dim=1)
        score, ended = new_score, toks == eos
    assert steps == cap or ended.all(), tag                                           # the stop rule
    worst_slack = max(s / (8 * (i + 1) * e32) for i, s in slack)
    worst_drift = max(d / (8 * (i + 1) * e32) for i, d in drift)
    print(f"{tag}: {steps} steps, e32 {e32:.3e}, worst slack / eps {worst_slack:.3f}, worst |score - float64| / eps {worst_drift:.3f}")
    parity_log.record(f"attn_search_{tag}", steps=steps, e32=e32, slack_over_eps=worst_slack, score_err_over_eps=worst_drift)
    assert e32 > 0 and worst_slack <= 1.0 and worst_drift <= 1.0, (tag, e32, worst_slack, worst_drift)
    # the results are the host backtrace of the trace, ordered by the penalised float32 scores
    mine = hyps[:, 1:].tolist()
    final = penalised(tr["score"][-1].astype(np.float32), mine, sos, eos, lp)
    for b, res in enumerate(results):
        order = sorted(range(N), key=lambda s: -final[b * N + s])
        assert res.nbest == [[t for t in mine[b * N + s] if t != eos] for s in order] and res.tokens == res.nbest[0]
        for got, s in zip(res.nbest_scores, order):
            assert got == final[b * N + s] or (math.isnan(got) and math.isnan(final[b * N + s]))
    return dict(eps=8 * steps * e32, hyps=mine, ended=ended, score=tr["score"][-1], steps=steps)


def _rescored(model64, enc64, mask, N, eos, info):
    """score_attention(backend="framework") in float64 of every slot's hypothesis against the kernel's unpenalised score: an
    ended beam's score is its tokens' and eos', a live one's its tokens' alone.  A wrong ancestor shows here."""
    B = enc64.size(0)
    lens = mask.squeeze(1).sum(1).tolist()
    hyps = [[[t for t in info["hyps"][b * N + s] if t != eos] for s in range(N)] for b in range(B)]
    sc = model64.score_attention(enc64, lens, hyps, 0.0, backend="framework")
    for b in range(B):
        for s in range(N):
            terms = sc.l2r_logp[b][s]
            want = math.fsum(terms if info["ended"][b * N + s] else terms[:-1])
            assert abs(info["score"][b * N + s] - want) <= info["eps"], (b, s, info["score"][b * N + s], want)


def _run_case(tag, normalize_before, N, dtype, lp=0.6):
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    model64 = search_model(normalize_before)
    enc64, mask = case_inputs("batch")
    gpu = search_model(normalize_before, dtype=torch.float32).cuda()
    gpu.decoder.fp32_split_operands = False                       # exact fp32 products: what the float32 yardstick measures
    model32 = search_model(normalize_before, dtype=torch.float32)
    enc32 = enc64.float()
    if dtype == torch.bfloat16:
        gpu.decoder.to(torch.bfloat16)
        model32.decoder.to(torch.bfloat16).to(torch.float32)      # the float32 CPU run on bf16-rounded weights and memory
        enc32 = enc64.bfloat16().float()
    res = attention_beam_search(gpu, enc64.float().cuda(), mask.cuda(), N, lp, backend="kernels", return_trace=True)
    info = _verify_engine(tag, res, model64.decoder.state_dict(), C.ref_conf(normalize_before), enc64, mask, N, T, model64.sos,
                          model64.eos, model32, enc32, lp)
    _rescored(model64, enc64, mask, N, model64.eos, info)
    return gpu, res, info


@pytest.mark.parametrize("N", [4, 10])
@pytest.mark.parametrize("normalize_before", [True, False], ids=["pre_norm", "post_norm"])
def test_kernels_backend_step_by_step_fp32(hip, normalize_before, N):
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    tag = f"{'pre' if normalize_before else 'post'}_N{N}_fp32"
    gpu, res, info = _run_case(tag, normalize_before, N, torch.float32)
    # None on the GPU is the kernels backend; two runs give the same trace
    enc, mask = case_inputs("batch")
    again = attention_beam_search(gpu, enc.float().cuda(), mask.cuda(), N, 0.6, return_trace=True)
    assert all(np.array_equal(again[0].trace[k], res[0].trace[k]) for k in ("parent", "token", "score"))
    assert [r.nbest for r in again] == [r.nbest for r in res] and again[0].stats["launches_per_step"] > 0
    # batching does not change an utterance's trace when the padded cap is held equal: the 70-frame utterance alone
    alone = attention_beam_search(gpu, enc[2:3].float().cuda(), mask[2:3].cuda(), N, 0.6, return_trace=True)
    n = min(alone[0].stats["steps"], info["steps"])
    assert n == alone[0].stats["steps"] or n == info["steps"]
    for k in ("parent", "token", "score"):           # (a GEMM's row does not depend on the rows beside it: the same bits)
        assert np.array_equal(alone[0].trace[k][:n], res[0].trace[k][:n, 2 * N:3 * N]), k
    assert alone[0].nbest == res[2].nbest or alone[0].stats["steps"] != info["steps"]


def test_kernels_backend_step_by_step_bf16(hip):
    _run_case("pre_N4_bf16", True, 4, torch.bfloat16)


def test_kernels_backend_one_frame_is_one_step(hip):
    """T' = 1: the cap is one step; max_len lowers the cap."""
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    gpu = search_model(True, dtype=torch.float32).cuda()
    enc, mask = case_inputs(0)
    res = attention_beam_search(gpu, enc.float().cuda(), mask.cuda(), 10, 0.0, return_trace=True)
    assert res[0].stats["steps"] == 1 and res[0].stats["host_reads"] == 1 and res[0].trace["parent"].shape == (1, 10)
    assert (res[0].trace["parent"] == 0).all() and len(set(res[0].trace["token"][0].tolist())) == 10
    enc, mask = case_inputs("batch")
    res = attention_beam_search(gpu, enc.float().cuda(), mask.cuda(), 10, 0.0, max_len=11, return_trace=True)
    assert res[0].stats["steps"] == 11 and res[0].stats["host_reads"] == 2 and res[0].stats["steps_issued"] == 11


def test_search_calls_no_library_gemm_and_reads_the_device_rarely(hip, monkeypatch):
    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile
    from paper_accurate_fast_cheap_amd.transformer import attn_search
    gpu = search_model(True, dtype=torch.float32).cuda()
    enc, mask = case_inputs("batch")
    enc, mask = enc.float().cuda(), mask.cuda()
    want = attn_search.attention_beam_search(gpu, enc, mask, 10, 0.6, max_len=20)               # (warm)

    def refuse(*a, **k):
        raise AssertionError("a library GEMM was called in the search")
    monkeypatch.setattr(F, "linear", refuse)
    monkeypatch.setattr(torch, "bmm", refuse)
    monkeypatch.setattr(torch, "matmul", refuse)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        got = attn_search.attention_beam_search(gpu, enc, mask, 10, 0.6, max_len=20)
        torch.cuda.synchronize()
    assert [r.nbest for r in got] == [r.nbest for r in want]
    names = [e.key for e in prof.key_averages()]
    for kernel in ("mha_step_kernel", "mha_rows_kernel", "beam_rows_kernel", "beam_utt_kernel"):
        assert any(kernel in n for n in names), (kernel, names)
    bad = [n for n in names if "Cijk_" in n or ("gemm" in n.lower() and "at::native" in n)
           or n in ("aten::mm", "aten::addmm", "aten::bmm")]
    assert not bad, bad
    st = got[0].stats
    assert st["steps"] == 20 and st["steps_issued"] == 20
    assert st["host_reads"] == 20 // attn_search.STEPS_PER_READ + 1                             # two looks and the final read
    # nothing inside a step reads the device: the only scalar reads of the call are the looks between the blocks
    items = sum(e.count for e in prof.key_averages() if e.key == "aten::_local_scalar_dense")
    assert items <= (st["host_reads"] - 1) * 2, items


def test_kernels_backend_refuses_what_it_cannot_take(hip, monkeypatch):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer import attn_search
    gpu = search_model(True, dtype=torch.float32).cuda()
    enc, mask = case_inputs("batch")
    enc, mask = enc.float().cuda(), mask.cuda()
    monkeypatch.setattr(attn_search, "CACHE_CAP_BYTES", 1 << 20)
    with pytest.raises(PafcError, match="set max_len"):
        attn_search.attention_beam_search(gpu, enc, mask, 10)
    assert attn_search.attention_beam_search(gpu, enc, mask, 10, max_len=8)[0].stats["cache_bytes"] <= 1 << 20
    with pytest.raises(PafcError, match="a beam of 17"):
        attn_search.attention_beam_search(gpu, enc, mask, 17)
    odd = C.model(True, dtype=torch.float32, attention_heads=4).cuda()                          # heads of 32 dimensions
    with pytest.raises(PafcError, match="the attention kernel takes 64"):
        attn_search.attention_beam_search(odd, enc, mask, 4)


def test_full_dimensions_and_decode_modes(hip):
    """d = 512, 8 heads, V = 5000, 3 blocks, B = 2, T' = 40, beam 10: the step-by-step check, and decode() on ASRModel and on
    Transducer equal to the direct call."""
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.attn_search import attention_beam_search
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from tests import attn_rescore_cases
    N, Tm, vocab, dim = 10, 40, 5000, 512
    g = torch.Generator().manual_seed(31)
    enc64 = torch.randn(2, Tm, dim, generator=g, dtype=torch.float64)
    lens = torch.tensor([Tm, 23])
    mask = (torch.arange(Tm)[None, :] < lens[:, None]).unsqueeze(1)
    old_v = attn_rescore_cases.V
    attn_rescore_cases.V = vocab                       # C.model builds its decoder and CTC at the module's V
    try:
        model64 = C.model(True, enc_out=enc64, attention_heads=8, linear_units=2048, num_blocks=3, r_num_blocks=1, seed=5)
    finally:
        attn_rescore_cases.V = old_v
    with torch.no_grad():
        model64.decoder.left_decoder.output_layer.bias[model64.eos] += 2.0     # nine steps, ended and live beams side by side
    import copy
    gpu = copy.deepcopy(model64).float().cuda()
    gpu.decoder.fp32_split_operands = False
    model32 = copy.deepcopy(model64).float()
    conf = dict(C.ref_conf(True, heads=8), num_blocks=3)
    res = attention_beam_search(gpu, enc64.float().cuda(), mask.cuda(), N, 0.6, backend="kernels", return_trace=True)
    info = _verify_engine("full_dims_fp32", res, model64.decoder.state_dict(), conf, enc64, mask, N, Tm, model64.sos, model64.eos,
                          model32, enc64.float(), 0.6)
    assert 5 <= info["steps"] < Tm and info["ended"].all()            # the search ran, and stopped on `done`
    _rescored(model64, enc64, mask, N, model64.eos, info)
    speech = torch.zeros(2, Tm, 2, device="cuda")
    out = gpu.decode(["attention_beam_search"], speech, lens.cuda(), beam_size=N, length_penalty=0.6)["attention_beam_search"]
    assert [r.nbest for r in out] == [r.nbest for r in res] and [r.nbest_scores for r in out] == [r.nbest_scores for r in res]
    tmodel = Transducer(vocab, 0, gpu.encoder, RNNPredictor(vocab, 32, 32, 0.0, 32, 1, dropout=0.0),
                        TransducerJoint(vocab, dim, 32, 32), ctc=CTC(vocab, dim), attention_decoder=gpu.decoder).eval().cuda()
    tmodel.sos, tmodel.eos = gpu.sos, gpu.eos
    out = tmodel.decode(["attention_beam_search"], speech, lens.cuda(), beam_size=N, length_penalty=0.6)["attention_beam_search"]
    assert [r.nbest for r in out] == [r.nbest for r in res]


def test_step_graph_replays_the_same_trace(hip):
    """step_graph=True: the first block of steps eager, the second captured, every later one a replay of that graph; the trace
    has the eager run's bits, also where the cap is no multiple of the block (the steps past it are frozen)."""
    from paper_accurate_fast_cheap_amd.transformer.attn_search import STEPS_PER_READ, attention_beam_search
    gpu = search_model(True, dtype=torch.float32).cuda()
    enc, mask = case_inputs("batch")
    enc, mask = enc.float().cuda(), mask.cuda()
    for N, max_len in ((10, None), (4, None), (10, 19)):
        eager = attention_beam_search(gpu, enc, mask, N, 0.6, max_len=max_len, return_trace=True)
        graphed = attention_beam_search(gpu, enc, mask, N, 0.6, max_len=max_len, return_trace=True, step_graph=True)
        st = graphed[0].stats
        parity_log.record(f"attn_search_step_graph_N{N}_cap{max_len}", mode=st["step_graph"], steps=st["steps"])
        assert eager[0].stats["step_graph"] == "eager" and st["step_graph"] == "replayed"
        assert st["steps"] == eager[0].stats["steps"] and st["steps_issued"] % STEPS_PER_READ == 0
        assert st["host_reads"] - 1 <= st["steps_issued"] / STEPS_PER_READ
        for k in ("parent", "token", "score"):
            assert np.array_equal(graphed[0].trace[k], eager[0].trace[k]), (N, max_len, k)
        assert [r.nbest for r in graphed] == [r.nbest for r in eager]
        assert [r.nbest_scores for r in graphed] == [r.nbest_scores for r in eager]
