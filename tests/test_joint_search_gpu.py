"""Joint CTC/attention decoding on the GPU: the kernels of include/pafc_joint_search.h against float64, and
joint_decoding(backend="kernels") against the float64 restatement (tests/joint_search_ref.py) on the shared case of
tests/test_joint_search.py.

Bounds.  pafc_mha_step_paths is held to pafc_mha_step's bound: fp32, max |err| against float64 <= 4 x the max |err| of the same
formula run in float32 on the CPU; bf16, 4 x the error of the float32 CPU run on operands rounded to bf16 against float64 on the
unrounded ones.  pafc_joint_frame runs its recursion in float64 on the float32 inputs the restatement reads, so with a stand-in
decoder (a fixed float32 table of logits rows, indexed by a hash of the prefix, the same for both) beams, candidates, times and
trace must be exact and (p_nb, p_b), joint scores and confidences agree to rel 1e-12 / abs 1e-9 (the tolerance of
tests/test_search_gpu.py for float64 search scores); the inputs keep every frame's best beam + 1 joint scores 1e-6 apart and free
of ties, asserted first.  The engine: a search is a chain of near-ties, so a run is checked frame by frame along its own path:
the restatement continues from the engine's beam of every frame (`forced`); every kept prefix is one of the restatement's
candidates of that frame, they are distinct, each scores at least the float64 N-th best - eps, and the engine's score is
within eps of the float64 score of the same prefix, eps = dec_w * 8 * L * e32 + 1e-9 with L the prefix's tokens (the decoder
terms in its score) and e32 the largest per-token log-probability error of this project's decoder run in float32 on the CPU
against float64 on the case's own prefixes (for bf16: float32 on bf16-rounded weights and memory) -- the eps_i convention of
tests/test_attn_search_gpu.py; 1e-9 is the float64 tolerance above, for the CTC term."""
import copy
import math

import pytest
import torch

from tests import attn_rescore_cases as C
from tests import joint_search_ref as JR
from tests import parity_log
from tests.test_joint_search import ctc_case, joint_model, restated, shared_logp

pytestmark = pytest.mark.gpu

H, DK = 2, 64
D = H * DK
NEG = -math.inf


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def close(a, b, rel=1e-12, abs_=1e-9):
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= max(abs_, rel * max(abs(a), abs(b)))


# ---- pafc_mha_step_paths -----------------------------------------------------------------------------------------------------

def _path_attention(qkv, cache, path, lengths):
    """out[r, h] = softmax_j(q . k_j / 8) v_j over the cache rows path[r, :L - 1] and the row's own k, v, in qkv's dtype."""
    R = qkv.shape[0]
    out = torch.zeros(R, D, dtype=qkv.dtype)
    for r in range(R):
        past = cache[path[r, :lengths[r] - 1]]                                       # (L - 1, 2 D)
        for h in range(H):
            cs = slice(h * DK, (h + 1) * DK)
            k = torch.cat([past[:, cs], qkv[r:r + 1, D:2 * D][:, cs]], dim=0)
            v = torch.cat([past[:, D:][:, cs], qkv[r:r + 1, 2 * D:][:, cs]], dim=0)
            s = (k @ qkv[r, cs]) / math.sqrt(DK)
            out[r, cs] = torch.softmax(s, dim=-1) @ v
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mha_step_paths_against_float64(hip, dtype):
    from paper_accurate_fast_cheap_amd import hip_ops
    rows, W = 150, 131
    g = torch.Generator().manual_seed(17)
    tag = "fp32" if dtype == torch.float32 else "bf16"
    dev = "cuda"
    for R in (15, 1):
        lengths = ([1, 2, 64, 65, 66, 131, 1, 2, 64, 65, 66, 131, 3, 100, 17] if R == 15 else [66])
        need = [1 if r % 3 != 1 else 0 for r in range(R)] if R == 15 else [1]
        assert 0 in need or R == 1
        qkv = torch.randn(R, 3 * D, generator=g, dtype=torch.float64)
        cache = torch.randn(rows, 2 * D, generator=g, dtype=torch.float64)
        path = torch.randint(0, rows - R, (R, W), generator=g)                      # rows share ancestors at random
        new_row = torch.arange(rows - R, rows)                                       # the rows' own slots: nobody's ancestor
        want = _path_attention(qkv, cache, path, lengths)
        src = (lambda t: t.float()) if dtype == torch.float32 else (lambda t: t.bfloat16().float())
        cpu = _path_attention(src(qkv), src(cache), path, lengths)
        qbuf = torch.full((R, 3 * D + 8), float("nan"), dtype=dtype, device=dev)    # a pitch wider than 3 D
        qbuf[:, :3 * D] = qkv.to(dtype)
        # NaN wherever a row must not read: the pool's own slots, and every cache row no table names
        cbuf = torch.full((rows, 2 * D), float("nan"), dtype=dtype, device=dev)
        used = sorted({int(path[r, j]) for r in range(R) for j in range(lengths[r] - 1)})
        cbuf[used] = cache[used].to(dtype).to(dev)
        pbuf = torch.full((R, W + 5), 10 ** 9, dtype=torch.int32, device=dev)       # beyond a row's length: far outside the pool
        for r in range(R):
            pbuf[r, :lengths[r] - 1] = path[r, :lengths[r] - 1].to(torch.int32)
        len_t = torch.tensor(lengths, dtype=torch.int32, device=dev)
        need_t = torch.tensor(need, dtype=torch.int32, device=dev)
        new_t = new_row.to(torch.int32).to(dev)
        before = _bits(cbuf)
        out = torch.full((R, D), float("nan"), dtype=dtype, device=dev)
        hip_ops.mha_step_paths(qbuf[:, :3 * D], cbuf, pbuf, len_t, new_t, need_t, H, out=out)
        again = torch.full((R, D), float("nan"), dtype=dtype, device=dev)
        hip_ops.mha_step_paths(qbuf[:, :3 * D], cbuf, pbuf, len_t, new_t, need_t, H, out=again)
        torch.cuda.synchronize()
        # every row's output is defined (need or not) and the same bits twice
        assert torch.isfinite(out).all() and torch.equal(_bits(out), _bits(again))
        after = _bits(cbuf)
        for r in range(R):
            slot = int(new_row[r])
            if need[r]:
                assert torch.equal(after[slot], _bits(qkv[r, D:].to(dtype)))          # the row's own slot: its k | v
            else:
                assert torch.equal(after[slot], before[slot])                         # need = 0: nothing written
        keep = torch.ones(rows, dtype=torch.bool)
        keep[new_row] = False
        assert torch.equal(after[keep], before[keep])                                 # every other row untouched
        got = out.double().cpu()
        ek, ec = (got - want).abs().max().item(), (cpu.double() - want).abs().max().item()
        print(f"mha_step_paths {tag} R={R}: max|err| kernel {ek:.3e}, cpu yardstick {ec:.3e}, ratio {ek / ec:.3f}")
        parity_log.record(f"mha_step_paths_{tag}_R{R}", max_abs_err=ek, cpu_yardstick_err=ec, ratio=ek / ec)
        assert ec > 0 and ek <= 4 * ec, (R, ek, ec)
        # entries outside the pool are clamped into it: nothing outside is read (a clamped read of a NaN row shows as NaN, not
        # as a fault), and a slot outside the pool is not written
        wild = pbuf.clone()
        wild[:, 0] = torch.tensor([-5 if r % 2 else 10 ** 9 for r in range(R)], dtype=torch.int32, device=dev)
        frozen = _bits(cbuf)
        hip_ops.mha_step_paths(qbuf[:, :3 * D], cbuf, wild, len_t, torch.full_like(new_t, rows), need_t, H, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_bits(cbuf), frozen)


# ---- pafc_joint_frame with a stand-in decoder ---------------------------------------------------------------------------------

K_TABLE = 251


def _slot_of(prefix):
    h = 7
    for tok in prefix:
        h = (h * 1000003 + tok + 1) % K_TABLE
    return h


def frame_case(V, N, lens, seed, ctc_dtype=torch.float32, ctc_weight=0.5, threshold=1.0, bonus=0.5, blank_bias=2.0):
    """A random CTC input (B, T, V) with a blank bias and two near-certain blank frames per long utterance, a random float32
    table of logits rows, and the float64 restatement's search of every utterance with that table as its decoder."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    logits = torch.randn(B, T, V, generator=g, dtype=torch.float64) * 2.0
    logits[:, :, 0] += blank_bias + math.log(V / 53)
    for t in (5, 40):
        if t < T:
            logits[:, t, 0] += 12.0
    ctc = logits.log_softmax(-1).to(ctc_dtype)
    table = torch.randn(K_TABLE, V, generator=g, dtype=torch.float32) * 1.5
    sos = V - 1
    logp = lambda prefix: torch.log_softmax(table[_slot_of(prefix)].double(), dim=-1)                     # noqa: E731
    refs = []
    for b, n in enumerate(lens):
        s = JR.Search(ctc[b, :n].float(), logp, sos, N, ctc_weight, bonus, blank_threshold=threshold)
        s.run()
        refs.append(s)
    return dict(ctc=ctc, table=table, sos=sos, refs=refs, lens=lens, V=V, N=N, C=int(1.5 * N), ctc_weight=ctc_weight,
                threshold=threshold, bonus=bonus)


FRAME_CASES = {
    "V53_N4_B3": dict(V=53, N=4, lens=[1, 17, 70], seed=3, threshold=0.9),
    "V53_N1_B1_T17": dict(V=53, N=1, lens=[17], seed=4),
    "V53_N10_B1_T1": dict(V=53, N=10, lens=[1], seed=5),
    "V5000_N16_B3": dict(V=5000, N=16, lens=[70, 33, 1], seed=6, threshold=0.9),
    "V53_N4_B3_bf16": dict(V=53, N=4, lens=[17, 1, 9], seed=12, ctc_dtype=torch.bfloat16, threshold=0.9),      # (a seed free of bf16 ties)
    "V5000_N10_B1_T17": dict(V=5000, N=10, lens=[17], seed=7),
    "V53_N10_B3_ctc_only": dict(V=53, N=10, lens=[70, 17, 1], seed=8, ctc_weight=1.0, threshold=0.9),
}


def _drive(case, check=True):
    """Frame by frame: read the beam, build every slot's logits row from the table, run the kernel; with `check`, compare the
    state with the restatement after every frame.  Returns what identifies the run (for the bit-equality of two runs)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    dev = "cuda"
    V, N, Cn, lens, sos = case["V"], case["N"], case["C"], case["lens"], case["sos"]
    B, T, R = len(lens), max(lens), len(lens) * N
    dec_w = 1.0 - case["ctc_weight"]
    st = hip_ops.JointSearchState(B, N, Cn, T, sos, dev, decode=dec_w > 0)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    ctc = case["ctc"].to(dev).contiguous()
    hip_ops.joint_candidates(st, ctc, lens_t, 0, math.log(case["threshold"]))
    table = case["table"].to(dev)
    refs = case["refs"]
    # what a frame that is not executed must leave alone, by how the utterance's part is addressed
    watch = dict(node="slot", score="slot", path="slot", n_nodes="utt", executed="utt", nlive="utt", parent="utt", token="utt",
                 end="utt", ctc_conf="utt", row="utt", att_sum="utt", p_nb="table", p_b="table", stamp="table")

    def prefixes():
        node, parent, token = st.node.cpu(), st.parent.cpu(), st.token.cpu()
        out = []
        for r in range(R):
            b, n, toks = r // N, int(node[r]), []
            while n >= 0:
                toks.append(int(token[b, n]))
                n = int(parent[b, n])
            out.append(tuple(toks[::-1]))
        return out

    for t in range(T):
        pre = prefixes()
        logits = None
        if dec_w > 0:
            idx = torch.tensor([_slot_of(p) if p else 0 for p in pre], device=dev)
            logits = table[idx].contiguous()
        before = {k: getattr(st, k).clone() for k in watch} if check else None
        hip_ops.joint_frame(st, t, logits, V, lens_t, case["ctc_weight"], dec_w, case["bonus"], 0)
        if not check:
            continue
        post = prefixes()
        node, score = st.node.cpu(), st.score.cpu()
        cand = st.cand_tok.cpu()
        e = st.executed.cpu()
        for b, n in enumerate(lens):
            sl = slice(b * N, (b + 1) * N)
            rec = refs[b].frames[t] if t < n else None
            if rec is None or rec["skipped"]:
                # a frame past the utterance's length, or a skipped one, changes nothing for the utterance (need is cleared)
                assert (st.need[sl] == 0).all()
                for k, kind in watch.items():
                    a0, a1 = before[k], getattr(st, k)
                    pick = (lambda x: x[sl]) if kind == "slot" else (lambda x: x[b]) if kind == "utt" else (lambda x: x[:, b])
                    assert torch.equal(_bits64(pick(a0)), _bits64(pick(a1))), (k, t, b)
                if rec is not None:
                    assert int(st.skip[b, t]) == 1 and int(st.trace_exec[t, b]) == 0
                continue
            assert int(st.skip[b, t]) == 0 and int(st.trace_exec[t, b]) == 1
            assert cand[b, t].tolist() == rec["cands"], (t, b)                                  # the candidate set
            want = rec["beam"]
            live = [r for r in range(b * N, (b + 1) * N) if node[r] >= 0]
            assert [post[r] for r in live] == want, (t, b)                                      # the beam, in order
            assert st.trace_node[t, sl].cpu().tolist() == node[sl].tolist()
            par = int(e[b]) & 1
            for r, h in zip(live, want):
                nd = int(node[r])
                assert close(float(score[r]), rec["scored"][h]), (t, b, h, float(score[r]), rec["scored"][h])
                assert float(st.trace_score[t, r]) == float(score[r])
                nb, pb = rec["table"][h]
                assert close(float(st.p_nb[par, b, nd]), nb) and close(float(st.p_b[par, b, nd]), pb), (t, b, h)
                assert int(st.stamp[par, b, nd]) == int(e[b])
                end, (ctc_conf, att_conf) = rec["live"][h]                                      # as they stood after this frame
                assert int(st.start[b, nd]) == refs[b].starts[h][-1] and int(st.end[b, nd]) == end, (t, b, h)
                assert float(st.ctc_conf[b, nd]) == ctc_conf and close(float(st.att_conf[b, nd]), att_conf), (t, b, h)
    got = hip_ops.joint_collect(st)
    torch.cuda.synchronize()
    return st, {k: v.cpu() for k, v in got.items()}


def _bits64(t):
    t = t.contiguous()
    return t.view(torch.int64).cpu() if t.dtype == torch.float64 else (t.view(torch.int32).cpu() if t.dtype == torch.float32 else
                                                                       t.cpu())


@pytest.mark.parametrize("name", sorted(FRAME_CASES))
def test_joint_frame_with_a_stand_in_decoder(hip, name):
    case = frame_case(**FRAME_CASES[name])
    refs, N = case["refs"], case["N"]
    margins = [s.min_margin() for s in refs]
    print(f"joint_frame {name}: smallest margins {['%.2e' % m for m in margins]}")
    assert min(margins) > 1e-6
    assert not any(f["pre_beam_tie"] or f["score_tie"] for s in refs for f in s.frames if not f["skipped"])
    if "B3" in name:
        assert any(f["skipped"] for s in refs for f in s.frames) or case["threshold"] == 1.0
    st, got = _drive(case)
    worst = 0.0
    for b, s in enumerate(refs):
        want = s.result()
        rows = [r for r in range(b * N, (b + 1) * N) if got["len"][r] >= 0]
        if not s.scores:                                          # every frame skipped: the beam is still [sos]
            assert [int(got["len"][r]) for r in rows] == [0]
            continue
        assert [got["tok"][r, :got["len"][r]].tolist() for r in rows] == want["nbest"]
        assert [got["start"][r, :got["len"][r]].tolist() for r in rows] == want["nbest_times"]
        assert [got["end"][r, :got["len"][r]].tolist() for r in rows] == want["nbest_end_times"]      # snapshots included
        for r, conf in zip(rows, want["nbest_confidence"]):
            mine = [math.exp(max(float(got["ctc_conf"][r, j]), float(got["att_conf"][r, j]))) for j in range(len(conf))]
            assert all(close(x, y) for x, y in zip(mine, conf)), (b, r)
        for r, sc in zip(rows, want["nbest_scores"]):
            assert close(float(st.score[r]), sc)
            if math.isfinite(sc):
                worst = max(worst, abs(float(st.score[r]) - sc) / max(1.0, abs(sc)))
        # a prefix asks for a decode at most once, and never at the utterance's last frame
        assert int(st.evals[b]) <= 1 + N * case["lens"][b]
    parity_log.record(f"joint_frame_{name}", worst_rel_score_err=worst, smallest_margin=min(margins))
    # two runs are bit-equal
    st2, got2 = _drive(case, check=False)
    assert all(torch.equal(_bits64(got[k]), _bits64(got2[k])) for k in got)
    assert torch.equal(_bits64(st.score), _bits64(st2.score)) and torch.equal(st.trace_node, st2.trace_node)
    assert torch.equal(_bits64(st.trace_score), _bits64(st2.trace_score))


# ---- the engine ---------------------------------------------------------------------------------------------------------------

def _models(normalize_before, dtype):
    model64 = joint_model(normalize_before)
    gpu = joint_model(normalize_before, dtype=torch.float32).cuda()
    gpu.decoder.fp32_split_operands = False                       # exact fp32 products: what the float32 yardstick measures
    model32 = joint_model(normalize_before, dtype=torch.float32)
    enc64 = C.encoder_out()
    enc32 = enc64.float()
    if dtype == torch.bfloat16:
        gpu.decoder.to(torch.bfloat16)
        model32.decoder.to(torch.bfloat16).to(torch.float32)      # the float32 CPU run on bf16-rounded weights and memory
        enc32 = enc64.bfloat16().float()
    return model64, gpu, model32, enc64, enc32


def _e32(model32, enc32_b, logp64, prefixes):
    """The largest per-token error of the float32 CPU decoder against float64 over `prefixes` of one utterance."""
    left = model32.decoder.left_decoder
    mask = torch.ones(1, 1, enc32_b.size(0), dtype=torch.bool)
    worst = 0.0
    with torch.no_grad():
        for p in prefixes:
            ys = torch.tensor([list(p)])
            row = torch.log_softmax(left(enc32_b[None], mask, ys, torch.tensor([len(p)]))[0][0, -1], dim=-1)
            worst = max(worst, (row.double() - logp64(p)).abs().max().item())
    return worst


def _verify_forced(tag, results, lens, ctcs, logps, model32, enc32, sos, N, ctc_w, bonus, threshold=1.0):
    """Every frame of the engine's trace against the restatement continued from the engine's own beams."""
    dec_w = 1.0 - ctc_w
    out = []
    worst_slack = worst_drift = 0.0
    for b, res in enumerate(results):
        tr = res.trace
        forced = [[(sos,) + tuple(h) for h in beam] if ex else None for beam, ex in zip(tr["beam"], tr["executed"])]
        s = JR.Search(ctcs[b], logps[b], sos, N, ctc_w, bonus, blank_threshold=threshold)
        for t in range(lens[b]):
            s.time_step(t, forced[t])
            rec = s.frames[-1]
            assert rec["skipped"] == (not tr["executed"][t]), (tag, b, t)
        e32 = _e32(model32, enc32[b, :lens[b]], logps[b], list(s.rows)) if dec_w > 0 else 0.0
        assert e32 > 0 or dec_w == 0
        for t, rec in enumerate(s.frames):
            if rec["skipped"]:
                continue
            beam = forced[t]
            assert len(set(beam)) == len(beam) and 1 <= len(beam) <= N, (tag, b, t)              # distinct
            assert len(beam) == min(N, len(rec["scored"])), (tag, b, t)
            ranked = sorted(rec["scored"].values(), reverse=True)
            nth = ranked[len(beam) - 1]
            for h, mine in zip(beam, tr["score"][t]):
                assert h in rec["scored"], (tag, b, t, h)                                        # a candidate of the frame
                want = rec["scored"][h]
                eps = dec_w * 8 * (len(h) - 1) * e32 + 1e-9
                if math.isinf(want) or math.isinf(nth):
                    assert mine == want or not math.isinf(want), (tag, b, t, h)
                    continue
                worst_slack = max(worst_slack, (nth - want) / eps)
                worst_drift = max(worst_drift, abs(mine - want) / eps)
        want = s.result()
        assert res.nbest == want["nbest"] and res.nbest_times == want["nbest_times"], (tag, b)   # times: exact
        assert res.stats["nbest_end_times"] == want["nbest_end_times"] and res.end_times == want["nbest_end_times"][0], (tag, b)
        for mine, conf in zip(res.stats["nbest_tokens_confidence"], want["nbest_confidence"]):
            assert len(mine) == len(conf) and all(abs(x - y) <= 8 * e32 + 1e-12 for x, y in zip(mine, conf)), (tag, b)
        # a prefix is decoded at most once and at most 1 + N * T' times per utterance
        assert res.stats["decoder_evaluations"] <= 1 + N * lens[b] and res.stats["host_reads"] == 1
        assert res.stats["decoder_evaluations"] <= len(s.ever_on_beam) or dec_w == 0
        out.append(dict(search=s, e32=e32))
    print(f"{tag}: worst slack / eps {worst_slack:.3f}, worst |score - float64| / eps {worst_drift:.3f}, "
          f"e32 {[o['e32'] for o in out]}")
    parity_log.record(f"joint_search_{tag}", slack_over_eps=worst_slack, score_err_over_eps=worst_drift,
                      e32=max(o["e32"] for o in out))
    assert worst_slack <= 1.0 and worst_drift <= 1.0, (tag, worst_slack, worst_drift)
    return out


def _run_case(tag, normalize_before, N, dtype, ctc_w=0.5, bonus=0.5):
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    model64, gpu, model32, enc64, enc32 = _models(normalize_before, dtype)
    ctc = ctc_case(normalize_before)
    res = joint_decoding(gpu, enc64.float().cuda(), torch.tensor(C.LENS), ctc.cuda(), ctc_w, N, 1.5, bonus, backend="kernels",
                         return_trace=True)
    logps = [shared_logp(normalize_before, b) for b in range(3)]
    info = _verify_forced(tag, res, C.LENS, [ctc[b, :n] for b, n in enumerate(C.LENS)], logps, model32, enc32, model64.sos, N,
                          ctc_w, bonus)
    return gpu, res, info, enc64, ctc


@pytest.mark.parametrize("N", [4, 10])
@pytest.mark.parametrize("normalize_before", [True, False], ids=["pre_norm", "post_norm"])
def test_kernels_backend_frame_by_frame_fp32(hip, normalize_before, N):
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    tag = f"{'pre' if normalize_before else 'post'}_N{N}_fp32"
    gpu, res, info, enc64, ctc = _run_case(tag, normalize_before, N, torch.float32)
    enc, ctc_g, lens = enc64.float().cuda(), ctc.cuda(), torch.tensor(C.LENS)
    # None on the GPU is the kernels backend; two runs give the same bits
    again = joint_decoding(gpu, enc, lens, ctc_g, 0.5, N, 1.5, 0.5)
    assert [r.nbest for r in again] == [r.nbest for r in res] and [r.nbest_scores for r in again] == [r.nbest_scores for r in res]
    assert again[0].trace is None and again[0].stats["launches_per_frame"] > 0 and again[0].stats["host_reads"] == 1
    # the 70-frame utterance alone gives the bits of its slots in the batch
    alone = joint_decoding(gpu, enc[2:3], [70], ctc_g[2:3], 0.5, N, 1.5, 0.5, return_trace=True)[0]
    assert alone.nbest == res[2].nbest and alone.nbest_scores == res[2].nbest_scores and alone.nbest_times == res[2].nbest_times
    assert alone.trace["score"] == res[2].trace["score"] and alone.trace["beam"] == res[2].trace["beam"]
    # unforced: where the restatement's smallest margin is at least 2 eps, the engine's lists equal the unforced restatement's
    left_out = []
    for b, n in enumerate(C.LENS):
        ref = restated(normalize_before, N, b)
        eps = 0.5 * 8 * max(len(h) - 1 for f in ref.frames for h in f["beam"]) * info[b]["e32"] + 1e-9
        margin = ref.min_margin()
        print(f"{tag} utterance {b}: margin {margin:.2e}, 2 eps {2 * eps:.2e}")
        parity_log.record(f"joint_search_unforced_{tag}_utt{b}", margin=margin, two_eps=2 * eps)
        if margin < 2 * eps:
            left_out.append(b)
            continue
        want = ref.result()
        assert res[b].nbest == want["nbest"] and res[b].nbest_times == want["nbest_times"], (tag, b)
        assert res[b].stats["nbest_end_times"] == want["nbest_end_times"], (tag, b)
    assert len(left_out) <= 1 and (N != 4 or not any(C.LENS[b] in (1, 17) for b in left_out)), left_out


def test_kernels_backend_frame_by_frame_bf16(hip):
    _run_case("pre_N4_bf16", True, 4, torch.bfloat16)


def test_kernels_backend_ctc_only_and_skipped_frames(hip):
    """ctc_weight = 1: the decoder is never run (no decoder kernel is launched) and the scores are the float64 restatement's;
    blank_threshold = 0.9 skips the frames the restatement skips."""
    from torch.profiler import ProfilerActivity, profile
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    model64, gpu, _, enc64, _ = _models(True, torch.float32)
    ctc = ctc_case(True)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = joint_decoding(gpu, enc64.float().cuda(), C.LENS, ctc.cuda(), 1.0, 4, 1.5, 0.5, blank_threshold=0.9)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert any("frame_kernel" in n for n in names) and not any("mha_step_paths_kernel" in n or "mha_rows" in n for n in names)
    for b, r in enumerate(res):
        ref = restated(True, 4, b, 1.0, 0.5, 0.9)
        want = ref.result()
        assert r.nbest == want["nbest"] and r.nbest_times == want["nbest_times"] and r.stats["decoder_evaluations"] == 0
        assert all(close(x, y) for x, y in zip(r.nbest_scores, want["nbest_scores"]))
        assert r.stats["frames_skipped"] == sum(f["skipped"] for f in ref.frames)
    assert sum(r.stats["frames_skipped"] for r in res) >= 2


def test_search_calls_no_library_gemm_and_reads_the_device_once(hip, monkeypatch):
    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile
    from paper_accurate_fast_cheap_amd.transformer import joint_search
    gpu = joint_model(True, dtype=torch.float32).cuda()
    enc, ctc, lens = C.encoder_out().float().cuda(), ctc_case(True).cuda(), list(C.LENS)          # (lengths on the host)
    want = joint_search.joint_decoding(gpu, enc, lens, ctc, 0.5, 10)                              # (warm)

    def refuse(*a, **k):
        raise AssertionError("a library GEMM was called in the search")
    monkeypatch.setattr(F, "linear", refuse)
    monkeypatch.setattr(torch, "bmm", refuse)
    monkeypatch.setattr(torch, "matmul", refuse)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        got = joint_search.joint_decoding(gpu, enc, lens, ctc, 0.5, 10)
        torch.cuda.synchronize()
    assert [r.nbest for r in got] == [r.nbest for r in want]
    names = [e.key for e in prof.key_averages()]
    for kernel in ("mha_step_paths_kernel", "mha_rows_kernel", "frame_kernel", "candidates_kernel", "collect_kernel"):
        assert any(kernel in n for n in names), (kernel, names)
    bad = [n for n in names if "Cijk_" in n or ("gemm" in n.lower() and "at::native" in n)
           or n in ("aten::mm", "aten::addmm", "aten::bmm")]
    assert not bad, bad
    st = got[0].stats
    assert st["host_reads"] == 1 and st["launches_per_frame"] == 3 + 4 + 11 * 1 + 1 + 2
    assert sum(e.count for e in prof.key_averages() if e.key == "aten::_local_scalar_dense") == 0
    for b, r in enumerate(got):
        assert r.stats["decoder_evaluations"] <= 1 + 10 * C.LENS[b] and r.stats["frames"] == C.LENS[b]


def test_pools_are_written_once_and_only_where_a_prefix_was_decoded(hip):
    """The engine over NaN-filled pools: after the search the rows that hold numbers are exactly the rows the trie's nodes name
    (one per decoded prefix, each named once), every other row of every pool is still NaN, and the scores are finite: no frame
    read a row that nobody had written."""
    from paper_accurate_fast_cheap_amd.transformer import joint_search as JS
    gpu = joint_model(True, dtype=torch.float32).cuda()
    enc, ctc, N = C.encoder_out().float().cuda(), ctc_case(True).cuda(), 4
    eng = JS._Engine(gpu, enc, list(C.LENS), ctc, N, 6, 0.5, 0.5, 0.5, 0, 1.0)
    nan = float("nan")
    for pool in eng.caches + [eng.hidden]:
        pool.fill_(nan)
    eng.decode()
    for t in range(eng.T):
        eng.frame(t, t == eng.T - 1)
    torch.cuda.synchronize()
    st = eng.state
    named = st.row[st.row >= 0].cpu().tolist()
    assert len(named) == len(set(named)) == int(st.evals.sum())              # a prefix is decoded at most once
    assert all(r // eng.R <= int(st.executed[(r % eng.R) // N]) for r in named)      # round e follows executed frame e
    want = torch.zeros(eng.rows, dtype=torch.bool)
    want[named] = True
    for pool in eng.caches + [eng.hidden[:eng.rows]]:
        full = torch.isfinite(pool).all(dim=1).cpu()
        empty = torch.isnan(pool).all(dim=1).cpu()
        assert torch.equal(full, want) and torch.equal(empty, ~want)
    live = st.node >= 0
    assert torch.isfinite(st.score[live]).all() and int(live.sum()) == 3 * N


def test_an_utterance_without_frames_rides_along(hip):
    """encoder_lens may hold a 0: that utterance asks for no decode (not even of [sos]; its source attention has no keys and
    gives zeros, which nobody stores), returns the empty hypothesis at 0.0, and leaves the bits of the others alone."""
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    gpu = joint_model(True, dtype=torch.float32).cuda()
    enc, ctc = C.encoder_out().float().cuda(), ctc_case(True).cuda()
    want = joint_decoding(gpu, enc, list(C.LENS), ctc, 0.5, 4)
    got = joint_decoding(gpu, enc, [0] + list(C.LENS[1:]), ctc, 0.5, 4)
    assert got[0].tokens == [] and got[0].score == 0.0 and got[0].nbest == [[]] and got[0].stats["decoder_evaluations"] == 0
    assert got[0].stats["frames"] == 0 and got[0].stats["host_reads"] == 1
    for a, b in zip(got[1:], want[1:]):
        assert a.nbest == b.nbest and a.nbest_scores == b.nbest_scores and a.nbest_times == b.nbest_times
        assert a.stats["decoder_evaluations"] == b.stats["decoder_evaluations"] > 1
        assert all(math.isfinite(x) for x in a.nbest_scores)
    only = joint_decoding(gpu, enc[:1], [0], ctc[:1], 0.5, 4)[0]                 # and a batch of nothing but such an utterance
    assert only.tokens == [] and only.score == 0.0 and only.stats["decoder_evaluations"] == 0


def test_kernels_backend_refuses_what_it_cannot_take(hip, monkeypatch):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer import joint_search
    gpu = joint_model(True, dtype=torch.float32).cuda()
    enc, ctc, lens = C.encoder_out().float().cuda(), ctc_case(True).cuda(), C.LENS
    monkeypatch.setattr(joint_search, "CACHE_CAP_BYTES", 1 << 20)
    with pytest.raises(PafcError, match="CACHE_CAP_BYTES"):
        joint_search.joint_decoding(gpu, enc, lens, ctc, 0.5, 10)
    with pytest.raises(PafcError, match="a beam of 17"):
        joint_search.joint_decoding(gpu, enc, lens, ctc, 0.5, 17)
    odd = C.model(True, dtype=torch.float32, attention_heads=4).cuda()                          # heads of 32 dimensions
    with pytest.raises(PafcError, match="the attention kernel takes 64"):
        joint_search.joint_decoding(odd, enc, lens, ctc, 0.5, 4)


def test_full_dimensions_and_decode_modes(hip):
    """d = 512, 8 heads, V = 5000, 3 blocks, B = 2, T' = 40, beam 10: the frame-by-frame check, and decode() on ASRModel and on
    Transducer equal to the direct call."""
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.joint_search import joint_decoding
    from tests import attn_rescore_cases
    N, Tm, vocab, dim = 10, 40, 5000, 512
    g = torch.Generator().manual_seed(31)
    enc64 = torch.randn(2, Tm, dim, generator=g, dtype=torch.float64)
    lens = [Tm, 23]
    old_v = attn_rescore_cases.V
    attn_rescore_cases.V = vocab                       # C.model builds its decoder and CTC at the module's V
    try:
        model64 = C.model(True, enc_out=enc64, attention_heads=8, linear_units=2048, num_blocks=3, r_num_blocks=1, seed=5)
    finally:
        attn_rescore_cases.V = old_v
    with torch.no_grad():
        model64.ctc.ctc_lo.bias[0] += 5.5              # blank-dominated at V = 5000
    gpu = copy.deepcopy(model64).float().cuda()
    gpu.decoder.fp32_split_operands = False
    model32 = copy.deepcopy(model64).float()
    conf = dict(C.ref_conf(True, heads=8), num_blocks=3)
    with torch.no_grad():
        ctc = model64.ctc.log_softmax(enc64).float()
    res = joint_decoding(gpu, enc64.float().cuda(), lens, ctc.cuda(), 0.5, N, 1.5, 0.5, backend="kernels", return_trace=True)
    logps = []
    for b in range(2):
        inner, memo = JR.decoder_logp(model64.decoder.state_dict(), conf, enc64[b, :lens[b]]), {}
        logps.append(lambda p, inner=inner, memo=memo: memo[p] if p in memo else memo.setdefault(p, inner(p)))
    info = _verify_forced("full_dims_fp32", res, lens, [ctc[b, :n] for b, n in enumerate(lens)], logps, model32, enc64.float(),
                          model64.sos, N, 0.5, 0.5)
    assert any(len(h) >= 1 for r in res for h in r.nbest) and all(i["search"].rows for i in info)
    speech = torch.zeros(2, Tm, 2, device="cuda")
    lens_t = torch.tensor(lens).cuda()
    kw = dict(beam_size=N, ctc_weight=0.5, length_penalty=0.5)
    want = joint_decoding(gpu, enc64.float().cuda(), lens, gpu.ctc_logprobs(enc64.float().cuda()), 0.5, N, 1.5, 0.5)
    out = gpu.decode(["joint_decoding"], speech, lens_t, **kw)["joint_decoding"]
    # (the CTC head runs on the framework's GEMM, whose bits differ between two calls on this size: the lists are exact, the
    # scores agree to the float32 rounding of the CTC log-probabilities)
    assert [r.nbest for r in out] == [r.nbest for r in want] and [r.nbest_times for r in out] == [r.nbest_times for r in want]
    assert all(a.nbest_scores == pytest.approx(b.nbest_scores, rel=1e-6) for a, b in zip(out, want))
    tmodel = Transducer(vocab, 0, gpu.encoder, RNNPredictor(vocab, 32, 32, 0.0, 32, 1, dropout=0.0),
                        TransducerJoint(vocab, dim, 32, 32), ctc=gpu.ctc, attention_decoder=gpu.decoder).eval().cuda()
    tmodel.sos, tmodel.eos = gpu.sos, gpu.eos
    out = tmodel.decode(["joint_decoding"], speech, lens_t, **kw)["joint_decoding"]
    assert [r.nbest for r in out] == [r.nbest for r in want] and [r.nbest_times for r in out] == [r.nbest_times for r in want]
