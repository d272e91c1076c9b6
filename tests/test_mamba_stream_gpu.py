"""Streaming the uni-directional Mamba-2 encoder on the MI355X: the SSD scan with an initial and a final state
(pafc_mamba2_scan_state), Mamba2.forward_state, the layer / encoder carries on the module path and on the fused, graph-replayed
chunk step, the look-ahead streamer of the shipped non-causal YAML shape, and the streaming decoders on a Mamba-2 model.

Encoder-level errors are measured against a WHOLE-SEQUENCE fp32 CPU oracle assembled here from the oracle's public pieces
(oracle/encoder_oracle.py has no mamba_att branch): global_cmvn, conv2d_subsampling4, layer_norm, positionwise_ff,
conv_module in the layer order of encoder_oracle.conformer_layer, with oracle.mamba2_oracle.mamba2_forward as the slot."""
import math

import pytest
import torch

from oracle import encoder_oracle as EO
from oracle import mamba2_oracle as MO
from tests import parity_log, synth

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# the scan kernel
# ---------------------------------------------------------------------------------------------------------------------
def _scan_inputs(B, L, H, seed=9):
    """The inputs of test_mamba_ssd_scan_raw_vs_sequential (tests/test_mamba_gpu.py), same generator and order."""
    g = torch.Generator().manual_seed(seed)
    xbc = (torch.randn(B, L, H * 64 + 256, generator=g) * 0.5).to(torch.bfloat16)
    dt = torch.rand(B, L, H, generator=g) * 0.2 + 0.01
    la = -dt * (torch.rand(H, generator=g) * 8 + 0.5)
    return xbc, dt, la


def _sequential_f64(xbc, dt, la, H, s0=None, reverse=False):
    """h_t = a_t h_{t-1} + dt_t B_t x_t^T, y_t = C_t h_t in float64 -> (y (B, L, H, 64), h_final (B, H, 128, 64))."""
    B, L, _ = xbc.shape
    x = xbc[..., :H * 64].double().view(B, L, H, 64)
    Bm, Cm = xbc[..., H * 64:H * 64 + 128].double(), xbc[..., H * 64 + 128:].double()
    y = torch.zeros(B, L, H, 64, dtype=torch.float64)
    hf = torch.zeros(B, H, 128, 64, dtype=torch.float64)
    order = range(L - 1, -1, -1) if reverse else range(L)
    for b in range(B):
        for h in range(H):
            st = s0[b, h].double().clone() if s0 is not None else torch.zeros(128, 64, dtype=torch.float64)
            for t in order:
                st = st * math.exp(float(la[b, t, h])) + float(dt[b, t, h]) * torch.outer(Bm[b, t], x[b, t, h])
                y[b, t, h] = Cm[b, t] @ st
            hf[b, h] = st
    return y, hf


def _pieces(xbc, dt, la, H, cuts, reverse, D, s0=None, one_chunk=False):
    """The rows fed to the stateful scan piece by piece in recurrence order, state carried -> (y in time order, state).
    one_chunk: every piece walked by one wave per (batch, head), as the one-shot scan it is compared with bit for bit (the
    library's own choice cuts a piece longer than 64 steps into chunks, whose sums are formed in another order)."""
    from paper_accurate_fast_cheap_amd.hip_ops import mamba2_scan_state
    L = xbc.shape[1]
    assert sum(cuts) == L
    ys, s, a = [], s0, 0
    for n in cuts:
        lo, hi = (L - a - n, L - a) if reverse else (a, a + n)
        y, s = mamba2_scan_state(xbc[:, lo:hi].contiguous(), dt[:, lo:hi].contiguous(), la[:, lo:hi].contiguous(), H, s,
                                 reverse=reverse, D=D, chunk_len=n if one_chunk else 0)
        ys.append(y)
        a += n
    return torch.cat(ys[::-1] if reverse else ys, 1), s


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("form", ["f32", "skip_bf16"])
def test_scan_in_pieces_of_whole_blocks_is_the_one_chunk_scan_bit_for_bit(hip, form, reverse):
    """Derivable: a one-chunk wave walks its 16-step blocks in order with the fp32 state in registers; storing it and loading
    it again between blocks changes nothing.  So pieces whose lengths are multiples of 16 give the bits of the one-shot scan."""
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    B, H, L = 2, 3, 160
    xbc, dt, la = (t.cuda() for t in _scan_inputs(B, L, H, seed=21))
    D = (torch.rand(H, generator=torch.Generator().manual_seed(2)) + 0.5).cuda() if form == "skip_bf16" else None
    Lb = _lib.lib()
    if D is None:
        want = torch.empty(B, L, H * 64, dtype=torch.float32, device="cuda")
        rc = Lb.pafc_mamba2_scan_dir(B, L, H, _lib.ptr(xbc), xbc.shape[2], _lib.ptr(dt), _lib.ptr(la), _lib.ptr(want),
                                     int(reverse), L, None, 0, _lib.stream_of(xbc))
    else:
        want = torch.empty(B, L, H * 64, dtype=torch.bfloat16, device="cuda")
        rc = Lb.pafc_mamba2_scan_skip_bf16(B, L, H, _lib.ptr(xbc), xbc.shape[2], _lib.ptr(dt), _lib.ptr(la), _lib.ptr(D),
                                           _lib.ptr(want), int(reverse), L, None, 0, _lib.stream_of(xbc))
    assert rc == 0
    one_y, one_s = hip_ops.mamba2_scan_state(xbc, dt, la, H, None, reverse=reverse, D=D, chunk_len=L)
    assert torch.equal(one_y, want)
    for cuts in ((16, 48, 64, 32), (16,) * 10, (80, 80)):
        y, s = _pieces(xbc, dt, la, H, cuts, reverse, D, one_chunk=True)
        assert torch.equal(y, want), cuts
        assert torch.equal(s, one_s), cuts
    assert float(one_s.abs().max()) > 0


@pytest.mark.parametrize("reverse", [False, True])
def test_scan_with_arbitrary_cuts_against_the_float64_recurrence(hip, reverse):
    """Cuts that split 16-step blocks: bounded, with the bound test_mamba_ssd_scan_raw_vs_sequential holds the kernel to
    (max |err| / max |y| < 2e-4), for y and for the carried state; same inputs and seed."""
    B, L, H = 2, 150, 3
    xbc, dt, la = _scan_inputs(B, L, H)
    want_y, want_s = _sequential_f64(xbc, dt, la, H, reverse=reverse)
    for cuts in ((7, 1, 40, 3, 99), (150,), (1,) * 5 + (145,)):       # (pieces of 99 and more steps: several chunks)
        y, s = _pieces(xbc.cuda(), dt.cuda(), la.cuda(), H, cuts, reverse, None)
        ey = float((y.cpu().double().view(B, L, H, 64) - want_y).abs().max() / want_y.abs().max())
        es = float((s.cpu().double() - want_s).abs().max() / want_s.abs().max())
        print(f"cuts {cuts} reverse {reverse}: y {ey:.3g} state {es:.3g}")
        assert ey < 2e-4 and es < 2e-4, (cuts, ey, es)


@pytest.mark.parametrize("form", ["f32", "skip_bf16"])
def test_scan_of_many_chunks_from_a_nonzero_state(hip, form):
    """L = 3000 at B = 1 is walked as several chunks (NC > 1): pass B seeded from s_in, s_out stored by the last chunk's wave."""
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    B, L, H = 1, 3000, 3
    assert _lib.lib().pafc_mamba2_scan_workspace_bytes(B, L, H, 0) > 0
    xbc, dt, la = _scan_inputs(B, L, H, seed=33)
    s0 = torch.randn(B, H, 128, 64, generator=torch.Generator().manual_seed(4))
    want_y, want_s = _sequential_f64(xbc, dt, la, H, s0=s0)
    D = torch.rand(H, generator=torch.Generator().manual_seed(7)).cuda() if form == "skip_bf16" else None
    s_in = s0.cuda()
    y, s = hip_ops.mamba2_scan_state(xbc.cuda(), dt.cuda(), la.cuda(), H, s_in, D=D)
    assert torch.equal(s_in.cpu(), s0)                         # separate buffers: the carried state is left alone
    es = float((s.cpu().double() - want_s).abs().max() / want_s.abs().max())
    if D is None:
        ey = float((y.cpu().double().view(B, L, H, 64) - want_y).abs().max() / want_y.abs().max())
        print(f"many chunks {form}: y {ey:.3g} state {es:.3g}")
        assert ey < 2e-4
    else:     # the bf16 form against bf16(raw scan + D x), the bound test_mamba_scan_bf16_output_carries_the_skip_term uses
        y32, _ = hip_ops.mamba2_scan_state(xbc.cuda(), dt.cuda(), la.cuda(), H, s_in)
        want16 = (y32 + xbc.cuda()[..., :H * 64].float().view(B, L, H, 64).mul(D.view(1, 1, H, 1)).view(B, L, H * 64)).to(torch.bfloat16)
        torch.testing.assert_close(y.float(), want16.float(), rtol=2 ** -7, atol=1e-3)
    assert es < 2e-4
    y2, s2 = hip_ops.mamba2_scan_state(xbc.cuda(), dt.cuda(), la.cuda(), H, s_in, s_in, D=D)      # aliased, several chunks
    assert s2 is s_in and torch.equal(y2, y) and torch.equal(s2, s)


@pytest.mark.parametrize("reverse", [False, True])
def test_state_updated_where_it_lies_equals_separate_buffers(hip, reverse):
    from paper_accurate_fast_cheap_amd import hip_ops
    B, L, H = 2, 64, 3
    xbc, dt, la = (t.cuda() for t in _scan_inputs(B, L, H, seed=5))
    s0 = torch.randn(B, H, 128, 64, generator=torch.Generator().manual_seed(6)).cuda()
    D = torch.ones(H).cuda()
    for d in (None, D):
        y, s = hip_ops.mamba2_scan_state(xbc, dt, la, H, s0, reverse=reverse, D=d)
        buf = s0.clone()
        y2, s2 = hip_ops.mamba2_scan_state(xbc, dt, la, H, buf, buf, reverse=reverse, D=d)
        assert s2 is buf and torch.equal(y2, y) and torch.equal(buf, s) and not torch.equal(s, s0)
    y3, none = hip_ops.mamba2_scan_state(xbc, dt, la, H, s0, want_state=False)     # state not wanted
    assert none is None and torch.equal(y3, hip_ops.mamba2_scan_state(xbc, dt, la, H, s0)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------------------------------
def _cuts(L, how):
    if how == "ragged":                                       # pieces shorter than the conv cache first
        head = [1, 2, 3, 7, 1, 40, 3]
        return head + [L - sum(head)]
    return [how] * (L // how) + ([L % how] if L % how else [])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("d_model,L,B", [(128, 200, 2), (512, 130, 1)])
def test_block_forward_state_over_chunks_is_forward_of_the_whole_sequence(hip, dtype, d_model, L, B):
    """Mamba2.forward_state chunk after chunk (16, 64, ragged cuts with pieces shorter than the conv cache) against
    Mamba2.forward on the whole sequence; bounds between paths of this block as in tests/test_mamba_gpu.py: bf16 max <= 2^-5
    max(1, |ref| max), mean < 3e-3 (test_mamba_ssd_scan_kernel); fp32 rtol 1e-4 / atol 1e-5 (test_mamba_fused_glue_...)."""
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2
    torch.manual_seed(4)
    m = Mamba2(d_model, headdim=64).eval()
    with torch.no_grad():
        m.norm.weight.uniform_(0.5, 1.5)
        m.D.uniform_(0.5, 1.5)
    m = m.to(dtype).cuda()
    u = synth.randn((B, L, d_model), 6).to(dtype).cuda()
    with torch.no_grad():
        want = m(u)
        for how in (16, 64, "ragged"):
            outs, conv, ssm, a = [], None, None, 0
            cuts = _cuts(L, how)
            assert sum(cuts) == L
            for n in cuts:
                o, conv, ssm = m.forward_state(u[:, a:a + n], conv, ssm)
                outs.append(o)
                a += n
            got = torch.cat(outs, 1)
            assert got.dtype == dtype and conv.shape == (B, 3, m.d_inner + 256) and ssm.shape == (B, m.nheads, 128, 64)
            assert ssm.dtype == torch.float32 and ssm.is_contiguous()
            d = (got.float() - want.float()).abs()
            print(f"forward_state {dtype} d_model {d_model} cuts {how}: max {float(d.max()):.3g} mean {float(d.mean()):.3g}")
            if dtype == torch.float32:
                torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
            else:
                assert float(d.max()) <= 2 ** -5 * max(1.0, float(want.float().abs().max())), (how, float(d.max()))
                assert float(d.mean()) < 3e-3, (how, float(d.mean()))


def test_carry_has_one_layout_whatever_the_precision(hip):
    """The fp32 path maps the public (B, H, 128, 64) carry to and from the WKV kernel's two pre-decayed [value][key] states:
    its carry after a chunk is the bf16 kernel's carry on the same (bf16-valued) parameters and input.  Bounds from the number
    formats: the bf16 block rounds in_proj's output once (2^-9 relative: the conv carry, held to 2^-7) and the scan's inputs
    again after conv + SiLU; the state is a decayed sum of products of those, held to the block-level bound between the bf16
    and fp32 paths (2^-5 of the largest element, tests/test_mamba_gpu.py)."""
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2
    torch.manual_seed(8)
    m16 = Mamba2(128, headdim=64).eval().to(torch.bfloat16)
    m32 = Mamba2(128, headdim=64).eval()
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    m16, m32 = m16.cuda(), m32.cuda()
    u = synth.randn((2, 48, 128), 7).to(torch.bfloat16).cuda()
    with torch.no_grad():
        _, c16, s16 = m16.forward_state(u[:, :32])
        _, c32, s32 = m32.forward_state(u[:, :32].float())
        _, _, t16 = m16.forward_state(u[:, 32:], c16, s16)
        _, _, t32 = m32.forward_state(u[:, 32:].float(), c32, s32)
    for a, b in ((s16, s32), (t16, t32)):
        assert float((a - b).abs().max()) <= 2 ** -5 * float(b.abs().max())
    assert float((c16.float() - c32).abs().max()) <= 2 ** -7 * max(1.0, float(c32.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------
def _conf(causal, kernel):
    return dict(output_size=128, attention_heads=2, linear_units=256, num_blocks=2, input_layer="conv2d", normalize_before=True,
                cnn_module_kernel=kernel, causal=causal, use_cnn_module=True, cnn_module_norm="layer_norm",
                activation_type="swish", pos_enc_layer_type="rel_pos", selfattention_layer_type="mamba_att",
                rnn_att_version="mamba2", rnn_att_direction="uni")


def _mamba_encoder(causal, kernel, seed=31):
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    torch.manual_seed(seed)
    enc = ConformerEncoder(80, **_conf(causal, kernel)).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if ".norm_" in n and n.endswith("weight"):
                p.uniform_(0.7, 1.3)
            if ".norm_" in n and n.endswith("bias"):
                p.normal_(0, 0.1)
            if n.endswith("mamba.D") or n.endswith("mamba.norm.weight"):
                p.uniform_(0.5, 1.5)
    return enc


def encoder_oracle(xs, sd, conf):
    """Whole-sequence fp32 forward of the uni Mamba-2 Conformer encoder on the CPU, from the oracle's public pieces."""
    sd = {k: v.float() for k, v in sd.items()}
    xs = EO.global_cmvn(xs.float(), sd)
    x, _ = EO.conv2d_subsampling4(xs, torch.ones(xs.size(0), 1, xs.size(1), dtype=torch.bool), sd)
    empty = torch.ones((0, 0, 0), dtype=torch.bool)
    causal, k = bool(conf["causal"]), conf["cnn_module_kernel"]
    for i in range(conf["num_blocks"]):
        p = f"encoders.{i}."
        x = x + 0.5 * EO.positionwise_ff(EO.layer_norm(x, sd, p + "norm_ff_macaron."), sd, p + "feed_forward_macaron.")
        x = x + MO.mamba2_forward(EO.layer_norm(x, sd, p + "norm_mha."), sd, p + "self_attn.mamba.",
                                  headdim=conf["output_size"] // conf["attention_heads"])
        c = EO.conv_module(EO.layer_norm(x, sd, p + "norm_conv."), empty, sd, p + "conv_module.", k, causal)
        x = x + (c[0] if causal else c)
        x = x + 0.5 * EO.positionwise_ff(EO.layer_norm(x, sd, p + "norm_ff."), sd, p + "feed_forward.")
        x = EO.layer_norm(x, sd, p + "norm_final.")
    return EO.layer_norm(x, sd, "after_norm.")


def _accept(tag, got, whole, ref):
    """The form of tests/test_streaming_gpu.py:212-215: the stream's error against the oracle within 1.1 x (mean) / 1.5 x (max)
    of the whole-sequence GPU forward's error against the same oracle, plus 1e-3 / 1e-2.  Both are measured here and logged."""
    assert got.shape == ref.shape == whole.shape, (got.shape, whole.shape, ref.shape)
    e_s, e_w = (got.float().cpu() - ref).abs(), (whole.float().cpu() - ref).abs()
    parity_log.record(f"mamba streaming/{tag}", stream_vs_oracle_max=float(e_s.max()), stream_vs_oracle_mean=float(e_s.mean()),
                      whole_vs_oracle_max=float(e_w.max()), whole_vs_oracle_mean=float(e_w.mean()))
    print(f"[mamba streaming] {tag}: stream vs oracle max {float(e_s.max()):.4g} mean {float(e_s.mean()):.4g}; whole-sequence "
          f"forward vs oracle max {float(e_w.max()):.4g} mean {float(e_w.mean()):.4g}")
    assert float(e_s.mean()) <= 1.1 * float(e_w.mean()) + 1e-3, tag
    assert float(e_s.max()) <= 1.5 * float(e_w.max()) + 1e-2, tag


def _case(causal, kernel, prec, T, B=1, seed=908):
    enc = _mamba_encoder(causal, kernel)
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    enc = enc.to(dt)
    xs = synth.randn((B, T, 80), seed, 2.0).to(dt)
    ref = encoder_oracle(xs, {k: v.detach() for k, v in enc.state_dict().items()}, _conf(causal, kernel))
    enc = enc.cuda().eval()
    with torch.no_grad():
        whole, _ = enc(xs.cuda(), torch.full((B,), T, device="cuda"))
    return enc, xs.cuda(), whole, ref


@pytest.mark.parametrize("chunk", [16, 64])
@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_causal_encoder_streams_to_the_whole_sequence(hip, prec, chunk):
    """stream_chunks of the reduced uni Mamba-2 encoder with `causal: true`, eager and replayed from the captured graph (bf16:
    the fused chunk step with the state updated where it lies; fp32: the module path)."""
    enc, xs, whole, ref = _case(True, 15, prec, 4 * chunk * 9 + 3)
    with torch.no_grad():
        enc._carry_plans = None
        eager = enc.stream_chunks(xs, chunk, use_graph=False)
        graph = enc.stream_chunks(xs, chunk, use_graph=True)
    if prec == "bf16":
        assert enc._carry_last_fused and enc._carry_plans is not None           # the fused chunk step really ran
    else:
        assert not enc._carry_last_fused
    _accept(f"causal k15 {prec} chunk {chunk} eager", eager, whole, ref)
    _accept(f"causal k15 {prec} chunk {chunk} graph", graph, whole, ref)


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_three_streams_per_step_and_each_equals_the_stream_alone(hip, prec):
    """B = 3 streams through forward_chunk_carry.  bf16 (the fused chunk step, the serving path for concurrent streams): stream
    b of the batch equals the stream run alone bit for bit.  fp32 (module path): the fp32 projections pick their tiles by the
    row count, so a batch of three sums in another order than one stream; measured on the MI355X the two differ in the last
    bits, and they are held to the fp32 bound of this block (rtol 1e-4, atol 1e-5), printed before it is asserted."""
    chunk, B = 16, 3
    enc, xs, whole, ref = _case(True, 15, prec, 4 * chunk * 5 + 3, B=B)
    sub, ctx = enc.embed.subsampling_rate, enc.embed.right_context + 1
    stride, window = sub * chunk, (chunk - 1) * sub + ctx
    starts = list(range(0, xs.size(1) - ctx + 1, stride))

    def run(x):
        ys, state = [], None
        for c in starts:
            y, state = enc.forward_chunk_carry(x[:, c:min(c + window, x.size(1))], 0, state)
            ys.append(y)
        return torch.cat(ys, 1), state
    with torch.no_grad():
        got, state = run(xs)
        assert set(state[0]) == {"conv", "ssm", "cnn"}
        assert state[0]["conv"].shape == (B, 3, 256 + 256) and state[0]["ssm"].shape == (B, 4, 128, 64)
        assert state[0]["ssm"].dtype == torch.float32 and state[0]["cnn"].shape == (B, 128, 14)
        _accept(f"causal k15 {prec} forward_chunk_carry, 3 streams", got, whole, ref)
        for b in range(B):
            alone, st1 = run(xs[b:b + 1])
            if prec == "bf16":
                assert torch.equal(alone[0], got[b]), b
                assert torch.equal(st1[1]["ssm"][0], state[1]["ssm"][b]) and torch.equal(st1[1]["conv"][0], state[1]["conv"][b])
            else:
                print(f"fp32 stream {b} of 3 vs alone: max |diff| {float((alone[0] - got[b]).abs().max()):.3g}")
                torch.testing.assert_close(alone[0], got[b], rtol=1e-4, atol=1e-5)
                torch.testing.assert_close(st1[1]["ssm"][0], state[1]["ssm"][b], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("chunk", [16, 32])
@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_lookahead_stream_of_the_shipped_shape(hip, prec, chunk):
    """The shipped YAML's conv module -- non-causal, k = 31 -- through stream_chunks_lookahead (for Mamba-2 the eager loop over
    ConformerEncoderLayer.forward_lookahead: the fused look-ahead step serves the RWKV slot only)."""
    enc, xs, whole, ref = _case(False, 31, prec, 4 * chunk * 9 + 5)
    with torch.no_grad():
        got = enc.stream_chunks_lookahead(xs, chunk)
        y0, st = enc.forward_chunk_lookahead(xs[:, :(chunk - 1) * 4 + 7], None)
    assert y0.shape[1] == max(0, chunk - 15 * 2) and set(st[0]) == {"conv", "ssm", "cu", "x2"}
    _accept(f"look-ahead k31 {prec} chunk {chunk}", got, whole, ref)


# ---------------------------------------------------------------------------------------------------------------------
# the streaming decoders on a Mamba-2 model
# ---------------------------------------------------------------------------------------------------------------------
def _encoder_steps(enc, speech, chunk, causal):
    sub, ctx = enc.embed.subsampling_rate, enc.embed.right_context + 1
    stride, window = sub * chunk, (chunk - 1) * sub + ctx
    T = speech.size(1)
    starts = list(range(0, T - ctx + 1, stride))
    ys, state = [], None
    for i, c in enumerate(starts):
        xs = speech[:, c:min(c + window, T)]
        if causal:
            y, state = enc.forward_chunk_carry(xs, 0, state)
        else:
            y, state = enc.forward_chunk_lookahead(xs, state, final=(i == len(starts) - 1))
        ys.append(y)
    return ys, len(starts)


@pytest.mark.parametrize("mode", ["ctc_prefix_beam_search", "ctc_greedy_search"])
@pytest.mark.parametrize("causal", [True, False])
def test_stream_ctc_search_on_a_mamba_model_equals_offline_on_the_same_encoder_steps(hip, mode, causal):
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_greedy_search, ctc_prefix_beam_search
    torch.manual_seed(3)
    model = ASRModel(60, _mamba_encoder(causal, 15 if causal else 31), CTC(60, 128)).eval().cuda()
    chunk = 16
    speech = torch.randn(2, 4 * chunk * 6 + 3, 80, generator=torch.Generator().manual_seed(5)).cuda()
    seen = []
    with torch.no_grad():
        res = model.stream_ctc_search(speech, chunk, mode=mode, beam_size=4, on_partial=lambda i, part, com: seen.append(i))
        ys, n = _encoder_steps(model.encoder, speech, chunk, causal)
        pieces = [model.ctc_logprobs(y[:, a:a + chunk]) for y in ys for a in range(0, y.size(1), chunk)]
        whole = model.ctc_logprobs(torch.cat(ys, 1))
        assert torch.equal(torch.cat(pieces, 1), whole)
        lens = torch.full((2,), whole.size(1), device="cuda")
        ref = ctc_greedy_search(whole, lens, 0) if mode == "ctc_greedy_search" else ctc_prefix_beam_search(whole, lens, 4, None, 0)
    assert seen == list(range(n))
    assert [list(r.tokens) for r in res] == [list(r.tokens) for r in ref]
    if mode == "ctc_prefix_beam_search":
        assert [r.nbest for r in res] == [r.nbest for r in ref] and [r.nbest_scores for r in res] == [r.nbest_scores for r in ref]
        assert [r.times for r in res] == [r.times for r in ref]
    assert sum(len(r.tokens) for r in res) > 0


@pytest.mark.parametrize("causal", [True, False])
def test_stream_greedy_search_on_a_mamba_transducer_equals_offline_on_the_same_encoder_steps(hip, causal):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import batch_greedy_search
    from tests.conftest import load_golden
    from tests.test_rnnt_greedy import golden_model
    model = golden_model(load_golden("rnnt_greedy_c5"), "cuda")
    model.encoder = _mamba_encoder(causal, 15 if causal else 31).cuda().eval()
    chunk = 16
    speech = torch.randn(2, 4 * chunk * 6 + 3, 80, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        res = model.stream_greedy_search(speech, chunk)
        ys, _ = _encoder_steps(model.encoder, speech, chunk, causal)
        Y = torch.cat(ys, 1)
        ref = batch_greedy_search(model, Y, torch.full((2,), Y.size(1), device="cuda"), 64)
    assert [r.tokens for r in res] == [r.tokens for r in ref]
    assert [r.times for r in res] == [r.times for r in ref]
    assert [r.score for r in res] == [r.score for r in ref]
    assert sum(len(r.tokens) for r in res) > 0
