"""The WKV-6 kernels (csrc/wkv6.hip, csrc/wkv6_mfma.inc) against the float64 recurrence of tests/wkv_ref.py, term by term, at
their edge shapes: every forward path and switch, the backward with and without a state, and properties that need no reference
(batch rows independent, runs repeatable, nothing read or written out of range).  The acceptance rules and their constants live
in tests/wkv_ref.py; the observed ratios go to the parity log.  Head size 64, so C = 64 H.  GPU only."""
import functools

import pytest
import torch

from tests import wkv_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
FWD = R.matrix(R.FORWARD_CASES, R.FORWARD_ALL_RECIPES)
BWD = R.matrix(R.BACKWARD_CASES, R.BACKWARD_ALL_RECIPES)
# chunks the launcher must cut each case into (chunk lengths are rounded up to 16 steps; 0 = the library's choice)
FWD_CHUNKS = {(1, 1, 1, 0): 1, (2, 15, 2, 0): 1, (2, 16, 2, 0): 1, (2, 17, 2, 0): 1, (1, 33, 1, 16): 3, (2, 83, 3, 32): 3,
              (1, 64, 1, 16): 4, (2, 45, 3, 24): 2, (1, 40, 8, 16): 3, (3, 37, 2, 10 ** 6): 1, (1, 130, 2, 0): 3}
BWD_CHUNKS = {(1, 1, 1, 0): 1, (2, 2, 1, 0): 1, (2, 17, 2, 0): 1, (2, 37, 2, 8): 3, (1, 83, 3, 32): 3, (1, 150, 2, 0): 3,
              (1, 1100, 1, 0): 18}


def _dev(ts):
    return [t.cuda() for t in ts]


def _tag(*parts):
    return "-".join(str(p).replace("torch.", "") for p in parts)


def _assert_forward_path(hip, B, T, H, chunk, ndir=1):
    """The path meant is the path that runs: the workspace the launcher asks for is that of the expected number of chunks."""
    nc = FWD_CHUNKS[(B, T, H, chunk)]
    if (B, T, H, chunk) == (1, 130, 2, 0):
        assert hip.pafc_wkv6_pick_chunk_len(B, T, 64 * H, H, ndir) == 64
    want = 0 if nc == 1 else 4 * ndir * B * H * nc * (64 * 64 + 64)
    assert hip.pafc_wkv6_fwd_workspace_bytes(B, T, 64 * H, H, ndir, chunk) == want


def _assert_backward_path(hip, B, T, H, chunk):
    nc = BWD_CHUNKS[(B, T, H, chunk)]
    floats = 2 * B * T * 64 * H + 2 * B * H * 64 * 64 + B * H * 64 * 64 + (2 * B * H * nc * (64 * 64 + 64) if nc > 1 else 0)
    assert hip.pafc_wkv6_bwd_workspace_bytes(B, T, 64 * H, H, chunk) == 4 * floats


def _accept_y(got, y, yabs, name):
    got = got.cpu()
    if got.dtype == BF16:
        R.accept_y_bf16(got, y, R.REL_Y * yabs, name)
    else:
        R.accept_y(got, y, yabs, name)


# ---- forward ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk,recipe", FWD)
def test_forward(hip, B, T, H, chunk, recipe, dtype, reverse):
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward
    _assert_forward_path(hip, B, T, H, chunk)
    a, y, _, yabs, _ = R.forward_case(B, T, H, dtype, recipe, reverse)
    got = wkv6_forward(*_dev(a), reverse=reverse, chunk_len=chunk)
    _accept_y(got, y, yabs, "wkv6_f64 forward [" + _tag(B, T, H, chunk, recipe, dtype, "rev" if reverse else "fwd") + "]")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk,recipe", FWD)
def test_forward_from_a_state_to_a_state(hip, B, T, H, chunk, recipe, dtype, reverse):
    """s_in / want_state; where the sequence is one chunk also in place (s_out = s_in): the same bits as out of place."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward
    _assert_forward_path(hip, B, T, H, chunk)
    a, y, S, yabs, Sabs = R.forward_case(B, T, H, dtype, recipe, reverse, state=True)
    g = _dev(a)
    got, s_out = wkv6_forward(*g[:5], s_in=g[5], want_state=True, reverse=reverse, chunk_len=chunk)
    name = "wkv6_f64 forward state [" + _tag(B, T, H, chunk, recipe, dtype, "rev" if reverse else "fwd") + "]"
    _accept_y(got, y, yabs, name + " y")
    R.accept_state(s_out.cpu(), S, Sabs, name + " S")
    assert torch.equal(g[5].cpu(), a[5])                     # the carried state is an input
    if FWD_CHUNKS[(B, T, H, chunk)] == 1:
        state = g[5].clone()
        got2, s2 = wkv6_forward(*g[:5], s_in=state, s_out=state, reverse=reverse, chunk_len=chunk)
        assert s2.data_ptr() == state.data_ptr() and torch.equal(got2, got) and torch.equal(s2, s_out)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk,recipe", [c for c in FWD if c[1] > 61])
def test_cut_and_carried(hip, B, T, H, chunk, recipe, dtype, reverse):
    """The first 61 steps of the walk (not a multiple of 16), then the rest from the state they leave: against float64, not
    against the uncut kernel run."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward
    a, y, S, yabs, Sabs = R.forward_case(B, T, H, dtype, recipe, reverse, state=True)
    g = _dev(a)
    first, rest = (slice(T - 61, T), slice(0, T - 61)) if reverse else (slice(0, 61), slice(61, T))
    cut = lambda sl: [t[:, sl].contiguous() for t in g[:4]]
    y1, s1 = wkv6_forward(*cut(first), g[4], s_in=g[5], want_state=True, reverse=reverse, chunk_len=chunk)
    y2, s2 = wkv6_forward(*cut(rest), g[4], s_in=s1, want_state=True, reverse=reverse, chunk_len=chunk)
    got = torch.cat([y2, y1] if reverse else [y1, y2], 1)
    name = "wkv6_f64 cut 61 [" + _tag(B, T, H, chunk, recipe, dtype, "rev" if reverse else "fwd") + "]"
    _accept_y(got, y, yabs, name + " y")
    R.accept_state(s2.cpu(), S, Sabs, name + " S")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk,recipe", FWD)
def test_both_directions_in_one_launch(hip, B, T, H, chunk, recipe, dtype):
    """wkv6_forward_bidir: different operands per direction."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward_bidir
    _assert_forward_path(hip, B, T, H, chunk, ndir=2)
    f, yf, _, yfabs, _ = R.forward_case(B, T, H, dtype, recipe, False)
    b, yb, _, ybabs, _ = R.forward_case(B, T, H, dtype, recipe, True, variant=1)
    gf, gb = wkv6_forward_bidir(_dev(f), _dev(b), chunk_len=chunk)
    name = "wkv6_f64 bidir [" + _tag(B, T, H, chunk, recipe, dtype) + "]"
    _accept_y(gf, yf, yfabs, name + " fwd")
    _accept_y(gb, yb, ybabs, name + " rev")


@functools.lru_cache(maxsize=None)
def _bias_case(B, T, H, dtype, recipe, reverse, variant):
    """A case whose decay is w + bias, rounded to the operands' dtype where the reference's `time_decay + lora` rounds it
    (tests/test_wkv6_gpu.py::test_decay_bias_inside_the_scan...): the reference reads the rounded sum."""
    a = R.forward_case(B, T, H, dtype, recipe, reverse, variant=variant)[0]
    g = torch.Generator().manual_seed(990 + variant + 7 * T)
    wb = (torch.randn(64 * H, generator=g) * 0.7).to(dtype)
    w = (a[3].float() + wb.float()).to(dtype)
    with torch.no_grad():
        y, _ = R.recurrence(a[0], a[1], a[2], w, a[4], None, reverse)
        yabs, _ = R.abs_recurrence(a[0], a[1], a[2], w, a[4], None, reverse)
    return a, wb, y, yabs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk,recipe", FWD)
def test_both_directions_with_a_decay_bias(hip, B, T, H, chunk, recipe, dtype):
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward_bidir
    f, wbf, yf, yfabs = _bias_case(B, T, H, dtype, recipe, False, 0)
    b, wbb, yb, ybabs = _bias_case(B, T, H, dtype, recipe, True, 1)
    gf, gb = wkv6_forward_bidir(_dev(f), _dev(b), chunk_len=chunk, w_bias=(wbf.cuda(), wbb.cuda()))
    name = "wkv6_f64 bidir w_bias [" + _tag(B, T, H, chunk, recipe, dtype) + "]"
    _accept_y(gf, yf, yfabs, name + " fwd")
    _accept_y(gb, yb, ybabs, name + " rev")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk,recipe", FWD)
def test_valu_formulation(hip, monkeypatch, B, T, H, chunk, recipe, dtype, reverse):
    """PAFC_WKV6_IMPL=valu: the register / LDS formulation of the same passes, from a state to a state."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward
    monkeypatch.setenv("PAFC_WKV6_IMPL", "valu")
    a, y, S, yabs, Sabs = R.forward_case(B, T, H, dtype, recipe, reverse, state=True)
    g = _dev(a)
    got, s_out = wkv6_forward(*g[:5], s_in=g[5], want_state=True, reverse=reverse, chunk_len=chunk)
    name = "wkv6_f64 valu [" + _tag(B, T, H, chunk, recipe, dtype, "rev" if reverse else "fwd") + "]"
    _accept_y(got, y, yabs, name + " y")
    R.accept_state(s_out.cpu(), S, Sabs, name + " S")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("B,T,H,chunk,recipe", FWD)
def test_bf16_time_lane_passes(hip, monkeypatch, B, T, H, chunk, recipe, reverse):
    """PAFC_WKV6_PASS_A=lt and PAFC_WKV6_PASS_C=lt: bf16 I/O on the time-lane kernels instead of the channel-lane ones."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward
    monkeypatch.setenv("PAFC_WKV6_PASS_A", "lt")
    monkeypatch.setenv("PAFC_WKV6_PASS_C", "lt")
    a, y, S, yabs, Sabs = R.forward_case(B, T, H, BF16, recipe, reverse, state=True)
    g = _dev(a)
    got, s_out = wkv6_forward(*g[:5], s_in=g[5], want_state=True, reverse=reverse, chunk_len=chunk)
    name = "wkv6_f64 bf16 lt [" + _tag(B, T, H, chunk, recipe, "rev" if reverse else "fwd") + "]"
    _accept_y(got, y, yabs, name + " y")
    R.accept_state(s_out.cpu(), S, Sabs, name + " S")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T", [17, 33, 48, 64])
def test_few_blocks_kernel(hip, monkeypatch, T, reverse):
    """PAFC_WKV6_FEW=1: the 2-4 blocks of a short bf16 sequence side by side, carried state in, new state out, also in place."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_forward
    B, H = 2, 2
    assert hip.pafc_wkv6_fwd_workspace_bytes(B, T, 64 * H, H, 1, 0) == 0          # one chunk: the few-blocks kernel's condition
    monkeypatch.setenv("PAFC_WKV6_FEW", "1")
    a, y, S, yabs, Sabs = R.forward_case(B, T, H, BF16, "mid", reverse, state=True)
    g = _dev(a)
    got, s_out = wkv6_forward(*g[:5], s_in=g[5], want_state=True, reverse=reverse)
    name = "wkv6_f64 few blocks [" + _tag(T, "rev" if reverse else "fwd") + "]"
    _accept_y(got, y, yabs, name + " y")
    R.accept_state(s_out.cpu(), S, Sabs, name + " S")
    state = g[5].clone()
    got2, s2 = wkv6_forward(*g[:5], s_in=state, s_out=state, reverse=reverse)
    assert s2.data_ptr() == state.data_ptr() and torch.equal(got2, got) and torch.equal(s2, s_out)


# ---- backward -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk,recipe", BWD)
def test_backward(hip, B, T, H, chunk, recipe, dtype, reverse, state):
    """wkv6_backward without a state, and with s_in / want_gs: gr, gk, gv, gu, gs by accept_grad, gw by accept_gw."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_backward
    _assert_backward_path(hip, B, T, H, chunk)
    a, gy, ref, mag, oerr = R.backward_case(B, T, H, dtype, recipe, reverse, state)
    g = _dev(a)
    kw = dict(s_in=g[5], want_gs=True) if state else {}
    got = [t.cpu() for t in wkv6_backward(*g[:5], gy.cuda(), reverse=reverse, chunk_len=chunk, **kw)]
    name = "wkv6_f64 backward [" + _tag(B, T, H, chunk, recipe, dtype, "rev" if reverse else "fwd", "s" if state else "z") + "]"
    for key, t in zip(("gr", "gk", "gv"), got[:3]):
        R.accept_grad(f"{name} {key}", t, ref[key], mag[key])
    R.accept_grad(f"{name} gu", got[4], ref["gu_b"], mag["gu_b"], batch_sum=True)
    if state:
        R.accept_grad(f"{name} gs", got[5], ref["gs"], mag["gs"])
    R.accept_gw(got[3], ref["gw"], mag["gw"], oerr, f"{name} gw", zero_steps=R.gw_zero_steps(T, state, reverse))


# ---- properties that need no reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_batch_rows_are_independent_and_runs_repeat(hip, dtype, reverse):
    """Row b of a batched call equals that row run alone, bit for bit, at a forced chunk length (the library's own choice
    depends on the batch), forward and backward; and a second run gives the same bits."""
    from paper_accurate_fast_cheap_amd.rwkv_v6.wkv6_op import wkv6_backward, wkv6_forward
    B, T, H, chunk = 3, 83, 2, 32
    a = _dev(R.make_inputs(B, T, H, 8100, dtype, "mid", state=True))
    gy = R.make_gy(B, T, H, 8101, dtype).cuda()
    fwd = lambda x: wkv6_forward(*x[:5], s_in=x[5], want_state=True, reverse=reverse, chunk_len=chunk)
    bwd = lambda x, gy_: wkv6_backward(*x[:5], gy_, reverse=reverse, chunk_len=chunk, s_in=x[5], want_gs=True)
    y, s = fwd(a)
    grads = bwd(a, gy)
    for t, t2 in zip((y, s) + tuple(grads), fwd(a) + tuple(bwd(a, gy))):
        assert torch.equal(t, t2)
    for b in range(B):
        row = [t[b:b + 1].contiguous() for t in a[:4]] + [a[4], a[5][b:b + 1].contiguous()]
        yb, sb = fwd(row)
        assert torch.equal(yb[0], y[b]) and torch.equal(sb[0], s[b]), b
        gb = bwd(row, gy[b:b + 1].contiguous())
        for i in (0, 1, 2, 3, 5):          # gr, gk, gv, gw, gs (gu is summed over the batch)
            assert torch.equal(gb[i][0], grads[i][b]), (b, i)


PAD = 4096        # guard elements on each side: 8 or 16 KiB, further than any row or tile the kernels address


class _Guarded:
    """A contiguous, 16-byte aligned view inside a NaN-filled flat buffer, NaN on both sides; `data` None: preset to NaN."""

    def __init__(self, shape, dtype, data=None):
        n = 1
        for d in shape:
            n *= d
        self.flat = torch.full((2 * PAD + n,), float("nan"), dtype=dtype, device="cuda")
        self.view = self.flat[PAD:PAD + n].view(shape)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()
        if data is not None:
            self.view.copy_(data)
        self.n = n
        self.bits = self._bits().clone()

    def _bits(self):
        return self.flat.view(torch.int32 if self.flat.element_size() == 4 else torch.int16)

    def guards_intact(self):
        now = self._bits()
        return torch.equal(now[:PAD], self.bits[:PAD]) and torch.equal(now[PAD + self.n:], self.bits[PAD + self.n:])

    def unchanged(self):
        return torch.equal(self._bits(), self.bits)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,chunk", [(2, 17, 2, 0), (2, 83, 3, 32)])
def test_nothing_is_read_or_written_out_of_range(hip, B, T, H, chunk, dtype, reverse):
    """Operands, outputs and workspaces sit between NaN guards; outputs and workspaces start as NaN.  A read outside an operand
    (or of a workspace slot nobody wrote) makes an output non-finite, a write outside an output changes a guard's bits."""
    from paper_accurate_fast_cheap_amd import _lib
    P = _lib.ptr
    C = 64 * H
    code = _lib.dtype_code(dtype)
    a = R.make_inputs(B, T, H, 8200 + T, dtype, "mid", state=True)
    gy = R.make_gy(B, T, H, 8300 + T, dtype)
    ins = [_Guarded(t.shape, t.dtype, t) for t in a + [gy]]
    r, k, v, w, u, s_in, gyg = ins
    stream = _lib.stream_of(r.view)

    y, s_out = _Guarded((B, T, C), dtype), _Guarded((B, H, 64, 64), F32)
    nbytes = hip.pafc_wkv6_fwd_workspace_bytes(B, T, C, H, 1, chunk)
    ws = _Guarded((max(nbytes, 16) // 4,), F32)
    rc = hip.pafc_wkv6_forward_state(code, B, T, C, H, P(r.view), P(k.view), P(v.view), P(w.view), P(u.view), P(y.view),
                                     P(s_in.view), P(s_out.view), int(reverse), chunk, P(ws.view) if nbytes else P(None), nbytes, stream)
    _lib.check(rc, "pafc_wkv6_forward_state")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.view).all()) and bool(torch.isfinite(s_out.view).all())
    assert all(g.guards_intact() for g in (y, s_out, ws)) and all(g.unchanged() for g in ins)

    outs = [_Guarded((B, T, C), dtype) for _ in range(4)] + [_Guarded((B, C), dtype), _Guarded((B, H, 64, 64), F32)]
    gr, gk, gv, gw, gu, gs = outs
    nbytes = hip.pafc_wkv6_bwd_workspace_bytes(B, T, C, H, chunk)
    ws = _Guarded((nbytes // 4,), F32)
    rc = hip.pafc_wkv6_backward_state(code, B, T, C, H, P(r.view), P(k.view), P(v.view), P(w.view), P(u.view), P(s_in.view),
                                      P(gyg.view), P(gr.view), P(gk.view), P(gv.view), P(gw.view), P(gu.view), P(gs.view),
                                      int(reverse), chunk, P(ws.view), nbytes, stream)
    _lib.check(rc, "pafc_wkv6_backward_state")
    torch.cuda.synchronize()
    for g in outs:
        assert bool(torch.isfinite(g.view).all())
    assert all(g.guards_intact() for g in outs + [ws]) and all(g.unchanged() for g in ins)
