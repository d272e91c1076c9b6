"""The Mamba-2 inference kernels against float64 at their edge shapes: the SSD scan (csrc/mamba2_scan.hip: fp32 and bf16 + skip
outputs, both directions, forced chunk lengths, carried state), the glue kernels (csrc/mamba2.hip: prep, finish, gate_norm), the
K = 4 depthwise convolution + SiLU as the block uses it (csrc/dwconv.hip, act 2) and the whole block on every inference path.

Acceptance rules (references and derivations in tests/ssd_ref.py):
  scan, fp32 output    ssd_ref.scan_accept: |got - ref| <= 2^-13 * yabs elementwise, yabs the scan of the operands' magnitudes
  scan, bf16 output    ssd_ref.scan_accept_bf16: between the bf16 roundings of (y + D x) -+ 2^-13 (yabs + |D x|)
  fp32 glue kernels    rtol 1e-4, atol 1e-5 (test_mamba_fused_glue_matches_op_by_op's fp32 figures), here against float64
  bf16 glue kernels    the kernel's error against float64 within 1.1 x (mean) and 2 x (max: one tie flipped at an intermediate
                       bf16 rounding is worth one further ulp) of the error of the same framework ops run on the CPU in bf16
  whole block          tests/test_mamba_stream_gpu.py's _accept: within 1.1 x (mean) + 1e-3 and 1.5 x (max) + 1e-2 of the
                       op-by-op path's error against the same float64 chain
Every measured ratio goes to the parity log."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import parity_log, ssd_ref, synth

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]

# (B, L, H, chunk_len)
SCAN_CASES = [
    (1, 1, 1, 0),                                     # one step
    (2, 15, 2, 0), (2, 16, 2, 0), (2, 17, 2, 0),      # either side of one 16-step block
    (1, 33, 1, 16),                                   # three chunks, the last holding one step
    (2, 83, 3, 32),                                   # three chunks and a partial last block
    (1, 64, 1, 16),                                   # four one-block chunks
    (2, 45, 3, 24),                                   # a chunk length the launcher rounds up to 32
    (1, 40, 16, 16),                                  # H = 16 (d_inner 1024), multi-chunk
    (3, 37, 2, 10 ** 6),                              # a forced single chunk, B = 3
]
DECAY_CASES = [(2, 83, 3, 32), (2, 17, 2, 0)]         # also run with the "slow" and "fast" recipes, and from a carried state
SCAN_MATRIX = [(*c, "mid") for c in SCAN_CASES] + [(*c, r) for c in DECAY_CASES for r in ("slow", "fast")]
CHUNKS = {(1, 33, 1, 16): 3, (2, 83, 3, 32): 3, (1, 64, 1, 16): 4, (2, 45, 3, 24): 2, (1, 40, 16, 16): 3}   # others: one chunk


@functools.lru_cache(maxsize=None)
def _scan_case(B, L, H, recipe, reverse, ldx=None, state=False):
    """Inputs and float64 references of one scan case, computed once: dict(xbc, dt, la, x, D, y, yabs[, h0, hT, habs])."""
    seed = 2000 + 17 * L + H + (7 if state else 0)
    xbc, dt, la, _ = ssd_ref.make_inputs(B, L, H, seed=seed, ldx=ldx, recipe=recipe)
    g = torch.Generator().manual_seed(seed + 1)
    D = torch.randn(H, generator=g)
    h0 = torch.randn(B, H, 128, 64, generator=g) if state else None
    x, Bm, Cm = ssd_ref.split_xbc(xbc, H)
    ops = (x, Bm, Cm, dt.double(), la.double(), reverse, None if h0 is None else h0.double(), True)
    y, hT = ssd_ref.scan_seq(*ops)
    yabs, habs = ssd_ref.abs_scan(*ops)
    return dict(xbc=xbc, dt=dt, la=la, x=x, D=D, y=y, yabs=yabs, h0=h0, hT=hT, habs=habs)


def _check_y(name, got, c, form, recipe):
    B, L, H, _ = c["x"].shape
    assert got.shape == (B, L, H * 64)
    got = got.cpu().view(B, L, H, 64)
    if form == "f32":
        assert got.dtype == F32
        ssd_ref.scan_accept(got, c["y"], c["yabs"], name=name, recipe=recipe)
    else:
        assert got.dtype == BF16
        skip = c["D"].double().view(1, 1, H, 1) * c["x"]
        ssd_ref.scan_accept_bf16(got, c["y"] + skip, ssd_ref.SCAN_REL * (c["yabs"] + skip.abs()), name=name)


def _run_scan(hip, B, L, H, chunk_len, recipe, reverse, form, ldx=None):
    from paper_accurate_fast_cheap_amd import hip_ops
    c = _scan_case(B, L, H, recipe, bool(reverse), ldx)
    nc = CHUNKS.get((B, L, H, chunk_len), 1)
    # the path the case is here for is the path that runs: the stateless multi-chunk schedule needs a workspace, one chunk none
    assert (hip.pafc_mamba2_scan_workspace_bytes(B, L, H, chunk_len) > 0) == (nc > 1)
    got = hip_ops.mamba2_scan(c["xbc"].cuda(), c["dt"].cuda(), c["la"].cuda(), H, bool(reverse),
                              D=c["D"].cuda() if form == "bf16" else None, chunk_len=chunk_len)
    _check_y(f"mamba2_scan[{B}-{L}-{H}-{chunk_len}-{recipe}-rev{reverse}-{form}{'-padded' if ldx else ''}]", got, c, form, recipe)


@pytest.mark.parametrize("form", ["f32", "bf16"])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("B,L,H,chunk_len,recipe", SCAN_MATRIX)
def test_scan_vs_float64(hip, B, L, H, chunk_len, recipe, reverse, form):
    _run_scan(hip, B, L, H, chunk_len, recipe, reverse, form)


@pytest.mark.parametrize("form", ["f32", "bf16"])
@pytest.mark.parametrize("reverse", [0, 1])
def test_scan_padded_rows(hip, reverse, form):
    """ldx = H * 64 + 256 + 64: rows wider than [x | B | C]."""
    _run_scan(hip, 2, 45, 3, 24, "mid", reverse, form, ldx=3 * 64 + 256 + 64)


def test_scan_default_chunk_len_is_the_librarys(hip):
    """chunk_len defaults to 0 = the library's own choice: the same bits as naming that chunk length."""
    from paper_accurate_fast_cheap_amd import hip_ops
    B, L, H = 2, 83, 3
    c = _scan_case(B, L, H, "mid", False)
    args = (c["xbc"].cuda(), c["dt"].cuda(), c["la"].cuda(), H)
    own = hip.pafc_mamba2_scan_chunk_len(B, L, H)
    assert torch.equal(hip_ops.mamba2_scan(*args), hip_ops.mamba2_scan(*args, chunk_len=own))
    assert torch.equal(hip_ops.mamba2_scan(*args), hip_ops.mamba2_scan(*args, chunk_len=0))


@pytest.mark.parametrize("form", ["f32", "bf16"])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("B,L,H,chunk_len", DECAY_CASES)
def test_scan_state_vs_float64(hip, B, L, H, chunk_len, reverse, form):
    """pafc_mamba2_scan_state from a random nonzero state: y (yabs includes the |h0| term) and the final state (on habs)."""
    from paper_accurate_fast_cheap_amd import hip_ops
    c = _scan_case(B, L, H, "mid", bool(reverse), None, True)
    s_in = c["h0"].cuda()
    y, s_out = hip_ops.mamba2_scan_state(c["xbc"].cuda(), c["dt"].cuda(), c["la"].cuda(), H, s_in, None, bool(reverse),
                                         D=c["D"].cuda() if form == "bf16" else None, chunk_len=chunk_len)
    name = f"mamba2_scan_state[{B}-{L}-{H}-{chunk_len}-rev{reverse}-{form}]"
    assert torch.equal(s_in.cpu(), c["h0"]) and s_out.data_ptr() != s_in.data_ptr()
    _check_y(name, y, c, form, "mid")
    ssd_ref.scan_accept(s_out.cpu(), c["hT"], c["habs"], name=name + " state", recipe="mid", head_dim=1)


@pytest.mark.parametrize("B,L,H,chunk_len", DECAY_CASES)
def test_scan_state_updated_where_it_lies(hip, B, L, H, chunk_len):
    """s_out is s_in: one and several chunks."""
    from paper_accurate_fast_cheap_amd import hip_ops
    c = _scan_case(B, L, H, "mid", False, None, True)
    s = c["h0"].cuda()
    y, s_out = hip_ops.mamba2_scan_state(c["xbc"].cuda(), c["dt"].cuda(), c["la"].cuda(), H, s, s, chunk_len=chunk_len)
    assert s_out is s
    name = f"mamba2_scan_state[{B}-{L}-{H}-{chunk_len}-in place]"
    _check_y(name, y, c, "f32", "mid")
    ssd_ref.scan_accept(s.cpu(), c["hT"], c["habs"], name=name + " state", recipe="mid", head_dim=1)


def test_scan_refuses_malformed_operands(hip):
    """mamba2_scan reads xbc with its row stride and dt / log_a as packed (B, L, H): anything else is refused, not misread."""
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd._lib import PafcError
    B, L, H = 2, 17, 2
    ldx = H * 64 + 256
    wide = torch.zeros(B, L, ldx + 64, dtype=BF16, device="cuda")
    xbc = torch.zeros(B, L, ldx, dtype=BF16, device="cuda")
    dt, la = torch.zeros(B, L, H, device="cuda"), torch.zeros(B, L, H, device="cuda")
    assert hip_ops.mamba2_scan(xbc, dt, la, H).shape == (B, L, H * 64)
    assert hip_ops.mamba2_scan(wide, dt, la, H).shape == (B, L, H * 64)           # a wider contiguous row is fine
    bad = [
        (wide[..., :ldx], dt, la),                                                 # a column slice: not contiguous
        (xbc[0], dt[0], la[0]),                                                    # not 3-D
        (xbc, torch.zeros(B, L, H + 1, device="cuda"), la),                        # dt of another shape
        (xbc, dt, torch.zeros(B, L + 1, H, device="cuda")),                        # log_a of another shape
        (xbc, torch.zeros(B, L, 2 * H, device="cuda")[..., ::2], la),              # dt not contiguous
        (xbc, dt, torch.zeros(B, L, 2 * H, device="cuda")[..., ::2]),              # log_a not contiguous
        (xbc[..., :ldx - 4].contiguous(), dt, la),                                 # rows shorter than [x | B | C]
    ]
    for args in bad:
        for D in (None, torch.ones(H, device="cuda")):
            with pytest.raises(PafcError):
                hip_ops.mamba2_scan(*args, H, D=D)


def test_prep_and_finish_refuse_another_row_width(hip):
    """Both kernels hard-code the row width d_inner + 256 of xbc."""
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd._lib import PafcError
    B, L, di, H = 1, 3, 128, 2
    dev = "cuda"
    zxbcdt = torch.zeros(B, L, 2 * di + 256 + H, device=dev)
    z, dt_raw = zxbcdt[..., :di], zxbcdt[..., 2 * di + 256:]
    dt_bias, A_log, D = (torch.zeros(H, device=dev) for _ in range(3))
    w = torch.ones(di, device=dev)
    y0 = torch.zeros(B, L, di, device=dev)
    good = torch.zeros(B, L, di + 256, device=dev)
    assert len(hip_ops.mamba2_prep(good, dt_raw, dt_bias, A_log, di)) == 6
    assert hip_ops.mamba2_finish(y0, None, good, dt_raw, z, dt_bias, D, w, 1e-5, di).shape == (B, L, di)
    wider = torch.zeros(B, L, di + 256 + 64, device=dev)
    for xbc in (wider, wider[..., :di + 256], zxbcdt[..., di:2 * di + 256], good[0]):
        with pytest.raises(PafcError):
            hip_ops.mamba2_prep(xbc, dt_raw, dt_bias, A_log, di)
        with pytest.raises(PafcError):
            hip_ops.mamba2_finish(y0, None, xbc, dt_raw, z, dt_bias, D, w, 1e-5, di)


# ---- glue kernels ------------------------------------------------------------------------------------------------------------

def _accept_f32(name, got, ref):
    """rtol 1e-4, atol 1e-5 against float64 (the fp32 figures of test_mamba_fused_glue_matches_op_by_op)."""
    assert got.dtype == F32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), name
    worst = float(((got - ref).abs() / (1e-5 + 1e-4 * ref.abs())).max())
    parity_log.record(name, err_over_bound=worst)
    print(f"{name}: max |err| / (1e-5 + 1e-4 |ref|) = {worst:.3g}")
    assert worst <= 1.0, (name, worst)


def _accept_bf16(name, got, comp, ref):
    """Kernel against float64 within 1.1 x (mean) and 2 x (max) of the CPU framework ops in bf16 against the same float64."""
    assert got.dtype == BF16 and comp.dtype == BF16 and got.shape == comp.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), name
    e_k, e_c = (got - ref).abs(), (comp.double() - ref).abs()
    vals = dict(kernel_max=float(e_k.max()), kernel_mean=float(e_k.mean()), cpu_bf16_max=float(e_c.max()), cpu_bf16_mean=float(e_c.mean()))
    parity_log.record(name, **vals)
    print(name, vals)
    assert vals["kernel_mean"] <= 1.1 * vals["cpu_bf16_mean"], (name, vals)
    assert vals["kernel_max"] <= 2 * vals["cpu_bf16_max"], (name, vals)


def _gate_norm_case(hip, name, rows, d, dtype, zmax=None):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import RMSNormGated
    g = torch.Generator().manual_seed(300 + 7 * rows + d)
    y = torch.randn(rows, d, generator=g).to(dtype)
    zw = torch.randn(rows, d + 24, generator=g)
    if zmax:
        zw = (torch.rand(rows, d + 24, generator=g) * 2 - 1) * zmax
    zw = zw.to(dtype)
    w = (torch.rand(d, generator=g) + 0.5).to(dtype)
    got = hip_ops.mamba2_gate_norm(y.cuda(), zw.cuda()[:, 8:8 + d], w.cuda(), 1e-5)
    ref = ssd_ref.gate_norm_ref(y, zw[:, 8:8 + d], w, 1e-5, dtype)
    if dtype == F32:
        return _accept_f32(name, got, ref)
    norm = RMSNormGated(d).to(BF16)
    with torch.no_grad():
        norm.weight.copy_(w)
        comp = norm(y, zw[:, 8:8 + d])
    _accept_bf16(name, got, comp, ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [8, 128, 520, 1024])
@pytest.mark.parametrize("rows", [1, 3, 5, 130])
def test_gate_norm_vs_float64(hip, rows, d, dtype):
    """Rows that do not fill the last four-row block, channels that end inside either 512-channel pass, z a column slice."""
    _gate_norm_case(hip, f"mamba2_gate_norm[{rows}x{d}-{dtype}]", rows, d, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_norm_saturated_silu(hip, dtype):
    """|z| up to 30: silu(z) = z on one side and about z e^z (1e-12) on the other."""
    _gate_norm_case(hip, f"mamba2_gate_norm[saturated-{dtype}]", 5, 520, dtype, zmax=30.0)


def _block_inputs(Bsz, L, di, dtype, seed):
    """One zxbcdt row tensor (z and dt_raw are its column slices, as the module passes them), the conv output xbc, per-head
    parameters.  dt_raw + dt_bias above 20 (softplus' linear branch) and below -30 at steps that are also some step's next."""
    H = di // 64
    g = torch.Generator().manual_seed(seed)
    zxbcdt = torch.randn(Bsz, L, 2 * di + 256 + H, generator=g)
    zxbcdt[..., 2 * di + 256:] *= 2
    zxbcdt[0, min(1, L - 1), 2 * di + 256] = 25.0
    if H > 1:
        zxbcdt[0, min(2, L - 1), 2 * di + 256 + H - 1] = -40.0
    zxbcdt = zxbcdt.to(dtype)
    xbc = (torch.randn(Bsz, L, di + 256, generator=g) * 0.5).to(dtype)
    dt_bias = torch.randn(H, generator=g) * 0.5
    A_log = torch.log(torch.rand(H, generator=g) * 15 + 1)
    D = torch.randn(H, generator=g)
    w = (torch.rand(di, generator=g) + 0.5).to(dtype)
    return zxbcdt, xbc, dt_bias, A_log, D, w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_y1", [False, True])
@pytest.mark.parametrize("diag", [0, 1])
@pytest.mark.parametrize("di", [64, 192, 1024])
@pytest.mark.parametrize("Bsz,L", [(1, 1), (2, 5)])
def test_finish_vs_float64(hip, Bsz, L, di, diag, with_y1, dtype):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import RMSNormGated
    H = di // 64
    zxbcdt, xbc, dt_bias, _, D, w = _block_inputs(Bsz, L, di, dtype, 400 + L + di)
    g = torch.Generator().manual_seed(401)
    y0 = torch.randn(Bsz, L, di, generator=g)
    y1 = torch.randn(Bsz, L, di, generator=g) if with_y1 else None
    sl = lambda t: (t[..., :di], t[..., 2 * di + 256:])
    z, dt_raw = sl(zxbcdt)
    zg, dtg = sl(zxbcdt.cuda())
    got = hip_ops.mamba2_finish(y0.cuda(), None if y1 is None else y1.cuda(), xbc.cuda(), dtg, zg, dt_bias.cuda(), D.cuda(),
                                w.cuda(), 1e-5, di, diag=bool(diag))
    ref = ssd_ref.finish_ref(y0, y1, xbc, dt_raw, z, dt_bias, D, w, 1e-5, di, bool(diag), dtype)
    name = f"mamba2_finish[{Bsz}x{L}-{di}-diag{diag}-y1{int(with_y1)}-{dtype}]"
    assert (dt_raw[0, min(1, L - 1), 0].float() + dt_bias[0]) > 20
    if dtype == F32:
        return _accept_f32(name, got, ref)
    # the module's lines in the framework's own arithmetic on the CPU
    xf = xbc[..., :di].float().view(Bsz, L, H, 64)
    dt = F.softplus(dt_raw.float() + dt_bias)
    y = y0 + (0 if y1 is None else y1)
    if diag:
        bc = (xbc[..., di:di + 128].float() * xbc[..., di + 128:].float()).sum(-1, keepdim=True).unsqueeze(-1)
        y = y + (bc * (xf * dt.unsqueeze(-1))).reshape(Bsz, L, di)
    y = y + (xf * D.view(1, 1, H, 1)).reshape(Bsz, L, di)
    norm = RMSNormGated(di).to(BF16)
    with torch.no_grad():
        norm.weight.copy_(w)
        comp = norm(y.to(BF16), z)
    _accept_bf16(name, got, comp, ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("di", [128, 1024])
@pytest.mark.parametrize("Bsz,L", [(1, 1), (2, 2), (2, 9)])
def test_prep_vs_float64(hip, Bsz, L, di, dtype):
    """All six planes (fp32 from exact inputs whatever the input dtype: the fp32 rule); the last step of every batch entry has
    a_next = 1 and w = log(1e-30), i.e. the read of the next row's dt never crosses into the following batch entry."""
    from paper_accurate_fast_cheap_amd import hip_ops
    H = di // 64
    zxbcdt, xbc, dt_bias, A_log, _, _ = _block_inputs(Bsz, L, di, dtype, 500 + L + di)
    dt_raw = zxbcdt[..., 2 * di + 256:]
    s = dt_raw.float() + dt_bias
    assert float(s.max()) > 20 and float(s.min()) < -30
    got = hip_ops.mamba2_prep(xbc.cuda(), zxbcdt.cuda()[..., 2 * di + 256:], dt_bias.cuda(), A_log.cuda(), di)
    ref = ssd_ref.prep_ref(xbc, dt_raw, dt_bias, A_log, di)
    for plane, a, b in zip(("r0", "r1", "k0", "k1", "v", "w"), got, ref):
        _accept_f32(f"mamba2_prep[{Bsz}x{L}-{di}-{dtype}] {plane}", a, b)
    k0, k1, wl = (got[i].cpu()[:, -1].view(Bsz, H, 64) for i in (2, 3, 5))
    Bm = xbc[:, -1, di:di + 128].float()
    assert torch.equal(k0, Bm[:, None, :64].expand(Bsz, H, 64)) and torch.equal(k1, Bm[:, None, 64:].expand(Bsz, H, 64))
    torch.testing.assert_close(wl, torch.full_like(wl, math.log(1e-30)), rtol=1e-6, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["causal", "reverse", "prefix"])
@pytest.mark.parametrize("C", [384, 1280])
def test_conv_silu_k4_vs_float64(hip, C, mode, dtype):
    """causal_conv_silu_cl (both directions) and causal_conv_silu_cl_prefix as the block calls them: K = 4, SiLU epilogue, the
    input a column slice of in_proj's wider row, sequences shorter than the kernel, two distinct batch entries."""
    from paper_accurate_fast_cheap_amd import hip_ops
    K, Bsz, di = 4, 2, C - 256
    g = torch.Generator().manual_seed(600 + C)
    w = (torch.randn(C, 1, K, generator=g) * 0.4).to(dtype)
    b = (torch.randn(C, generator=g) * 0.1).to(dtype)
    for L in (1, 2, 3, 4, 5, 37):
        wide = torch.randn(Bsz, L, 2 * di + 256 + di // 64, generator=g).to(dtype)
        ctx = torch.randn(Bsz, K - 1, C, generator=g).to(dtype)
        x = wide[..., di:2 * di + 256]
        xg = wide.cuda()[..., di:2 * di + 256]
        assert not xg.is_contiguous()
        if mode == "prefix":
            got = hip_ops.causal_conv_silu_cl_prefix(torch.cat([ctx.cuda(), xg], 1), w.cuda(), b.cuda())
            ref = ssd_ref.conv_silu_ref(x, w, b, dtype, prefix=ctx)
        else:
            got = hip_ops.causal_conv_silu_cl(xg, w.cuda(), b.cuda(), reverse=mode == "reverse")
            ref = ssd_ref.conv_silu_ref(x, w, b, dtype, reverse=mode == "reverse")
        name = f"causal_conv_silu_cl[{mode}-C{C}-L{L}-{dtype}]"
        assert got.is_contiguous()
        if dtype == F32:
            _accept_f32(name, got, ref)
            continue
        xp = torch.cat([ctx if mode == "prefix" else torch.zeros_like(ctx), torch.flip(x, [1]) if mode == "reverse" else x], 1)
        comp = F.silu(F.conv1d(xp.transpose(1, 2), w, b, groups=C).transpose(1, 2))
        _accept_bf16(name, got, torch.flip(comp, [1]) if mode == "reverse" else comp, ref)


# ---- whole block -------------------------------------------------------------------------------------------------------------

def _accept_block(tag, got, plain, ref):
    """The form of tests/test_mamba_stream_gpu.py's _accept: the path's error against the float64 chain within 1.1 x (mean) /
    1.5 x (max) of the op-by-op path's error against the same chain, plus 1e-3 / 1e-2.  Both are measured here and logged."""
    assert got.shape == ref.shape == plain.shape, (got.shape, plain.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), tag
    e_k, e_p = (got.double().cpu() - ref).abs(), (plain.double().cpu() - ref).abs()
    vals = dict(path_max=float(e_k.max()), path_mean=float(e_k.mean()), op_by_op_max=float(e_p.max()), op_by_op_mean=float(e_p.mean()),
                ref_abs_max=float(ref.abs().max()))
    parity_log.record(f"mamba2 block/{tag}", **vals)
    print(f"[mamba2 block] {tag}: {vals}")
    assert vals["path_mean"] <= 1.1 * vals["op_by_op_mean"] + 1e-3, (tag, vals)
    assert vals["path_max"] <= 1.5 * vals["op_by_op_max"] + 1e-2, (tag, vals)


def _block(cls, d_model, dtype, seed):
    torch.manual_seed(seed)
    m = cls(d_model, headdim=64).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.weight") or n.endswith("D"):
                p.uniform_(0.5, 1.5)
    m = m.to(dtype)
    params = {k: v.detach().double() for k, v in m.named_parameters()}          # as rounded to the module's dtype
    return m.cuda(), params


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("L", [1, 45])
@pytest.mark.parametrize("d_model", [128, 512])
def test_block_vs_float64_chain(hip, d_model, L, reverse, dtype):
    """Every inference path of the block against ssd_ref.mamba2_chain in float64: bf16 on the SSD kernel with the bf16 + skip
    output (scan, gate_norm) and with the fp32 output (scan, finish), bf16 on the operand planes and the WKV-6 scan (prep,
    finish), fp32 fused."""
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2
    m, params = _block(Mamba2, d_model, dtype, 700 + d_model)
    u = synth.randn((2, L, d_model), 71).to(dtype)
    ref = ssd_ref.mamba2_chain(params, u.double(), reverse)
    paths = ([("ssd bf16 out", True, True), ("ssd f32 out", True, False), ("wkv planes", False, True)] if dtype == BF16
             else [("fused", True, True)])
    ug = u.cuda()
    with torch.no_grad():
        m.fused_inference = False
        plain = m(ug, reverse=reverse)
        m.fused_inference = True
        for tag, ssd, bf16_out in paths:
            m.ssd_kernel, m.scan_bf16_out = ssd, bf16_out
            assert m.fused_eligible(ug)
            got = m(ug, reverse=reverse)
            assert got.dtype == dtype
            _accept_block(f"{tag} d{d_model} L{L} rev{int(reverse)} {dtype}", got, plain, ref)


def test_bidirectional_block_vs_float64_chains(hip):
    """Mamba2Bidirectional in bf16: the float64 average of the left-to-right and the right-to-left chain."""
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2Bidirectional
    m, params = _block(Mamba2Bidirectional, 128, BF16, 800)
    u = synth.randn((2, 45, 128), 72).to(BF16)
    sub = lambda pre: {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}
    ref = (ssd_ref.mamba2_chain(sub("mamba_forward."), u.double()) + ssd_ref.mamba2_chain(sub("mamba_backward."), u.double(), True)) / 2
    with torch.no_grad():
        m.mamba_forward.fused_inference = m.mamba_backward.fused_inference = False
        plain = m(u.cuda())
        m.mamba_forward.fused_inference = m.mamba_backward.fused_inference = True
        got = m(u.cuda())
    _accept_block("bidirectional d128 L45 bf16", got, plain, ref)
