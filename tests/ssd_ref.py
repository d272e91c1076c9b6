"""Float64 references of the Mamba-2 selective scan (SSD) and of its backward; no GPU code.

Per head (head dim P = 64, state dim N = 128, B_t / C_t shared by the heads, a_t = exp(la_t)):
    h_t = a_t h_{t-1} + dt_t B_t x_t^T ,   y_t = C_t . h_t
`scan_seq` is that recurrence, step by step, differentiable by autograd.  `closed_forms` is the backward written out
(the forms the kernel of csrc/mamba2_scan_bwd.hip evaluates):
    G_t = C_t gy_t^T + a_{t+1} G_{t+1}     gxu_t = B_t . G_t     g_x_t = dt_t gxu_t     g_dt_t = gxu_t . x_t
    g_B_t = sum_heads dt_t G_t x_t         g_C_t = sum_heads h_t gy_t
    g_la_t = a_t <G_t, h_{t-1}> = sum_{s >= t} (gy_s . y_s - dt_s g_dt_s)
`mamba2_chain` is the whole Mamba-2 block on top of scan_seq, for gradients of the module's parameters.
`abs_scan` is the recurrence on the operands' magnitudes: the sum of the magnitudes of the terms of each output, which is what a
kernel's rounding errors scale with; `scan_accept` / `scan_accept_bf16` are the forward kernels' acceptance rule built on it.
`gate_norm_ref`, `finish_ref`, `prep_ref`, `conv_silu_ref` restate the lines of transformer/mamba2.py that the glue kernels of
csrc/mamba2.hip and the K = 4 depthwise convolution fuse, in float64 with the module's bf16 rounding points made explicit.
reverse = True: step s of the recurrence is time index L - 1 - s; inputs and outputs stay at their own time index."""
import functools

import torch
import torch.nn.functional as F

N, P = 128, 64


RECIPES = {"mid": ((0.01, 0.21), (0.5, 8.5)), "slow": ((0.001, 0.01), (1.0, 2.0)), "fast": ((1.0, 5.0), (8.0, 16.0))}


def make_inputs(B, L, H, seed, ldx=None, recipe="mid"):
    """xbc randn * 0.5 in bf16, dt uniform in the recipe's first range, la = -dt * A with A per head uniform in its second, gy
    randn rounded to bf16 and stored as fp32.  Recipes ((dt range), (A range)):
        "mid"   the recipe of test_mamba_ssd_scan_raw_vs_sequential: dt in [0.01, 0.21], A in [0.5, 8.5];
        "slow"  dt in [0.001, 0.01], A in [1, 2]: the module's initialisation range, the state integrates over the whole sequence;
        "fast"  dt in [1, 5], A in [8, 16]: log a per step between -80 and -8, so e^{cum_15} and most of a 16 x 16 decay mask
                underflow to zero in fp32."""
    (d0, d1), (a0, a1) = RECIPES[recipe]
    g = torch.Generator().manual_seed(seed)
    ldx = ldx or H * P + 2 * N
    xbc = (torch.randn(B, L, ldx, generator=g) * 0.5).to(torch.bfloat16)
    dt = torch.rand(B, L, H, generator=g) * (d1 - d0) + d0
    la = -dt * (torch.rand(H, generator=g) * (a1 - a0) + a0)
    gy = torch.randn(B, L, H * P, generator=g).to(torch.bfloat16).float()
    return xbc, dt, la, gy


def split_xbc(xbc, H, dtype=torch.float64):
    """xbc (B, L, >= H * 64 + 256) -> x (B, L, H, 64), B (B, L, 128), C (B, L, 128) in `dtype`."""
    Bsz, L, _ = xbc.shape
    d = H * P
    return xbc[..., :d].to(dtype).reshape(Bsz, L, H, P), xbc[..., d:d + N].to(dtype), xbc[..., d + N:d + 2 * N].to(dtype)


def scan_seq(x, Bm, Cm, dt, la, reverse=False, h0=None, return_state=False):
    """x (B, L, H, 64), Bm / Cm (B, L, 128), dt / la (B, L, H) -> y (B, L, H, 64), in the inputs' dtype, differentiable.
    h0 (B, H, 128, 64): the state before the recurrence's first step (None = zero); return_state: -> (y, state after its last)."""
    if reverse:
        out = scan_seq(*(torch.flip(t, [1]) for t in (x, Bm, Cm, dt, la)), h0=h0, return_state=return_state)
        return (torch.flip(out[0], [1]), out[1]) if return_state else torch.flip(out, [1])
    Bsz, L, H, _ = x.shape
    h = x.new_zeros(Bsz, H, N, P) if h0 is None else h0.to(x.dtype)
    ys = []
    for t in range(L):
        h = h * torch.exp(la[:, t]).view(Bsz, H, 1, 1) + (dt[:, t].view(Bsz, H, 1, 1) * Bm[:, t].view(Bsz, 1, N, 1)
                                                         * x[:, t].view(Bsz, H, 1, P))
        ys.append(torch.einsum("bn,bhnp->bhp", Cm[:, t], h))
    y = torch.stack(ys, 1)
    return (y, h) if return_state else y


def abs_scan(x, Bm, Cm, dt, la, reverse=False, h0=None, return_state=False):
    """scan_seq on |x|, |B|, |C| (and |h0|) with the same dt and la: yabs_t = sum over the terms of y_t of their magnitudes
    (habs likewise for the final state).  yabs >= |y| elementwise; an error bound relative to yabs is a bound per term."""
    return scan_seq(x.abs(), Bm.abs(), Cm.abs(), dt, la, reverse, None if h0 is None else h0.abs(), return_state)


SCAN_REL = 2.0 ** -13


def scan_accept(got, ref, yabs, name="scan", recipe="mid", head_dim=2):
    """The acceptance rule of the forward SSD scan kernels against float64, elementwise:
        |got - ref| <= 2^-13 * yabs + 1e-30,        yabs = abs_scan(...), same shape as ref
    The constant is derived from the kernel's arithmetic (csrc/mamba2_scan.hip), per term dt_s e^{cum_t - cum_s} (C_t . B_s) x_s
    of y_t (x, B, C are bf16 and enter the matrix cores exactly, C . B is an exact bf16 product summed in fp32):
      * a term passes through at most two hi + lo bf16 operand splits (the decay-scaled B_s into the state, the state into
        C_t . H; or the masked 16 x 16 matrix alone): each keeps 16 bits, error <= 2^-16 of the term;
      * the fp32 roundings of the state update and of the sums, and __expf (relative error about |x| 2^-24 for |x| <= 128),
        add at most 2^-17;
    together below 2^-14 per term; the bound allows twice that.  (1e-30: terms whose decay underflows in fp32.)
    recipe "mid" also keeps the project's existing bound (test_mamba_ssd_scan_raw_vs_sequential's 2e-4 of max |y|), per (batch,
    head) instead of globally: max |got - ref| <= 2e-4 * max |ref| over each head (axis `head_dim`; axis 0 is the batch).
    Both observed ratios go to the parity log."""
    from tests import parity_log
    got, ref, yabs = got.double(), ref.double(), yabs.double()
    assert got.shape == ref.shape == yabs.shape, (got.shape, ref.shape, yabs.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    worst = float((err / (yabs + 1e-30 / SCAN_REL)).max())
    rest = [d for d in range(ref.dim()) if d not in (0, head_dim)]
    per_head = float((err.amax(rest) / ref.abs().amax(rest).clamp_min(1e-300)).max())
    parity_log.record(name, err_over_yabs=worst, err_over_head_max=per_head)
    print(f"{name}: max |err| / yabs {worst:.3g} (bound {SCAN_REL:.3g}), per-head max |err| / max |ref| {per_head:.3g}")
    assert bool((err <= SCAN_REL * yabs + 1e-30).all()), (name, worst)
    if recipe == "mid":
        assert per_head <= 2e-4, (name, per_head)


def scan_accept_bf16(got, ref, tol, name="scan bf16"):
    """A bf16 output of a value known to within `tol` of `ref` (both float64, elementwise): every element must lie between the bf16
    roundings of ref - tol and ref + tol (the interval form of test_mamba_train_gpu.py's g_x).  For pafc_mamba2_scan_skip_bf16:
    ref = y + D x, tol = 2^-13 * (yabs + |D x|)."""
    from tests import parity_log
    got, ref, tol = got.double(), ref.double(), tol.double()
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    lo, hi = (ref - tol).float().to(torch.bfloat16).double(), (ref + tol).float().to(torch.bfloat16).double()
    out = torch.maximum(lo - got, got - hi).clamp_min(0)             # distance outside the interval
    worst = float((out / ref.abs().clamp_min(1e-30)).max())
    parity_log.record(name, outside_interval_over_ref=worst, elements_outside=int((out > 0).sum()))
    print(f"{name}: {int((out > 0).sum())} of {out.numel()} elements outside the rounded interval, worst by {worst:.3g} |ref|")
    assert bool((out == 0).all()), (name, worst)


def scan_xbc(xbc, dt, la, H, reverse=False, dtype=torch.float64):
    """The scan on the kernel's operands, y (B, L, H * 64) in `dtype`: a differentiable stand-in for hip_ops.mamba2_scan_train
    (gradients flow back into xbc, dt and la in their own dtypes)."""
    x, Bm, Cm = split_xbc(xbc, H, dtype)
    y = scan_seq(x, Bm, Cm, dt.to(dtype), la.to(dtype), reverse)
    return y.reshape(y.shape[0], y.shape[1], H * P)


def autograd_grads(xbc, dt, la, gy, H, reverse=False):
    """float64 autograd of scan_seq: {y, g_x (B, L, H, 64), g_B, g_C (B, L, 128), g_dt, g_la (B, L, H)}."""
    x, Bm, Cm = (t.requires_grad_() for t in split_xbc(xbc, H))
    dt64, la64 = dt.double().requires_grad_(), la.double().requires_grad_()
    y = scan_seq(x, Bm, Cm, dt64, la64, reverse)
    g = torch.autograd.grad(y, (x, Bm, Cm, dt64, la64), gy.double().view_as(y))
    return dict(y=y.detach(), g_x=g[0], g_B=g[1], g_C=g[2], g_dt=g[3], g_la=g[4])


def closed_forms(xbc, dt, la, gy, H, reverse=False):
    """The backward written out in float64: the keys of autograd_grads plus g_la_suffix (the suffix-sum form of g_la)."""
    if reverse:
        out = closed_forms(*(torch.flip(t, [1]) for t in (xbc, dt, la, gy)), H)
        return {k: torch.flip(v, [1]) for k, v in out.items()}
    x, Bm, Cm = split_xbc(xbc, H)
    dt, la = dt.double(), la.double()
    Bsz, L = x.shape[:2]
    gy = gy.double().view(Bsz, L, H, P)
    a = torch.exp(la)
    hs = [x.new_zeros(Bsz, H, N, P)]
    for t in range(L):
        hs.append(hs[-1] * a[:, t].view(Bsz, H, 1, 1)
                  + dt[:, t].view(Bsz, H, 1, 1) * Bm[:, t].view(Bsz, 1, N, 1) * x[:, t].view(Bsz, H, 1, P))
    y = torch.stack([torch.einsum("bn,bhnp->bhp", Cm[:, t], hs[t + 1]) for t in range(L)], 1)
    g_x, g_B, g_C = torch.zeros_like(x), torch.zeros_like(Bm), torch.zeros_like(Cm)
    g_dt, g_la = torch.zeros_like(dt), torch.zeros_like(la)
    G = x.new_zeros(Bsz, H, N, P)
    for t in range(L - 1, -1, -1):
        if t + 1 < L:
            G = G * a[:, t + 1].view(Bsz, H, 1, 1)
        G = G + Cm[:, t].view(Bsz, 1, N, 1) * gy[:, t].view(Bsz, H, 1, P)
        gxu = torch.einsum("bn,bhnp->bhp", Bm[:, t], G)
        g_x[:, t] = dt[:, t].unsqueeze(-1) * gxu
        g_dt[:, t] = (gxu * x[:, t]).sum(-1)
        g_B[:, t] = torch.einsum("bh,bhnp,bhp->bn", dt[:, t], G, x[:, t])
        g_C[:, t] = torch.einsum("bhnp,bhp->bn", hs[t + 1], gy[:, t])
        g_la[:, t] = a[:, t] * (G * hs[t]).sum((-1, -2))
    d = (gy * y).sum(-1) - dt * g_dt
    g_la_suffix = torch.flip(torch.cumsum(torch.flip(d, [1]), 1), [1])
    return dict(y=y, g_x=g_x, g_B=g_B, g_C=g_C, g_dt=g_dt, g_la=g_la, g_la_suffix=g_la_suffix)


def cancellation_scale(ref, dt, gy):
    """S = max over (batch, head) of sum_s (|gy_s . y_s| + |dt_s g_dt_s|): the size of the terms whose suffix sums are g_la."""
    y = ref["y"]
    gyy = (gy.double().view_as(y) * y).sum(-1).abs()
    return float((gyy + (dt.double() * ref["g_dt"]).abs()).sum(1).max())


@functools.lru_cache(maxsize=None)
def kernel_case(B, L, H, reverse, ldx=None):
    """Inputs and float64 reference of one kernel test case, computed once: (xbc, dt, la, gy, ref, S)."""
    xbc, dt, la, gy = make_inputs(B, L, H, seed=1000 + 17 * L + H, ldx=ldx)
    ref = autograd_grads(xbc, dt, la, gy, H, reverse)
    return xbc, dt, la, gy, ref, cancellation_scale(ref, dt, gy)


def mamba2_chain(params, u, reverse=False):
    """transformer/mamba2.py's block in the dtype of `params` (a dict with the module's parameter names), sequential scan:
        z, xBC, dt = split(in_proj(u));  xBC = silu(causal depthwise conv1d(xBC));  x, B, C = split(xBC)
        dt = softplus(dt + dt_bias);  la = -dt exp(A_log);  y = scan + D x;  out = out_proj(RMSNorm(y silu(z)) norm.weight)"""
    if reverse:
        return torch.flip(mamba2_chain(params, torch.flip(u, [1])), [1])
    H = params["A_log"].numel()
    d_inner = H * P
    Bsz, L, _ = u.shape
    zxbcdt = u @ params["in_proj.weight"].t()
    z, xBC, dt = torch.split(zxbcdt, [d_inner, d_inner + 2 * N, H], dim=-1)
    w = params["conv1d.weight"]
    K = w.shape[-1]
    xBC = F.conv1d(xBC.transpose(1, 2), w, params["conv1d.bias"], padding=K - 1, groups=w.shape[0])[..., :L].transpose(1, 2)
    xBC = F.silu(xBC)
    x, Bm, Cm = torch.split(xBC, [d_inner, N, N], dim=-1)
    dt = F.softplus(dt + params["dt_bias"])
    la = dt * -torch.exp(params["A_log"])
    x = x.reshape(Bsz, L, H, P)
    y = scan_seq(x, Bm, Cm, dt, la) + x * params["D"].view(1, 1, H, 1)
    y = y.reshape(Bsz, L, d_inner) * F.silu(z)
    y = y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + 1e-5) * params["norm.weight"]
    return y @ params["out_proj.weight"].t()


def _rnd(t, dtype):
    """A float64 tensor rounded to `dtype` where the module holds it in that dtype (float32: the reference stays exact)."""
    return t.float().to(dtype).double() if dtype == torch.bfloat16 else t


def _silu(t):
    return t * torch.sigmoid(t)


def _softplus(t):
    return torch.where(t > 20, t, torch.log1p(torch.exp(t.clamp(max=20))))          # F.softplus: beta 1, threshold 20


def gate_norm_ref(y, z, weight, eps, dtype):
    """RMSNormGated: (y * silu(z)).float() -> x rsqrt(mean x^2 + eps) * weight.  float64; for bf16 silu(z) and the product are
    rounded as the framework's ops round them.  The value BEFORE the output's own rounding."""
    g = _rnd(y.double() * _rnd(_silu(z.double()), dtype), dtype)
    return g * torch.rsqrt(g.pow(2).mean(-1, keepdim=True) + eps) * weight.double()


def finish_ref(y0, y1, xbc, dt_raw, z, dt_bias, D, weight, eps, d_inner, diag, dtype):
    """The tail of Mamba2.forward: y = y0 (+ y1) (+ (B . C) dt x, the s = t term the WKV-6 scan leaves out) + D x; y.to(dtype);
    RMSNormGated(y, z).  y0 / y1 (B, L, d_inner) fp32 scan outputs, xbc (B, L, d_inner + 256), dt_raw (B, L, H)."""
    Bsz, L, _ = xbc.shape
    H = d_inner // P
    x, Bm, Cm = split_xbc(xbc, H)
    dt = _softplus(dt_raw.double() + dt_bias.double())
    y = y0.double().view(Bsz, L, H, P) + (0 if y1 is None else y1.double().view(Bsz, L, H, P))
    if diag:
        y = y + (Bm * Cm).sum(-1).view(Bsz, L, 1, 1) * (x * dt.unsqueeze(-1))
    y = y + x * D.double().view(1, 1, H, 1)
    return gate_norm_ref(_rnd(y.reshape(Bsz, L, d_inner), dtype), z, weight, eps, dtype)


def prep_ref(xbc, dt_raw, dt_bias, A_log, d_inner):
    """The six fp32 operand planes of the two WKV-6 scans (Mamba2.forward's lines), float64, each (B, L, d_inner):
    r_half = C_half, k_half = a_{t+1} B_half (both the same for every head), v = dt x, w = log(max(-log a_{t+1}, 1e-30)); the last
    step of every batch entry has log a_{t+1} = 0."""
    Bsz, L, _ = xbc.shape
    H = d_inner // P
    x, Bm, Cm = split_xbc(xbc, H)
    dt = _softplus(dt_raw.double() + dt_bias.double())
    logdec = dt * -torch.exp(A_log.double())
    nxt = torch.cat([logdec[:, 1:], torch.zeros_like(logdec[:, :1])], dim=1)
    a_next = torch.exp(nxt)
    w = torch.log((-nxt).clamp_min(1e-30))
    per_head = lambda t: t.unsqueeze(2).expand(Bsz, L, H, 64).reshape(Bsz, L, d_inner)
    halves = lambda t: (t[..., :64], t[..., 64:])
    r0, r1 = (per_head(c) for c in halves(Cm))
    k0, k1 = ((a_next.unsqueeze(-1) * b.unsqueeze(2)).reshape(Bsz, L, d_inner) for b in halves(Bm))
    v = (x * dt.unsqueeze(-1)).reshape(Bsz, L, d_inner)
    return [r0, r1, k0, k1, v, w.unsqueeze(-1).expand(Bsz, L, H, 64).reshape(Bsz, L, d_inner)]


def conv_silu_ref(x, weight, bias, dtype, reverse=False, prefix=None):
    """silu(causal depthwise conv1d) in channels-last layout, float64: x (B, L, C), weight (C, 1, K), bias (C) -> (B, L, C); for
    bf16 the convolution's output is rounded before the SiLU, as the framework's two ops round it.  prefix (B, K - 1, C): the
    rows in front of x instead of the zero padding.  reverse: flip, convolve, flip.  The value BEFORE the output's own rounding."""
    if reverse:
        return torch.flip(conv_silu_ref(torch.flip(x, [1]), weight, bias, dtype), [1])
    K = weight.shape[-1]
    Bsz, L, C = x.shape
    ctx = x.new_zeros(Bsz, K - 1, C) if prefix is None else prefix
    xp = torch.cat([ctx, x], 1).double().transpose(1, 2)
    u = F.conv1d(xp, weight.double(), bias.double(), groups=C).transpose(1, 2)
    return _silu(_rnd(u, dtype))
