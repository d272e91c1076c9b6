"""Float64 references of the Mamba-2 selective scan (SSD) and of its backward; no GPU code.

Per head (head dim P = 64, state dim N = 128, B_t / C_t shared by the heads, a_t = exp(la_t)):
    h_t = a_t h_{t-1} + dt_t B_t x_t^T ,   y_t = C_t . h_t
`scan_seq` is that recurrence, step by step, differentiable by autograd.  `closed_forms` is the backward written out
(the forms the kernel of csrc/mamba2_scan_bwd.hip evaluates):
    G_t = C_t gy_t^T + a_{t+1} G_{t+1}     gxu_t = B_t . G_t     g_x_t = dt_t gxu_t     g_dt_t = gxu_t . x_t
    g_B_t = sum_heads dt_t G_t x_t         g_C_t = sum_heads h_t gy_t
    g_la_t = a_t <G_t, h_{t-1}> = sum_{s >= t} (gy_s . y_s - dt_s g_dt_s)
`mamba2_chain` is the whole Mamba-2 block on top of scan_seq, for gradients of the module's parameters.
reverse = True: step s of the recurrence is time index L - 1 - s; inputs and outputs stay at their own time index."""
import functools

import torch
import torch.nn.functional as F

N, P = 128, 64


def make_inputs(B, L, H, seed, ldx=None):
    """The recipe of test_mamba_ssd_scan_raw_vs_sequential plus a gradient: xbc randn * 0.5 in bf16, dt in [0.01, 0.21],
    la = -dt * U(0.5, 8.5) per head, gy randn rounded to bf16 and stored as fp32."""
    g = torch.Generator().manual_seed(seed)
    ldx = ldx or H * P + 2 * N
    xbc = (torch.randn(B, L, ldx, generator=g) * 0.5).to(torch.bfloat16)
    dt = torch.rand(B, L, H, generator=g) * 0.2 + 0.01
    la = -dt * (torch.rand(H, generator=g) * 8 + 0.5)
    gy = torch.randn(B, L, H * P, generator=g).to(torch.bfloat16).float()
    return xbc, dt, la, gy


def split_xbc(xbc, H, dtype=torch.float64):
    """xbc (B, L, >= H * 64 + 256) -> x (B, L, H, 64), B (B, L, 128), C (B, L, 128) in `dtype`."""
    Bsz, L, _ = xbc.shape
    d = H * P
    return xbc[..., :d].to(dtype).reshape(Bsz, L, H, P), xbc[..., d:d + N].to(dtype), xbc[..., d + N:d + 2 * N].to(dtype)


def scan_seq(x, Bm, Cm, dt, la, reverse=False):
    """x (B, L, H, 64), Bm / Cm (B, L, 128), dt / la (B, L, H) -> y (B, L, H, 64), in the inputs' dtype, differentiable."""
    if reverse:
        return torch.flip(scan_seq(*(torch.flip(t, [1]) for t in (x, Bm, Cm, dt, la))), [1])
    Bsz, L, H, _ = x.shape
    h = x.new_zeros(Bsz, H, N, P)
    ys = []
    for t in range(L):
        h = h * torch.exp(la[:, t]).view(Bsz, H, 1, 1) + (dt[:, t].view(Bsz, H, 1, 1) * Bm[:, t].view(Bsz, 1, N, 1)
                                                         * x[:, t].view(Bsz, H, 1, P))
        ys.append(torch.einsum("bn,bhnp->bhp", Cm[:, t], h))
    return torch.stack(ys, 1)


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
