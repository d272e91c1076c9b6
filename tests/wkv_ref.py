"""Float64 references of the WKV-6 recurrence and of its backward, and the acceptance rules of the kernels; no GPU code, no
import from the package.

Per head (head size 64; i = value channel, j = key channel, d_t[j] = exp(-exp(w_t[j]))), the formula of
oracle.wkv6_oracle.state_recurrence_f64:
    y_t[i] = sum_j r_t[j] (u[j] k_t[j] v_t[i] + S_t[i][j]) ,      S_{t+1}[i][j] = d_t[j] S_t[i][j] + k_t[j] v_t[i]
so a TERM of y_t[i] is r_t[j] k_s[j] (prod_{s<tau<t} d_tau[j]) v_s[i] for an earlier step s, r_t[j] u[j] k_t[j] v_t[i] (the
bonus), or r_t[j] (prod_{tau<t} d_tau[j]) S_0[i][j].  `recurrence` is that loop, differentiable by autograd; `abs_recurrence`
is the same loop on the operands' magnitudes: the sum of the magnitudes of the terms of each output element, which is what a
kernel's rounding errors scale with.  `grads` / `abs_grads` are float64 autograd of the two.  `accept_*` are the rules the HIP
kernels of csrc/wkv6.hip and csrc/wkv6_mfma.inc are held to (tests/test_wkv6_f64_gpu.py); tests/test_wkv_ref.py checks on
the CPU that the float32 C oracle passes them with room and that planted faults do not.
reverse = True: step s of the recurrence is time index T - 1 - s; inputs and outputs stay at their own time index."""
import functools
import math

import torch

N = 64
RECIPES = ("mid", "slow", "fast")


def make_inputs(B, T, H, seed, dtype, recipe="mid", state=False):
    """r, k, v, w (B, T, 64 H), u (H, 64) (and s0 (B, H, 64, 64) fp32 with state=True).  r, k, v randn * 0.5, u randn * 0.3,
    s0 randn * 0.5 (the scales of tests/test_wkv6_gpu.py); the decay recipes:
        "mid"   w ~ N(-3, 1):   d around 0.95, a term fades over some tens of steps;
        "slow"  w ~ N(-7, 0.5): d around 0.999, every term of the whole sequence survives;
        "fast"  w ~ N(+1, 1) clipped at +3: d between e^-20 and about 0.5, decay products underflow to exactly 0 in fp32.
    Everything is rounded to `dtype` and returned in it; the references read the rounded values as float64."""
    g = torch.Generator().manual_seed(seed)
    C = N * H
    r, k, v = (torch.randn(B, T, C, generator=g) * 0.5 for _ in range(3))
    z = torch.randn(B, T, C, generator=g)
    w = {"mid": z - 3.0, "slow": z * 0.5 - 7.0, "fast": (z + 1.0).clamp(max=3.0)}[recipe]
    u = torch.randn(H, N, generator=g) * 0.3
    out = [t.to(dtype).contiguous() for t in (r, k, v, w, u)]
    if state:
        out.append((torch.randn(B, H, N, N, generator=g) * 0.5).contiguous())
    return out


def make_gy(B, T, H, seed, dtype):
    """The output's gradient of the backward cases: randn rounded to `dtype`."""
    return torch.randn(B, T, N * H, generator=torch.Generator().manual_seed(seed)).to(dtype).contiguous()


def recurrence(r, k, v, w, u, s0=None, reverse=False):
    """(y (B, T, C), S_T (B, H, 64, 64) indexed [value i][key j]) in float64, differentiable.  u is (H, 64), or (B, H, 64) for a
    bonus per batch entry (whose gradient is then per batch entry, as the kernel stores it before the sum over the batch)."""
    if reverse:
        y, S = recurrence(*(torch.flip(t, [1]) for t in (r, k, v, w)), u, s0)
        return torch.flip(y, [1]), S
    B, T, C = r.shape
    H = C // N
    r, k, v, w = (t.double().view(B, T, H, N) for t in (r, k, v, w))
    u = u.double()
    u = (u[None] if u.dim() == 2 else u)[:, :, None, :]
    S = r.new_zeros(B, H, N, N) if s0 is None else s0.double()
    d = torch.exp(-torch.exp(w))
    ys = []
    for t in range(T):
        kv = v[:, t, :, :, None] * k[:, t, :, None, :]                      # (B, H, i, j)
        ys.append(((u * kv + S) * r[:, t, :, None, :]).sum(-1))
        S = S * d[:, t, :, None, :] + kv
    return torch.stack(ys, 1).reshape(B, T, C), S


def abs_recurrence(r, k, v, w, u, s0=None, reverse=False):
    """recurrence on |r|, |k|, |v|, |u|, |s0| with the same w: (yabs, Sabs), the sum of the magnitudes of the terms of each
    element of y and of the final state.  yabs >= |y| elementwise; an error bound relative to yabs is a bound per term."""
    return recurrence(r.abs(), k.abs(), v.abs(), w, u.abs(), None if s0 is None else s0.abs(), reverse)


def _autograd(r, k, v, w, u, gy, s0, reverse):
    B = r.shape[0]
    leaves = [t.detach().double().clone().requires_grad_() for t in (r, k, v, w)]
    ub = u.detach().double()[None].expand(B, -1, -1).clone().requires_grad_()
    leaves.append(ub)
    if s0 is not None:
        leaves.append(s0.detach().double().clone().requires_grad_())
    y, S = recurrence(*leaves[:5], leaves[5] if s0 is not None else None, reverse)
    g = torch.autograd.grad(y, leaves, gy.double().view_as(y), allow_unused=True)
    g = [torch.zeros_like(l) if x is None else x for x, l in zip(g, leaves)]        # T == 1: nothing depends on w
    return dict(y=y.detach(), S=S.detach(), gr=g[0], gk=g[1], gv=g[2], gw=g[3], gu=g[4].sum(0), gu_b=g[4],
                gs=g[5] if s0 is not None else None)


def grads(r, k, v, w, u, gy, s0=None, reverse=False):
    """float64 autograd of `recurrence` under gy: a dict with gr, gk, gv, gw (B, T, C), gu (H, 64), gs (B, H, 64, 64) or None,
    plus gu_b (B, H, 64), the bonus' gradient per batch entry (gu is its sum), and y, S of the forward."""
    return _autograd(r, k, v, w, u, gy, s0, reverse)


def abs_grads(r, k, v, w, u, gy, s0=None, reverse=False):
    """|autograd| of `abs_recurrence` under |gy|, the keys of `grads`.  Every term of a gradient of the all-positive problem
    has one sign, so for gr, gk, gv, gu, gs this IS the sum of the magnitudes of the terms of each gradient element; for gw
    (d/dw of d = exp(-e^w) is -e^w d) it is e^w times that sum."""
    out = _autograd(r.abs(), k.abs(), v.abs(), w, u.abs(), gy.abs(), None if s0 is None else s0.abs(), reverse)
    return {key: (None if val is None else val.abs()) for key, val in out.items()}


# ---- acceptance rules ---------------------------------------------------------------------------------------------------------

REL_Y = 7 * 2.0 ** -16      # derived in accept_y
REL_G = 7 * 2.0 ** -16      # derived in accept_grad


def _log(name, **values):
    """To the parity log; a ratio also as its log2 (the log keeps nine decimals).  The CPU tests that expect a rule to refuse
    something call the rules with log=False: what they measure is no kernel's."""
    from tests import parity_log
    for key, val in list(values.items()):
        if isinstance(val, float) and "_over_" in key and val > 0:
            values["log2_" + key] = math.log2(val)
    parity_log.record(name, **values)


def _accept_elementwise(got, ref, mag, rel, name, what, log=True):
    got, ref, mag = got.double(), ref.double(), mag.double()
    assert got.shape == ref.shape == mag.shape, (name, got.shape, ref.shape, mag.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    worst = float((err / (mag + 1e-30 / rel)).max()) if err.numel() else 0.0
    if log:
        _log(name, **{what: worst, "bound": rel})
    print(f"{name}: max |err| / {what.split('_over_')[1]} {worst:.3g} = 2^{math.log2(max(worst, 1e-300)):.1f} (bound {rel:.3g})")
    assert bool((err <= rel * mag + 1e-30).all()), (name, worst, rel)
    return worst


def accept_y(got, ref, yabs, name="wkv6 y", log=True):
    """The acceptance rule of the WKV-6 forward kernels against float64, elementwise:
        |got - ref| <= REL_Y * yabs + 1e-30,        yabs = abs_recurrence(...)[0], REL_Y = 7 * 2^-16 (one constant for fp32 and bf16 I/O)
    REL_Y is derived from the kernels' arithmetic (csrc/wkv6_mfma.inc, DESIGN.md "The scan on the matrix cores"), per term of
    y_t[i].  A bf16 matrix-core product takes an fp32 operand a in [2^e, 2^(e+1)) as hi + lo, hi = bf16(a), lo = bf16(a - hi),
    both rounded to nearest.  bf16 has 8 significant bits: |a - hi| <= 2^(e-8); a remainder of exactly 2^(e-8) is a bf16 value,
    and below it bf16's half step is at most 2^(e-17).  So the operand keeps 16 significant bits, |a - hi - lo| <= 2^-17 |a| (the
    figure DESIGN.md quotes; a = 1.00376 splits into 1 + 0.00376, which bf16 holds to 7.6e-6 = 2^-17), and the product
    hi hi + lo hi + hi lo leaves out lo lo <= 2^-16 |a b|.  A product of two split operands is therefore off by at most
    2 * 2^-17 + 2^-16 = 2 * 2^-16 of each of its terms, a product of a split and an exact bf16 operand by 2^-17.  (The dropped
    lo lo is the larger half of that: a final-state element that is a single product k v, both split, is observed 1.45 * 2^-16
    off on the GPU.)
      * operand splits.  bf16 I/O: a term from an earlier step of the same 16-step block goes through the level product
        X_b = c_b c_b^T (both operands split: 2 * 2^-16) and through X v (X split, v exact: 2^-17); a term from an earlier block
        goes through the state update (k G_4) v^T (k G_4 split, v exact: 2^-17) -- in pass C, or in pass A followed by the chunk
        scan -- and, once, through the inter-block product (r E_4) S0 of the block of t (both split: 2 * 2^-16); the state itself
        stays fp32 in the accumulators between blocks; the bonus goes through no split product.  fp32 I/O: the three products
        that feed y run on the fp32 matrix instructions and only the state update is split (both operands: 2 * 2^-16).  The VALU
        formulation has no split at all.  At most 2.5 * 2^-16 per term.
      * fp32 roundings.  The decay of a term is a product of at most four level factors E_b / G_b, the block decay and the
        chunk decay, each a chain of at most 4 multiplies (with the scaling of the operand about 14 roundings of the term);
        the chunk scan's fmaf rounds once per chunk crossed; and while the term sits in an fp32 accumulator at most 64
        (channels) + 16 (steps) + the blocks of a chunk + the chunks crossed (<= 19 + 18 in every case here) further additions
        round a partial sum that is at most yabs.  Below 128 * 2^-24 = 2^-17 of yabs.
      * __expf in d = exp(-exp(w)).  v_exp_f32 is good to 1 ulp: for d in [0.5, 1) that is 2^-24 relative, and the error of the
        inner e^w (relative (|w| + 2) 2^-24) moves log d by e^w times that; per step at most 1.3 * 2^-24 for w <= -2, and a
        term under stronger decay is gone after a few steps.  A term decayed over n steps carries n of these: its share GROWS
        LINEARLY with n, 1.3 * n * 2^-24 of the term, so against yabs the exp's share is 1.3 * 2^-24 times the |term|-weighted
        mean number of decayed steps.  That mean is at most the sequence length under the "slow" recipe (used up to T = 83) and
        a few tens under "mid" (E e^w = 0.08 per step): at most 100 steps in every case these rules are used on, 2^-17.  A test
        that runs hundreds of slowly decayed steps has to add the share of its own length.
    Together 2.5 * 2^-16 + 2^-17 + 2^-17 = 3.5 * 2^-16 per term; the bound allows twice that.  These are worst cases per term; an
    output sums many terms whose roundings do not line up, and the kernels are observed at 2^-17.6 of yabs (the parity log has
    the ratio of every case).  (1e-30: terms whose decay underflows in fp32.)"""
    return _accept_elementwise(got, ref, yabs, REL_Y, name, "err_over_yabs", log)


def accept_state(got, ref, Sabs, name="wkv6 state", log=True):
    """The final state against float64, elementwise: |got - ref| <= REL_Y * Sabs + 1e-30, Sabs = abs_recurrence(...)[1].  A term
    of the state passes through a subset of what a term of y passes through (the state update, the chunk scan, the decay
    products; no inter-block product: at most 2 * 2^-16 of splits), so accept_y's constant covers it."""
    return _accept_elementwise(got, ref, Sabs, REL_Y, name, "err_over_Sabs", log)


def _outside_interval(got, ref, tol):
    got, ref, tol = got.double(), ref.double(), tol.double()
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    assert bool(torch.isfinite(got).all())
    lo, hi = (ref - tol).float().to(torch.bfloat16).double(), (ref + tol).float().to(torch.bfloat16).double()
    return torch.maximum(lo - got, got - hi).clamp_min(0), lo, hi             # distance outside the interval


def accept_y_bf16(got, ref, tol, name="wkv6 y bf16", log=True):
    """A bf16 output of a value known to within `tol` of `ref` (the interval form of ssd_ref.scan_accept_bf16): every element
    must lie between the bf16 roundings of ref - tol and ref + tol; for y, tol = REL_Y * yabs.  Recorded: how many elements lie
    outside and by how much of |ref|, and where inside the interval's tolerance the stored values sit (|got - ref| / (tol +
    half a bf16 step), at most about 1 for an accepted output)."""
    out, lo, hi = _outside_interval(got, ref, tol)
    worst = float((out / ref.double().abs().clamp_min(1e-30)).max()) if out.numel() else 0.0
    used = float(((got.double() - ref.double()).abs() / (tol.double() + 2.0 ** -9 * ref.double().abs() + 1e-30)).max()) if out.numel() else 0.0
    if log:
        _log(name, outside_interval_over_ref=worst, elements_outside=int((out > 0).sum()), err_over_tol_plus_half_step=used)
    print(f"{name}: {int((out > 0).sum())} of {out.numel()} elements outside the rounded interval, worst by {worst:.3g} |ref|; "
          f"max |err| / (tol + half a bf16 step) {used:.3g}")
    assert bool((out == 0).all()), (name, worst)
    return worst


def accept_grad(name, got, ref, gabs, batch_sum=False, log=True):
    """gr, gk, gv, gu, gs against float64 autograd, elementwise:  |got - ref| <= REL_G * gabs + 1e-30, gabs = abs_grads(...);
    a bf16 output in the interval form of accept_y_bf16 with tol = REL_G * gabs.  REL_G = 7 * 2^-16, from the backward's
    arithmetic (csrc/wkv6.hip, launch_bwd).  It runs the forward kernels on (k, v) for the chunk states of S and on (r, gy), in
    reversed time, for those of its adjoint G: gv IS that second forward's output and gs its final state, so accept_y's
    3.5 * 2^-16 per term is their figure.  For gr and gk, wkv6_row_kernel then walks every chunk in fp32 from its incoming
    state, st = fmaf(st, d, a p) and a 64-term dot per step, so a term of P (gr) or Q (gk) carries
      * the split of pass A's state update where it crossed a chunk seam (bf16: 2^-17; fp32, both operands split: 2 * 2^-16);
      * one fp32 rounding per step it is decayed over, n * 2^-24 for n steps; with the |term|-weighted mean of n at most 100
        as in accept_y: 0.4 * 2^-16;
      * the exp's share of accept_y, 2^-17, and the other fp32 roundings (the chunk scan, the dot's 16 + 2 additions, the
        epilogue's fmaf for the bonus term; gu summed over at most 24 steps per time chunk and 64 chunks), 2^-17:
    3.4 * 2^-16, below gv's figure.  One constant, 3.5 * 2^-16 per term; the bound allows twice that.
    batch_sum (gu): ref and gabs are per batch entry, (B, H, 64); the kernel stores each entry's sum in the output's dtype and
    the caller adds the B entries in fp32 (then one more rounding to the dtype): got (H, 64) is compared with the sum over the
    entries, each rounded where the kernel rounds it; the fp32 sum's B - 1 additions each round a partial sum that is at most
    the sum of the entries' magnitudes, (B - 1) * 2^-24 of it."""
    if got.dtype != torch.bfloat16:
        if batch_sum:
            ref, gabs = ref.sum(0), gabs.sum(0)
        return _accept_elementwise(got, ref, gabs, REL_G, name, "err_over_gabs", log)
    tol = REL_G * gabs.double()
    if batch_sum:                                  # the interval of the sum of the per-entry bf16 roundings, summed in fp32
        rnd = lambda t: t.float().to(torch.bfloat16).double()
        lo_b, hi_b = rnd(ref.double() - tol), rnd(ref.double() + tol)
        lo, hi = lo_b.sum(0), hi_b.sum(0)
        slack = (ref.shape[0] - 1) * 2.0 ** -24 * torch.maximum(lo_b.abs(), hi_b.abs()).sum(0)
        ref, tol = (lo + hi) / 2, (hi - lo) / 2 + slack
    return accept_y_bf16(got, ref, tol, name, log)


def gw_zero_steps(T, has_state, reverse=False):
    """Time indices whose gw the kernel stores as exact zeros: the recurrence's last step (nothing after it) and, without an
    initial state, its first (nothing to decay)."""
    steps = {T - 1} | (set() if has_state else {0})
    return sorted((T - 1 - s) if reverse else s for s in steps)


def per_head_max(t, H):
    """max |t| over time and channels per (batch, head): (B, T, 64 H) -> (B, H)."""
    B, T, _ = t.shape
    return t.double().abs().view(B, T, H, N).amax((1, 3))


def accept_gw(got, ref, gabs_w, oracle_err, name="wkv6 gw", zero_steps=()):
    """gw is judged per (batch, head), not per element:
        max over the head |got - ref|  <=  4 * max(oracle_err_head, REL_G * max over the head of gabs_w)
    Why not per element: the kernel forms gw_t = Z_t * (-e^{w_t}) with Z_t a PREFIX SUM over time of signed per-step terms
    (csrc/wkv6.hip, wkv6_bwd_epilogue_kernel; the reference's sbbbb / sss recursion is the same sum): the terms cancel, so the
    rounding of Z_t scales with the terms summed so far, not with the terms of gw_t itself -- under strong decay gw_t is tiny
    and Z_t is not.  The cancellation is in the algorithm and in the reference's as well, so the yardstick is the reference:
    oracle_err (B, H) is the error of the float32 C oracle (oracle.wkv6_oracle.backward) on the same case against float64, per
    head; REL_G * max gabs_w keeps the rule from asking more than accept_grad where the oracle happens to be exact; the margin
    4 is the project's factor (tests/test_mha_rows_gpu.py) for a different summation order and the device's exp.  The rule
    is set from the reference, never from the kernel.  A bf16 output is held to the interval form with the head's bound as
    tol.  `zero_steps`: time indices that must be stored as exact zeros (gw_zero_steps)."""
    B, T, C = ref.shape
    H = C // N
    assert got.shape == ref.shape == gabs_w.shape and oracle_err.shape == (B, H), (got.shape, ref.shape, oracle_err.shape)
    assert bool(torch.isfinite(got).all()), name
    for t in zero_steps:
        assert float(got[:, t].double().abs().max()) == 0.0, (name, "gw must be an exact zero at step", t)
    floor = REL_G * per_head_max(gabs_w, H)
    bound = 4 * torch.maximum(oracle_err.double(), floor)
    kern = per_head_max(got.double() - ref.double(), H)
    heads = lambda t: [round(float(x), 12) for x in t.flatten()]
    print(f"{name}: per-head max |err| kernel {heads(kern)} oracle {heads(oracle_err)} floor {heads(floor)}")
    if got.dtype == torch.bfloat16:      # the stored value carries its own rounding: the interval form, per head
        tol = bound.view(B, 1, H, 1).expand(B, T, H, N).reshape(B, T, C)
        out, _, _ = _outside_interval(got, ref, tol)
        _log(name, kernel_err_per_head=heads(kern), oracle_err_per_head=heads(oracle_err), floor_per_head=heads(floor),
             elements_outside=int((out > 0).sum()))
        assert bool((out == 0).all()), (name, float(out.max()))
        return 0.0
    worst = float((kern / bound.clamp_min(1e-300)).max())
    _log(name, kernel_err_per_head=heads(kern), oracle_err_per_head=heads(oracle_err), floor_per_head=heads(floor),
         worst_err_over_bound=worst)
    assert bool((kern <= bound).all()), (name, kern.tolist(), bound.tolist())
    return worst


# ---- the kernel tests' cases: inputs and float64 references, computed once -------------------------------------------------------

def _seed(B, T, H, recipe):
    return 7000 + 131 * T + 17 * H + B + 1000 * RECIPES.index(recipe)


@functools.lru_cache(maxsize=None)
def forward_case(B, T, H, dtype, recipe="mid", reverse=False, state=False, variant=0):
    """(inputs, y, S, yabs, Sabs): make_inputs and the float64 forward of one case; shared by the fp32 / bf16 kernel tests of a
    path and by tests/test_wkv_ref.py.  Nothing of it may be modified.  variant: another draw of the same case."""
    a = make_inputs(B, T, H, _seed(B, T, H, recipe) + 50000 * variant, dtype, recipe, state)
    s0 = a[5] if state else None
    with torch.no_grad():
        y, S = recurrence(*a[:5], s0, reverse)
        yabs, Sabs = abs_recurrence(*a[:5], s0, reverse)
    return a, y, S, yabs, Sabs


def oracle_gw_err(a, gy, ref_gw, reverse):
    """Per-head error (B, H) of the float32 C oracle's gw against float64 on the operands `a` (zero initial state: the C
    restatement of the reference's backward has no other).  reverse: the oracle runs the flipped problem."""
    from oracle import wkv6_oracle as WO
    fl = (lambda t: torch.flip(t, [1]).contiguous()) if reverse else (lambda t: t)
    out = WO.backward(*(fl(t.float()) for t in a[:4]), a[4].float().contiguous(), fl(gy.float()))
    return per_head_max(fl(out[3]).double() - ref_gw, a[4].shape[0]), out


@functools.lru_cache(maxsize=None)
def backward_case(B, T, H, dtype, recipe="mid", reverse=False, state=False):
    """(inputs, gy, grads, abs_grads, oracle_gw_err (B, H)) of one backward case.  With an initial state the oracle's gw error is
    taken on the same operands from a zero state (it has no state entry); the floor REL_G * gabs_w carries the state's terms."""
    a = make_inputs(B, T, H, _seed(B, T, H, recipe) + 500, dtype, recipe, state)
    gy = make_gy(B, T, H, _seed(B, T, H, recipe) + 900, dtype)
    s0 = a[5] if state else None
    ref = grads(*a[:5], gy, s0, reverse)
    mag = abs_grads(*a[:5], gy, s0, reverse)
    ref_gw0 = ref["gw"] if not state else grads(*a[:5], gy, None, reverse)["gw"]
    oerr, _ = oracle_gw_err(a, gy, ref_gw0, reverse)
    return a, gy, ref, mag, oerr


# (B, T, H, chunk_len) of tests/test_wkv6_f64_gpu.py; the cases in *_ALL_RECIPES also run on "slow" and "fast"
FORWARD_CASES = [(1, 1, 1, 0), (2, 15, 2, 0), (2, 16, 2, 0), (2, 17, 2, 0), (1, 33, 1, 16), (2, 83, 3, 32), (1, 64, 1, 16),
                 (2, 45, 3, 24), (1, 40, 8, 16), (3, 37, 2, 10 ** 6), (1, 130, 2, 0)]
FORWARD_ALL_RECIPES = [(2, 83, 3, 32), (2, 17, 2, 0)]
BACKWARD_CASES = [(1, 1, 1, 0), (2, 2, 1, 0), (2, 17, 2, 0), (2, 37, 2, 8), (1, 83, 3, 32), (1, 150, 2, 0), (1, 1100, 1, 0)]
BACKWARD_ALL_RECIPES = [(2, 37, 2, 8)]


def matrix(cases, all_recipes):
    """[(B, T, H, chunk_len, recipe)]: every case on "mid", the cases of `all_recipes` on "slow" and "fast" as well."""
    return [c + ("mid",) for c in cases] + [c + (rcp,) for c in all_recipes for rcp in ("slow", "fast")]
