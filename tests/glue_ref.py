"""float64 specification of the conv-module and LayerNorm glue kernels (csrc/glue.hip: add_layernorm_kernel, split_planes_kernel;
csrc/dwconv.hip: dwconv_kernel ACT 0-3, dwconv_wgrad_kernel + its reduce) and a derived per-element bound.  Plain torch, CPU or
GPU, no kernels of this package.

Every `*_rounded` function evaluates each operation exactly in float64 and rounds only where the kernels' comments and the module
chain (convolution.py:109-141) store a tensor.  rb = nearest bf16 (tests/tmix_ref.py), r32 = nearest float32; rX / rO below are
the rounding of the residual dtype / of the LayerNorm-output dtype, rET that of the convolution's element type.

add_layernorm     y' = y with the rows t >= lens[b] zeroed (mask_y: the masked_fill of convolution.py:140-141)
                  x_new = rX(x + rX(alpha y'))           no inner rounding when alpha == 1; alpha is a float32
                  LN(v) = (v - mean) rsqrt(var + eps) gamma + beta,  mean and var (divisor C) exact over the row
                  o1 = rO(LN1(x_new)); silu: o1 = rO(silu(o1)); zero_rows: rows t >= lens[b] are 0 (convolution.py:109-111)
                  o2 = rO(LN2(o1 as stored))             a plane output stores the fp32 value v: its o1 "as stored" is v
                  stats_x / stats_out1 = (sum, sum of squares) of x_new / of o1 in pair 0 of 8, pairs 1-7 exact zeros
                  planes of an fp32 value v: hi = rb(v), lo = rb(v - hi)
dwconv forward    in = x with the frames s >= lens[b] zeroed; ACT 1 (GLU, convolution.py:130): in = rET(value sigmoid(gate)),
                  x = [value | gate]
                  conv[t][c] = bias[c] + sum_k w[c][k] in[t - left_pad + k][c],  zero outside 0 <= s < T_in (convolution.py:133)
                  ACT 0, 1: y = rET(conv)        ACT 2: y = rET(silu(rET(conv)))
                  ACT 3 (convolution.py:134-138): u = rb(conv), o = rb(LN(u)), y = rb(silu(o))
dwconv wgrad      dw[c][k] = sum_{b, t < T_out} dy[b][t][c] x[b][t + k - left_pad][c],  db[c] = sum_{b, t} dy[b][t][c]: exact sums
split_planes      hi = rb(x), lo = rb(x - hi); double form [hi | lo] with lo at column lo_off, triple form [hi | hi | lo]

THE BOUND.  u = 2^-24.  A correct kernel works in fp32: before each rounding it holds the exact value a up to an error E that is
derived here from the fp32 operations behind it, and then rounds once.  Rounding is monotone, so its stored value lies in
[r(a - E), r(a + E)]; the bound of an element is the distance of the reference r(a) from the farther end.  It is zero wherever
no midpoint of the output grid lies within E of a: such elements must be bit-identical.  An intermediate the kernel formed
itself (x_new, o1 feeding LN2 and the statistics, the GLU product and the rounded convolution feeding ACT 2 / 3) may sit at
either end of its own interval; that deviation d is an input error of what follows, as tests/tmix_ref.py carries m_q and td.

  sums         n terms added in fp32 in any order, each term an exact product (the two factors of a fused multiply-add are not
               rounded): at most n - 1 roundings on the way of any term, each relative u of a partial sum that is at most
               S = sum |terms|, plus the store / one scaling: (n + 2) u S.  n = C for the row statistics (+1: the product
               with 1 / C, whose own rounding is another u), K for the taps (+ the bias the accumulator starts from), B T_out
               for the weight gradient (frames beyond T_out and partials of other blocks add exact zeros or are terms of the
               same sum).
  x_new        a product and a sum of two numbers are single, correctly rounded fp32 operations, so the kernel's own x_new is
               known exactly: bf16 rb(r32(x + rb(r32(alpha y')))) (a value rounded to fp32 and then to bf16 may land a step
               from rb of the exact one), fp32 r32(x + r32(alpha y')) or, the product contracted into the add, r32(x + alpha y').
               The bound is the distance of these from the reference: zero for alpha == 1 in fp32, and wherever the
               exact sum fits fp32.
  LayerNorm    input v with |v~ - v| <= d:
                 mean   Em = mean(d) + (C + 2) u mean(|v| + d)
                 centre Ec = d + Em + u (|c| + d + Em)                          c = v - mean, one subtraction
                 var    Ev = mean(Ec (2 |c| + Ec)) + (C + 3) u mean((|c| + Ec)^2)
                 rstd   Er = Ev / 2 (max(var - Ev, 0) + eps)^-3/2 + 4 u rstd    d/dx x^-1/2 = -x^-3/2 / 2, decreasing in x; the
                                                                                 add of eps, the 1-ulp hardware rsqrt: 4 u
                 value  E  = |gamma| (Ec rstd + (|c| + Ec) Er + 2 u |c| rstd) + u (|c rstd gamma| + |beta|)
  sigmoid      1 / (1 + e), e = exp(-x) from the hardware exp2: the rounded product x log2(e) moves e by a relative 2 |x| u, exp2,
               the add and the division are 1 u each.  sigmoid is within (2 |x| + 4) u sigmoid(x) + the activation term; the
               GLU product one more u.  Lipschitz constants: sigmoid 1/4, SiLU 1.1 (sup |silu'| = 1.0998 at x = 2.3994).
  SiLU         x sigmoid(x) or x / (1 + e): (2 |x| + 6) u |silu(x)| + the activation term + 1.1 d
  activation   term: 4 x the worst |float32 torch - float64 torch| of the function over the case's own arguments
               (as gemm_ref.activation_term: a number of torch's, not of the kernel)
  planes       hi + lo of a kernel's fp32 value v~ reproduces v~ to 2^-16 |v~| (|v~ - hi| <= 2^-8 |v~|, lo rounds that once more):
               bound(v) + 2^-16 (|v| + bound(v)) against the fp32 reference value; |lo| <= half a bf16 step of hi.
  split_planes no bound: x - hi is exact in fp32, hi and lo are bit-exact.

No constant above is fitted to a kernel, and no element is excluded: every element has to be within its own bound (rows whose
input is NaN by construction have a NaN reference, and the kernel's element has to be NaN as well).  tests/test_glue_ref.py
checks on the CPU that the same chains in float32 torch stay within the bound, and that a list of plausible kernel mistakes
does not."""
import torch
import torch.nn.functional as F

from tests.tmix_ref import rb

U32 = 2.0 ** -24
SILU_LIP = 1.1
BF16, F32 = torch.bfloat16, torch.float32


def r32(v: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest float32 (ties to even, subnormals kept), as float64."""
    return v.to(torch.float32).to(torch.float64)


ROUND = {BF16: rb, F32: r32}


def silu(v):
    return v * torch.sigmoid(v)


def activation_term(fn, pre: torch.Tensor) -> float:
    """4 x the worst |fn in float32 - fn in float64| over the finite values of pre (the CPU's float32 kernels)."""
    pre = pre.detach().double().cpu().flatten()
    pre = pre[torch.isfinite(pre)]
    if not pre.numel():
        return 0.0
    return 4.0 * float((fn(pre.float()).double() - fn(pre)).abs().max())


def _iv(a, E, r):
    return r(a - E), r(a + E)


def _dev(ref, lo, hi):
    return torch.maximum(hi - ref, ref - lo)


def _silu_err(o, d):
    return SILU_LIP * d + (2 * o.abs() + 6) * U32 * silu(o).abs() + activation_term(silu, o)


def planes(v: torch.Tensor):
    """fp32 value (as float64) -> (hi, lo) bf16 planes (as float64)."""
    hi = rb(v)
    return hi, rb(v - hi)


def planes_bound(v: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """hi + lo of a kernel's planes against the fp32 reference value v whose own bound is b."""
    return b + 2.0 ** -16 * (v.abs() + b)


def bf16_half_step(hi: torch.Tensor) -> torch.Tensor:
    """Half the distance between hi (a bf16 value, as float64) and its neighbour away from zero; 0 maps to 0."""
    e = torch.floor(torch.log2(hi.abs().clamp_min(2.0 ** -126)))
    return torch.where(hi == 0, torch.zeros_like(hi), torch.exp2(e - 8))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------

def _ln(v, g, b, eps):
    m = v.mean(-1, keepdim=True)
    c = v - m
    var = (c * c).mean(-1, keepdim=True)
    r = (var + eps) ** -0.5
    return c * r * g + b, (c, var, r)


def _ln_err(v, d, g, b, eps):
    """E of the docstring: what a correct fp32 LayerNorm of v~, |v~ - v| <= d, may be away from the exact one of v."""
    C = v.shape[-1]
    a, (c, var, r) = _ln(v, g, b, eps)
    mean = lambda t: t.mean(-1, keepdim=True)
    Em = mean(d) + (C + 2) * U32 * mean(v.abs() + d)
    Ec = d + Em + U32 * (c.abs() + d + Em)
    Ev = mean(Ec * (2 * c.abs() + Ec)) + (C + 3) * U32 * mean((c.abs() + Ec) ** 2)
    Er = 0.5 * Ev * ((var - Ev).clamp_min(0) + eps) ** -1.5 + 4 * U32 * r
    return a, g.abs() * (Ec * r + (c.abs() + Ec) * Er + 2 * U32 * c.abs() * r) + U32 * ((c * r * g).abs() + b.abs())


def _stats(v, d):
    """(rows, 8, 2) statistics of v and their bound, the kernel's own v~ within d of v."""
    C = v.shape[-1]
    st = torch.zeros(v.shape[0], 8, 2, dtype=torch.float64, device=v.device)
    bd = torch.zeros_like(st)
    st[:, 0, 0], st[:, 0, 1] = v.sum(-1), (v * v).sum(-1)
    w = v.abs() + d
    bd[:, 0, 0] = d.sum(-1) + (C + 2) * U32 * w.sum(-1)
    bd[:, 0, 1] = (d * (2 * v.abs() + d)).sum(-1) + (C + 2) * U32 * (w * w).sum(-1)
    return st, bd


def rows_beyond(rows: int, lens, T: int, device) -> torch.Tensor:
    """(rows, 1) bool: row r = b T + t has t >= lens[b]."""
    if lens is None:
        return torch.zeros(rows, 1, dtype=torch.bool, device=device)
    i = torch.arange(rows, device=device)
    return (i % T >= lens.long().to(device)[i // T]).unsqueeze(1)


def add_layernorm_rounded(x, y, alpha, g1, b1, out_dtype=None, *, lens=None, T=0, mask_y=False, silu_=False, zero_rows=False,
                          g2=None, b2=None, eps=1e-5) -> dict:
    """x, y, gamma, beta in the residual dtype (fp32 or bf16), out_dtype that of the LayerNorm outputs.  -> x_new, o1, o2 (rows, C),
    stats_x, stats_o1 (rows, 8, 2) in float64, and under "_bound" the bound of each."""
    rX, rO = ROUND[x.dtype], ROUND[out_dtype or x.dtype]
    C = x.shape[-1]
    X = x.double().reshape(-1, C)
    beyond = rows_beyond(X.shape[0], lens, T, X.device)
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    g1, b1 = g1.double(), b1.double()
    out, bnd = {}, {}
    if y is not None:
        a32 = float(torch.tensor(float(alpha), dtype=torch.float32))
        Y = y.double().reshape(-1, C)
        if mask_y:
            Y = torch.where(beyond, zero, Y)
        pe = a32 * Y
        p = pe if a32 == 1.0 else rX(pe)
        xn = rX(X + p)
        # the kernel's own: every fp32 operation is correctly rounded, so it is one of these
        if x.dtype == BF16:
            own = [rb(r32(X + rb(r32(pe))))]
        else:
            own = [r32(X + r32(pe)), r32(X + pe)]
        d_x = torch.stack([(o - xn).abs() for o in own]).amax(0)
    else:
        xn, d_x = X, torch.zeros_like(X)
    out["x_new"], bnd["x_new"] = xn, d_x
    out["stats_x"], bnd["stats_x"] = _stats(xn, d_x)
    a1, E1 = _ln_err(xn, d_x, g1, b1, eps)
    o1 = rO(a1)
    lo, hi = _iv(a1, E1, rO)
    if silu_:
        s = silu(o1)
        lo, hi = _iv(s, _silu_err(o1, _dev(o1, lo, hi)), rO)
        o1 = rO(s)
    if zero_rows:
        o1, lo, hi = (torch.where(beyond, zero, t) for t in (o1, lo, hi))
    d1 = _dev(o1, lo, hi)
    out["o1"], bnd["o1"] = o1, d1
    out["stats_o1"], bnd["stats_o1"] = _stats(o1, d1)
    if g2 is not None:
        a2, E2 = _ln_err(o1, d1, g2.double(), b2.double(), eps)
        out["o2"] = rO(a2)
        bnd["o2"] = _dev(out["o2"], *_iv(a2, E2, rO))
    out["_bound"] = bnd
    return out


# ---- depthwise convolution -----------------------------------------------------------------------------------------------

def _windows(v, K, left_pad, T_out):
    """(B, T_in, C) -> (B, T_out, C, K): frame t - left_pad + k, zero outside."""
    right = max(0, T_out + K - 1 - left_pad - v.shape[1])
    return F.pad(v, (0, 0, left_pad, right)).unfold(1, K, 1)[:, :T_out]


def conv_input(x, C, act, lens):
    """The convolution's input (B, T_in, C) as stored, and how far a correct kernel's own may be from it."""
    r = ROUND[x.dtype]
    X = x.double()
    T_in = X.shape[1]
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    valid = torch.ones(X.shape[:2], dtype=torch.bool, device=X.device)
    if lens is not None:
        valid = torch.arange(T_in, device=X.device)[None, :] < lens.long().to(X.device)[:, None]
    X = torch.where(valid.unsqueeze(-1), X, zero)
    if act != 1:
        return X[..., :C], torch.zeros_like(X[..., :C])
    val, gate = X[..., :C], X[..., C:2 * C]
    sg = torch.sigmoid(gate)
    a = val * sg
    E = val.abs() * ((2 * gate.abs() + 4) * U32 * sg + activation_term(torch.sigmoid, gate)) + U32 * a.abs()
    return r(a), _dev(r(a), *_iv(a, E, r))


def dwconv_rounded(x, w, bias, left_pad, T_out, act=0, lens=None, gamma=None, beta=None, eps=1e-5) -> dict:
    """x (B, T_in, C) [ACT 1: (B, T_in, 2C)], w (C, 1, K), bias (C) or None -> "y" (B, T_out, C) in float64 and "_bound"."""
    r = ROUND[x.dtype]
    C, K = w.shape[0], w.shape[-1]
    W = w.double().view(C, K)
    inp, d_in = conv_input(x, C, act, lens)
    bv = bias.double() if bias is not None else torch.zeros(C, dtype=torch.float64, device=inp.device)
    win = _windows(inp, K, left_pad, T_out)
    conv = (win * W).sum(-1) + bv
    D = (_windows(d_in, K, left_pad, T_out) * W.abs()).sum(-1)
    Ec = D + (K + 2) * U32 * ((win.abs() * W.abs()).sum(-1) + bv.abs() + D)
    u = r(conv)
    ulo, uhi = _iv(conv, Ec, r)
    if act in (0, 1):
        return {"y": u, "_bound": {"y": _dev(u, ulo, uhi)}, "conv": conv}
    if act == 3:
        a, E = _ln_err(u, _dev(u, ulo, uhi), gamma.double(), beta.double(), eps)
        u = r(a)
        ulo, uhi = _iv(a, E, r)
    s = silu(u)
    y = r(s)
    return {"y": y, "_bound": {"y": _dev(y, *_iv(s, _silu_err(u, _dev(u, ulo, uhi)), r))}, "conv": conv}


def dwconv_wgrad_rounded(x, dy, K, left_pad) -> dict:
    """x (B, T_in, C), dy (B, T_out, C) -> dw (C, 1, K), db (C) in float64 and "_bound"."""
    B, T_out, C = dy.shape
    win = _windows(x.double(), K, left_pad, T_out)
    G = dy.double()
    n = B * T_out
    dw = torch.einsum("btck,btc->ck", win, G).view(C, 1, K)
    S = torch.einsum("btck,btc->ck", win.abs(), G.abs()).view(C, 1, K)
    return {"dw": dw, "db": G.sum((0, 1)), "_bound": {"dw": (n + 2) * U32 * S, "db": (n + 2) * U32 * G.abs().sum((0, 1))}}


def split_planes_rounded(x, triple=False):
    hi, lo = planes(x.double())
    return torch.cat([hi, hi, lo] if triple else [hi, lo], -1)


def bound(ref: dict, name: str) -> torch.Tensor:
    """Per-element distance a correct kernel may have from ref[name]; ref is what a *_rounded function returned."""
    return ref["_bound"][name]


def worst_ratio(got: torch.Tensor, want: torch.Tensor, bnd: torch.Tensor) -> float:
    """max(err / bound) over ALL elements: an element off a zero bound, or not NaN where the reference is NaN (a row whose
    input is NaN by construction), or NaN where the reference is not, counts as infinite."""
    got, want, bnd = got.double().reshape(-1), want.reshape(-1), bnd.reshape(-1)
    assert got.shape == want.shape == bnd.shape, (got.shape, want.shape, bnd.shape)
    nan = torch.isnan(want)
    err = (got - want).abs()
    ratio = torch.where(bnd > 0, err / bnd, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(nan, torch.where(torch.isnan(got), torch.zeros_like(err), torch.full_like(err, float("inf"))), ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(err, float("inf")), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- the cases both test files run -------------------------------------------------------------------------------------------

LN_WIDTHS = [8, 72, 504, 512, 520, 1024]
LN_ROWS = [(1, 1), (1, 3), (1, 4), (1, 5), (3, 7)]         # (B, T): four rows make a block; (3, 7) with lens [7, 3, 1]
LN_PAIRS = ["f32", "bf16", "f32->bf16", "split1", "split2"]
# every call of transformer/fused.py and each switch alone: keyword -> value (y: has a branch output; nan: NaN beyond lens in "y" / "x")
LN_FORMS = {
    "plain": dict(),
    "y alpha 1": dict(y=True),
    "y alpha 0.5": dict(y=True, alpha=0.5),
    "want_x False": dict(y=True, want_x=False),
    "stats only": dict(want_ln=False, stats_x=True),
    "silu": dict(silu=True),
    "zero_rows": dict(lens=True, zero_rows=True),
    "mask_y": dict(y=True, lens=True, mask_y=True, nan="y"),
    "zero mask silu": dict(y=True, lens=True, zero_rows=True, mask_y=True, silu=True, nan="y"),
    "y zero_rows": dict(y=True, lens=True, zero_rows=True),
    "zero_rows nan x": dict(y=True, lens=True, zero_rows=True, mask_y=True, nan="xy"),
    "ln2": dict(ln2=True),
    "y ln2 silu": dict(y=True, ln2=True, silu=True),
    "out1 slice": dict(slice=True),
    "both stats": dict(y=True, stats_x=True, stats_o1=True),
    "mean 40": dict(y=True, ln2=True, mean=40.0, stats_x=True),
}


def ln_lens(B, T):
    return [7, 3, 1] if (B, T) == (3, 7) else [T - 1] * B


def make_ln_case(C, B, T, pair, form, seed=0, device="cpu", nan=True) -> dict:
    """Seeded operands of one add_layernorm call.  pair: LN_PAIRS; form: a key of LN_FORMS."""
    f = dict(LN_FORMS[form])
    xdt = BF16 if pair == "bf16" else F32
    odt = F32 if pair in ("f32", "split1", "split2") else BF16
    g = torch.Generator().manual_seed(1000 * C + 10 * B * T + seed)
    rnd = lambda *s: torch.randn(s, generator=g)
    put = lambda t: t.to(xdt).to(device)
    c = dict(C=C, B=B, T=T, pair=pair, form=form, xdt=xdt, odt=odt, alpha=f.get("alpha", 1.0), silu=f.get("silu", False),
             zero_rows=f.get("zero_rows", False), mask_y=f.get("mask_y", False), want_x=f.get("want_x", True),
             want_ln=f.get("want_ln", True), stats_x=f.get("stats_x", False), stats_o1=f.get("stats_o1", False),
             slice=f.get("slice", False), split1=pair == "split1", split2=pair == "split2", y=None, lens=None, g2=None, b2=None)
    x = rnd(B * T, C) + f.get("mean", 0.0)
    y = rnd(B * T, C)
    c["g1"], c["b1"] = put(1 + 0.3 * rnd(C)), put(0.2 * rnd(C))
    if (f.get("ln2") or pair == "split2") and c["want_ln"]:
        c["g2"], c["b2"] = put(1 + 0.3 * rnd(C)), put(0.2 * rnd(C))
    if f.get("lens"):
        c["lens"] = torch.tensor(ln_lens(B, T), dtype=torch.int32, device=device)
        beyond = rows_beyond(B * T, c["lens"].cpu(), T, "cpu")
        if nan and "y" in f.get("nan", ""):
            y = torch.where(beyond, torch.full_like(y, float("nan")), y)
        if nan and "x" in f.get("nan", ""):
            x = torch.where(beyond, torch.full_like(x, float("nan")), x)
    c["x"] = put(x)
    if f.get("y"):
        c["y"] = put(y)
    return c


def ln_reference(c: dict) -> dict:
    return add_layernorm_rounded(c["x"], c["y"], c["alpha"], c["g1"], c["b1"], c["odt"], lens=c["lens"], T=c["T"], mask_y=c["mask_y"],
                                 silu_=c["silu"], zero_rows=c["zero_rows"], g2=c["g2"], b2=c["b2"])


def ln_forms_of(pair: str):
    return [k for k, f in LN_FORMS.items() if not (f.get("slice") and pair in ("split1", "split2"))]


CONV_KS = [3, 4, 7, 15, 31]
CONV_TOUT = [1, 15, 16, 17, 33]
CONV_CS = [2, 130, 512, 514, 1024]
CONV_LENS = ["T", 1, 16, 17]
CONV_TIN = ["same", "causal", "one"]


def conv_cases():
    """The forward cases (ACT 0 / 1 / 2): every T_out, C, left_pad, T_in variant, lens value and bias setting with every K, and
    every (dtype, ACT) with every C.  -> list of dicts."""
    cases = []
    for ki, K in enumerate(CONV_KS):
        for i in range(6):
            cases.append(dict(K=K, T_out=CONV_TOUT[i % 5], C=CONV_CS[(i + ki) % 5], pad=[0, (K - 1) // 2, K - 1][i % 3],
                              tin=CONV_TIN[i % 3] if i < 5 else "same", lens=(CONV_LENS + [None, None])[(i + ki) % 6] if i < 5 else
                              CONV_LENS[(ki + 3) % 4], bias=(i + ki) % 2 == 0, act=(i + ki) % 3, dtype=[F32, BF16][i % 2],
                              wide=i % 4 != 3))
    # lens values a rotation above missed for some K, and bias on / off with every K
    for ki, K in enumerate(CONV_KS):
        seen = {c["lens"] for c in cases if c["K"] == K}
        for j, L in enumerate(v for v in CONV_LENS if v not in seen):
            cases.append(dict(K=K, T_out=33, C=130, pad=(K - 1) // 2, tin="same", lens=L, bias=j % 2 == 1, act=j % 3,
                              dtype=[BF16, F32][j % 2], wide=True))
    for ai, act in enumerate((0, 1, 2)):
        for di, dt in enumerate((F32, BF16)):
            for ci, C in enumerate(CONV_CS):
                K = CONV_KS[(ai + di + ci) % 5]
                cases.append(dict(K=K, T_out=17, C=C, pad=(K - 1) // 2, tin="same", lens=16 if ci % 2 else None, bias=True, act=act,
                                  dtype=dt, wide=True))
    return cases


def make_conv_case(K, T_out, C, pad, tin, lens, bias, act, dtype, wide, B=2, seed=0, device="cpu", nan=True, shift=0.0) -> dict:
    """Seeded operands of one forward call.  wide: x is a column slice (8 columns in) of a buffer 16 columns wider, the other
    columns NaN; the frames beyond lens are NaN as well."""
    T_in = {"same": T_out, "causal": T_out + K - 1, "one": 1}[tin]
    Cx = 2 * C if act == 1 else C
    g = torch.Generator().manual_seed(7919 * K + 131 * T_out + C + 17 * act + seed)
    rnd = lambda *s: torch.randn(s, generator=g)
    x = rnd(B, T_in, Cx)
    L = None
    if lens is not None:
        L = torch.tensor([T_in if lens == "T" else lens, max(1, T_in - 1)][:B], dtype=torch.int32)
        if nan:
            beyond = torch.arange(T_in)[None, :] >= L[:, None]
            x = torch.where(beyond.unsqueeze(-1), torch.full_like(x, float("nan")), x)
        L = L.to(device)
    buf = torch.full((B, T_in, Cx + 16), float("nan") if nan else 0.0) if wide else x
    if wide:
        buf[..., 8:8 + Cx] = x
    buf = buf.to(dtype).to(device)
    return dict(K=K, T_out=T_out, T_in=T_in, C=C, pad=pad, act=act, dtype=dtype, lens=L, B=B,
                x=buf[..., 8:8 + Cx] if wide else buf, w=(0.2 * rnd(C, 1, K)).to(dtype).to(device),
                bias=(0.1 * rnd(C) + shift).to(dtype).to(device) if bias else None)


def conv_reference(c: dict, **kw) -> dict:
    return dwconv_rounded(c["x"], c["w"], c["bias"], c["pad"], c["T_out"], act=c["act"], lens=c["lens"], **kw)


def act3_cases():
    """ACT 3: C = 512, K in {15, 31}, every T, same-padded with lens and causal, bias shift 0 and 40, x contiguous and a slice."""
    cases = []
    for K in (15, 31):
        for i, T in enumerate(CONV_TOUT):
            for causal in (False, True):
                cases.append(dict(K=K, T_out=T, C=512, pad=0 if causal else (K - 1) // 2, tin="causal" if causal else "same",
                                  lens=None if causal else [16, "T", 1, 17, 16][i], bias=True, act=3, dtype=BF16,
                                  wide=(i + causal) % 2 == 0, shift=40.0 if (i + causal + K) % 2 else 0.0))
    return cases


def make_act3_case(spec, device="cpu", nan=True) -> dict:
    c = make_conv_case(**spec, device=device, nan=nan)
    g = torch.Generator().manual_seed(spec["K"] + spec["T_out"])
    c["gamma"] = (1 + 0.3 * torch.randn(512, generator=g)).to(BF16).to(device)
    c["beta"] = (0.2 * torch.randn(512, generator=g)).to(BF16).to(device)
    return c


WGRAD_BT = [(1, 1), (1, 127), (1, 128), (1, 129), (3, 257)]      # the edges of the 128-frame span of a block
WGRAD_CS = [2, 130, 514]


def wgrad_cases():
    cases = []
    for ki, K in enumerate(CONV_KS):
        for i, (B, T) in enumerate(WGRAD_BT):
            cases.append(dict(K=K, B=B, T_out=T, C=WGRAD_CS[(i + ki) % 3], causal=(i + ki) % 2 == 0, dtype=[F32, BF16][(i + ki // 2) % 2],
                              wide=i % 2 == 0, want_bias=(i + ki) % 3 != 0))
    for di, dt in enumerate((F32, BF16)):       # every C and both paddings in both dtypes
        for ci, C in enumerate(WGRAD_CS):
            for causal in (False, True):
                cases.append(dict(K=CONV_KS[(ci + di + causal) % 5], B=3, T_out=257, C=C, causal=causal, dtype=dt, wide=not causal,
                                  want_bias=True))
    return cases


def make_wgrad_case(K, B, T_out, C, causal, dtype, wide, want_bias, device="cpu") -> dict:
    T_in, pad = (T_out + K - 1, 0) if causal else (T_out, (K - 1) // 2)
    g = torch.Generator().manual_seed(31 * K + T_out + C)
    x = torch.randn(B, T_in, C, generator=g)
    if wide:
        buf = torch.full((B, T_in, C + 16), float("nan"))
        buf[..., 8:8 + C] = x
        x = buf.to(dtype).to(device)[..., 8:8 + C]
    else:
        x = x.to(dtype).to(device)
    return dict(K=K, pad=pad, x=x, dy=torch.randn(B, T_out, C, generator=g).to(dtype).to(device), want_bias=want_bias)
