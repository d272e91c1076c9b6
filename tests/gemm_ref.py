"""float64 reference of the fused-epilogue GEMMs (csrc/gemm_ph.hip, csrc/gemm_bf16.hip, csrc/gemm_f32.hip) and of the
weight-gradient GEMM (csrc/gemm_tn.hip), and a derived per-element error bound.  Plain torch, CPU or GPU, no kernels of
this package.

`ideal(form, operands)` is the float64 value of what a kernel is specified to compute from the operands AS IT RECEIVES
THEM (the bf16 values, the planes of a split operand), so it depends on torch alone:

    P    = A W^T                                   plain bf16 operands: the float64 product of the bf16 values
         = hi W0^T + lo W1^T + hi W2^T             split operands: A = [hi | lo], W = [W0 | W1 | W2] = [hi_w | hi_w | lo_w]
    pre  = alpha P + bias
    out  = act(pre) + residual                     the activation BEFORE the residual
         = act(pre + residual)                     operands["act_after_residual"]: csrc/gemm_f32.hip (pafc_gemm_f32)
    GLU:   out[t h + c] = pre[2h t + c] * sigmoid(pre[2h t + h + c]),  h = 32 (operands["glu_half"])

`bound(form, operands)` is what a correct kernel may differ from `ideal` by, per element.  With u = 2^-24:

    S    = |alpha| (|A| |W|^T) + |bias| + |residual|      over the operands the kernel multiplies (three plane products)
    E    = L (Kw + 8) u S       fp32 accumulation of the Kw columns the K loop walks, in any order, plus up to eight fp32
                                roundings in the epilogue (the alpha / bias fma, the activation's own steps, the residual
                                add); L = the activation's Lipschitz constant (1; SiLU: 1.1 >= sup |silu'| = 1.0998).
                                GLU: E = E_a + (|a| + E_a) E_b / 4   (|d/da| = sigmoid <= 1, |d/db| = |a| sigmoid' <= |a| / 4)
    out  = u_out (|ideal| + E)  the ONE rounding to the output type, relative to the value that is rounded:
                                fp32 2^-24; planes hi + lo 2^-16 (lo = bf16(x - hi) leaves 2^-8 of 2^-8); bf16 2^-8.
    act  = activation_term()    SiLU / tanh / GLU: 4 x the worst error of the same formula in float32 torch against
                                float64 over the case's own pre-activation values (4 x: fast exponentials and reciprocals).
                                A measured number of torch's, not of the kernel; tests write it to the parity log.
    bound = E + out + act

With operands["act_after_residual"] E is the same L c (S + |residual|) and the activation term is measured over pre + residual.

The accumulation constant c (E = L c S, c = (Kw + 8) u above) counts the roundings on the longest path to one output element:
    bf16 operands     (Kw + 8) u       a product of two bf16 values is an fp32 number: one rounding per column added
    fp32 operands     (2 Kw + 8) u     operands["f32_operands"]: the product of two fp32 values rounds before it is added
    operands["roundings"] = n          c = n u, counted by whoever builds the operands: tn_problem() below does, for the
                                       weight-gradient GEMM (csrc/gemm_tn.hip), whose walk is not one K loop

The bf16 term is 2^-8 |x|, not 2^-9 |x|: half a bf16 step is 2^(e - 8) for |x| in [2^e, 2^(e + 1)), which is 2^-8 |x| at the
bottom of the binade (x = 1 + 2^-8 rounds to 1 or 1 + 2^-7, either way 2^-8 off).  tests/test_gemm_ref.py shows that a
correctly rounded `ideal` breaks a 2^-9 term on a quarter of the elements, and that 2^-8 still tells a second rounding, a
dropped plane product and a bias scaled by alpha from a correct kernel."""
from collections import namedtuple

import torch

# a_split: A / W are planes of fp32 operands; out: "bf16" | "f32" | "planes"; act: "none" | "silu" | "tanh" | "relu" | "glu";
# res: None | "bf16" | "f32" (the residual's type)
Form = namedtuple("Form", "a_split out act res")

U32 = 2.0 ** -24
_U_OUT = {"f32": 2.0 ** -24, "planes": 2.0 ** -16, "bf16": 2.0 ** -8}
_LIP = {"none": 1.0, "relu": 1.0, "tanh": 1.0, "silu": 1.1, "glu": 1.0}

# every instantiation pafc_gemm_ph_ex2 can launch.  (The CONV ones have their own entry points and their own battery on this
# reference: tests/conv_ref.py, tests/test_conv_sub_f64_gpu.py; the folded-LayerNorm ones have their own entry points too.)
SHARED_FRAGMENT_FORMS = {
    "split-f32": Form(True, "f32", "none", None),
    "split-f32-res": Form(True, "f32", "none", "f32"),
    "split-f32-res-inplace": Form(True, "f32", "none", "f32"),
    "split-f32-glu": Form(True, "f32", "glu", None),
    "split-planes": Form(True, "planes", "none", None),
    "split-planes-silu": Form(True, "planes", "silu", None),
}
HI_LO_HI_FORMS = {
    "split-bf16": Form(True, "bf16", "none", None),
    "split-bf16-silu": Form(True, "bf16", "silu", None),
    "split-bf16-res": Form(True, "bf16", "none", "bf16"),
    "split-bf16-glu": Form(True, "bf16", "glu", None),
}
PLAIN_FORMS = {
    "bf16": Form(False, "bf16", "none", None),
    "bf16-silu": Form(False, "bf16", "silu", None),
    "bf16-tanh": Form(False, "bf16", "tanh", None),
    "bf16-relu": Form(False, "bf16", "relu", None),
    "bf16-glu": Form(False, "bf16", "glu", None),
    "bf16-res": Form(False, "bf16", "none", "bf16"),
    "f32": Form(False, "f32", "none", None),
    "f32-glu": Form(False, "f32", "glu", None),
    "f32-res": Form(False, "f32", "none", "f32"),
    "planes": Form(False, "planes", "none", None),
    "planes-silu": Form(False, "planes", "silu", None),
}
FORMS = {**SHARED_FRAGMENT_FORMS, **HI_LO_HI_FORMS, **PLAIN_FORMS}

# what the small tiles of csrc/gemm_bf16.hip take beyond that (pafc_gemm_bf16_f32out_pb: every activation with an fp32 or a
# planes output, an fp32 residual behind an activation; pafc_gemm_bf16: a bf16 residual behind an activation, GLU over
# blocks of 64 -- operands["glu_half"] = GLU64_HALF)
GLU64_HALF = 64
SMALL_TILE_FORMS = {
    "f32-res-inplace": Form(False, "f32", "none", "f32"),
    "f32-silu": Form(False, "f32", "silu", None),
    "f32-tanh": Form(False, "f32", "tanh", None),
    "f32-relu": Form(False, "f32", "relu", None),
    "f32-silu-res": Form(False, "f32", "silu", "f32"),
    "split-f32-silu": Form(True, "f32", "silu", None),
    "split-f32-tanh": Form(True, "f32", "tanh", None),
    "split-f32-relu": Form(True, "f32", "relu", None),
    "split-f32-silu-res": Form(True, "f32", "silu", "f32"),
    "bf16-silu-res": Form(False, "bf16", "silu", "bf16"),
    "bf16-tanh-res": Form(False, "bf16", "tanh", "bf16"),
    "bf16-relu-res": Form(False, "bf16", "relu", "bf16"),
    "bf16-glu64": Form(False, "bf16", "glu", None),
}


def split_hi_lo(x: torch.Tensor):
    """fp32 x -> bf16 (hi, lo) with hi = bf16(x), lo = bf16(x - hi): x = hi + lo to 2^-16 relative."""
    hi = x.float().bfloat16()
    lo = (x.float() - hi.float()).bfloat16()
    return hi, lo


def split_a(x: torch.Tensor, plane_block: int = 0) -> torch.Tensor:
    """fp32 (..., K) -> the split A operand (..., 2K): [hi K | lo K], or blocks [hi PB | lo PB] ... of plane_block columns."""
    hi, lo = split_hi_lo(x)
    if not plane_block:
        return torch.cat([hi, lo], dim=-1)
    K = x.shape[-1]
    sh = x.shape[:-1] + (K // plane_block, plane_block)
    return torch.cat([hi.reshape(sh), lo.reshape(sh)], dim=-1).reshape(x.shape[:-1] + (2 * K,))


def split_w(w: torch.Tensor) -> torch.Tensor:
    """fp32 (..., K) -> the split weight (..., 3K) = [hi | hi | lo]."""
    hi, lo = split_hi_lo(w)
    return torch.cat([hi, hi, lo], dim=-1)


def glu_interleave(t: torch.Tensor, half: int = 32, dim: int = 0) -> torch.Tensor:
    """Rows [values C | gates C] along `dim` -> blocks of `half` value rows followed by the `half` gate rows of the same
    channels (the row order the kernels want for act "glu")."""
    t = t.movedim(dim, 0)
    C = t.shape[0] // 2
    v = t[:C].reshape(C // half, half, *t.shape[1:])
    g = t[C:].reshape(C // half, half, *t.shape[1:])
    return torch.cat([v, g], dim=1).reshape(t.shape).movedim(0, dim).contiguous()


def planes_value(out: torch.Tensor, n: int, lo_off: int = None) -> torch.Tensor:
    """A planes output (..., >= lo_off + n) bf16 read back as the float64 value hi + lo."""
    lo_off = n if lo_off is None else lo_off
    return out[..., :n].double() + out[..., lo_off:lo_off + n].double()


def _planes_of(form: Form, ops: dict):
    """[(A plane, W plane)] the kernel multiplies, as float64, and Kw."""
    A, W = ops["A"].double(), ops["W"].double()
    if not form.a_split:
        return [(A, W)], A.shape[-1]
    K = W.shape[-1] // 3
    pb = ops.get("plane_block", 0) or K
    blocks = A.reshape(A.shape[:-1] + (K // pb, 2, pb))
    hi = blocks[..., 0, :].reshape(A.shape[:-1] + (K,))
    lo = blocks[..., 1, :].reshape(A.shape[:-1] + (K,))
    return [(hi, W[..., :K]), (lo, W[..., K:2 * K]), (hi, W[..., 2 * K:])], 3 * K


def products(form: Form, ops: dict):
    """(P, |A| |W|^T, Kw) in float64; kept in `ops` so that ideal(), bound() and the forms that share operands form them once."""
    if "_prod" not in ops:
        pairs, Kw = _planes_of(form, ops)
        P = sum(a @ w.transpose(-1, -2) for a, w in pairs)
        Sp = sum(a.abs() @ w.abs().transpose(-1, -2) for a, w in pairs)
        ops["_prod"] = (P, Sp, Kw)
    return ops["_prod"]


def rows(ops: dict, M: int) -> dict:
    """The problem of the first M rows: A, the residual and the products sliced, everything else shared."""
    out = dict(ops)
    out["A"] = ops["A"][..., :M, :]
    if ops.get("residual") is not None:
        out["residual"] = ops["residual"][..., :M, :]
    if "_prod" in ops:
        P, Sp, Kw = ops["_prod"]
        out["_prod"] = (P[..., :M, :], Sp[..., :M, :], Kw)
    return out


def _row_vec(t):
    return 0.0 if t is None else t.double().unsqueeze(-2)


def _glu_parts(x: torch.Tensor, half: int):
    b = x.reshape(x.shape[:-1] + (x.shape[-1] // (2 * half), 2, half))
    sh = x.shape[:-1] + (x.shape[-1] // 2,)
    return b[..., 0, :].reshape(sh), b[..., 1, :].reshape(sh)


def _act(form: Form, pre: torch.Tensor, half: int) -> torch.Tensor:
    if form.act == "glu":
        a, b = _glu_parts(pre, half)
        return a * torch.sigmoid(b)
    if form.act == "silu":
        return pre * torch.sigmoid(pre)
    if form.act == "tanh":
        return torch.tanh(pre)
    if form.act == "relu":
        return torch.relu(pre)
    return pre


def pre_activation(form: Form, ops: dict) -> torch.Tensor:
    """What the activation is applied to: alpha P + bias, and the residual too with operands["act_after_residual"]."""
    P, _, _ = products(form, ops)
    pre = float(ops.get("alpha", 1.0)) * P + _row_vec(ops.get("bias"))
    if ops.get("act_after_residual") and ops.get("residual") is not None:
        pre = pre + ops["residual"].double()
    return pre


def ideal(form: Form, ops: dict) -> torch.Tensor:
    out = _act(form, pre_activation(form, ops), ops.get("glu_half", 32))
    if ops.get("residual") is not None and not ops.get("act_after_residual"):
        out = out + ops["residual"].double()
    return out


def accumulation_constant(ops: dict, Kw: int) -> float:
    """c of the module docstring: the roundings on the longest path to one element, times u."""
    if ops.get("roundings") is not None:
        return float(ops["roundings"]) * U32
    return ((2 if ops.get("f32_operands") else 1) * Kw + 8) * U32


def activation_term(form: Form, ops: dict) -> float:
    """4 x the worst |float32 formula - float64 formula| over this case's pre-activation values (0 for none / ReLU)."""
    if form.act not in ("silu", "tanh", "glu"):
        return 0.0
    pre = pre_activation(form, ops).cpu()          # measured with the CPU's float32 kernels, wherever the operands live
    half = ops.get("glu_half", 32)
    return 4.0 * float((_act(form, pre.float(), half).double() - _act(form, pre, half)).abs().max())


def bound(form: Form, ops: dict, act_term: float = None) -> torch.Tensor:
    _, Sp, Kw = products(form, ops)
    S = abs(float(ops.get("alpha", 1.0))) * Sp
    if ops.get("bias") is not None:
        S = S + _row_vec(ops["bias"]).abs()
    res = ops["residual"].double().abs() if ops.get("residual") is not None else 0.0
    c = accumulation_constant(ops, Kw)
    if form.act == "glu":
        half = ops.get("glu_half", 32)
        Ea, Eb = _glu_parts(c * S, half)
        a, _ = _glu_parts(pre_activation(form, ops), half)
        E = Ea + (a.abs() + Ea) * Eb / 4
    else:
        E = _LIP[form.act] * c * (S + res)
    if act_term is None:
        act_term = activation_term(form, ops)
    return E + _U_OUT[form.out] * (ideal(form, ops).abs() + E) + act_term


def round_to(form: Form, x: torch.Tensor) -> torch.Tensor:
    """float64 x rounded once to the form's output type, read back as float64 (planes: hi + lo)."""
    x32 = x.float()
    if form.out == "f32":
        return x32.double()
    if form.out == "bf16":
        return x32.bfloat16().double()
    hi, lo = split_hi_lo(x32)
    return hi.double() + lo.double()


def make_operands(form: Form, M: int, N: int, K: int, seed: int, batch: int = 0, alpha: float = 1.0, plane_block: int = 0,
                  shared_bias: bool = False, device="cpu", f32_operands: bool = False) -> dict:
    """Seeded operands as the kernel receives them: randn A, W scaled by K^-0.5, bias by 0.3, residual by 1; bias and
    residual in the types the form takes.  batch > 0 adds a leading batch dimension.  GLU: N counts the weight rows.
    f32_operands (plain forms): A and W stay fp32, and the bound counts a rounding per product."""
    assert not (f32_operands and form.a_split)
    g = torch.Generator().manual_seed(seed)
    lead = (batch,) if batch else ()
    rnd = lambda *s: torch.randn(lead + s, generator=g)
    a, w = rnd(M, K), rnd(N, K) * K ** -0.5
    b = (torch.randn((N,), generator=g) if shared_bias else rnd(N)) * 0.3
    No = N // 2 if form.act == "glu" else N
    r = rnd(M, No)
    ops = {"alpha": alpha, "plane_block": plane_block, "f32_operands": f32_operands}
    ops["A"] = split_a(a, plane_block) if form.a_split else (a if f32_operands else a.bfloat16())
    ops["W"] = split_w(w) if form.a_split else (w if f32_operands else w.bfloat16())
    ops["bias"] = b.bfloat16() if form.out == "bf16" else b
    ops["residual"] = None if form.res is None else (r.bfloat16() if form.res == "bf16" else r)
    ops["a32"], ops["w32"] = a, w                # the fp32 operands the planes were split from
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}


def make_grid_operands(form: Form, M: int, N: int, K: int, seed: int, plane_block: int = 0, alpha: float = 1.0,
                       glu_half: int = 32, device="cpu", f32_operands: bool = False, batch: int = 0,
                       shared_bias: bool = False) -> dict:
    """Operands on a grid, for which fp32 accumulation is EXACT in any order and in any number of K shares: the hi plane of
    A (or a plain A) and the weights are integers in [-3, 3]; the lo plane of A, lo_w, the bias and the residual are integers
    times 2^-6 (in [-3, 3] 2^-6 and [-31, 31] 2^-6).  A kernel multiplies the planes it is given: they need not be the
    hi / lo split of anything.  With alpha 1 or 0.5 every product, every partial sum and every step of the epilogue before
    the activation is then a multiple of 2^-7 below 2^17 -- an fp32 number -- as the precondition asserted here says:

        max(|A| |W|^T + |bias| + |residual|) 2^7 < 2^24

    so `round_to(form, ideal(form, ops))` is what a correct kernel gives BIT FOR BIT for act "none", and a K-step that is
    dropped, walked twice or taken from the wrong plane changes nearly every element (tests/test_gemm_ref.py).
    f32_operands: the same integers as fp32 A and W (plain forms).  batch > 0 adds a leading batch dimension (the bias per
    entry, or one for all with shared_bias)."""
    assert alpha in (1.0, 0.5), alpha
    assert not (f32_operands and form.a_split)
    g = torch.Generator().manual_seed(seed)
    lead = (batch,) if batch else ()
    ints = lambda lim, *s: torch.randint(-lim, lim + 1, lead + s, generator=g).float()
    No = N // 2 if form.act == "glu" else N
    ops = {"alpha": alpha, "plane_block": plane_block, "glu_half": glu_half, "f32_operands": f32_operands}
    if form.a_split:
        hi, lo = ints(3, M, K), ints(3, M, K) * 2.0 ** -6
        if plane_block:
            sh = lead + (M, K // plane_block, plane_block)
            A = torch.cat([hi.reshape(sh), lo.reshape(sh)], dim=-1).reshape(lead + (M, 2 * K))
        else:
            A = torch.cat([hi, lo], dim=-1)
        hi_w = ints(3, N, K)
        W = torch.cat([hi_w, hi_w, ints(3, N, K) * 2.0 ** -6], dim=-1)
    else:
        A, W = ints(3, M, K), ints(3, N, K)
    b = (torch.randint(-31, 32, (N,), generator=g).float() if shared_bias else ints(31, N)) * 2.0 ** -6
    r = ints(31, M, No) * 2.0 ** -6
    ops["A"], ops["W"] = (A, W) if f32_operands else (A.bfloat16(), W.bfloat16())
    assert torch.equal(ops["A"].float(), A) and torch.equal(ops["W"].float(), W)
    ops["bias"] = b.bfloat16() if form.out == "bf16" else b
    ops["residual"] = None if form.res is None else (r.bfloat16() if form.res == "bf16" else r)
    ops = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}
    assert grid_bits(form, ops) < 24.0, (form, M, N, K, grid_bits(form, ops))
    return ops


def grid_bits(form: Form, ops: dict) -> float:
    """log2 of max(|A| |W|^T + |bias| + |residual|) 2^7: the significand bits the grid operands' sums need (< 24: exact)."""
    import math
    _, Sp, _ = products(form, ops)
    S = Sp if ops.get("bias") is None else Sp + _row_vec(ops["bias"]).abs()
    if ops.get("residual") is not None and form.act != "glu":
        S = S + ops["residual"].double().abs()
    return math.log2(float(S.max()) * 2.0 ** 7)


# ---- the transposed product of the training step: dW = dY^T X, dbias = column sums of dY (csrc/gemm_tn.hip) ---------------
def make_tn_operands(R: int, M: int, N: int, seed: int, batch: int = 0, grid: bool = False, device="cpu"):
    """(dy (.., R, M), x (.., R, N)) bf16: randn, or integers in [-3, 3] (`grid`: every sum is an fp32 number far beyond the R
    of the tests -- 9 R < 2^24 -- in any order, in any number of splits)."""
    g = torch.Generator().manual_seed(seed)
    lead = (batch,) if batch else ()
    if grid:
        dy, x = (torch.randint(-3, 4, lead + (R, n), generator=g).float() for n in (M, N))
    else:
        dy, x = (torch.randn(lead + (R, n), generator=g) for n in (M, N))
    return dy.bfloat16().to(device), x.bfloat16().to(device)


def tn_plan(R: int, s: int):
    """The documented plan arithmetic for a split count s: rows per split in whole 64-row K-steps, and the S that leaves no
    split empty.  -> (S, rows per split)"""
    rps = -(-(-(-R // s)) // 64) * 64
    return -(-R // rps), rps


def tn_problem(dy: torch.Tensor, x: torch.Tensor, out: str, S: int, rps: int):
    """dW = dY^T X as the plain form Form(False, out, "none", None) with A = dY^T, W = X^T, Kw = R, and the bias gradient as
    the same form against a column of ones.  -> (form, operands of dW, operands of dbias (.., M, 1))

    roundings = min(rps, R) + 1 + S + 1, the sum over the longest path to one element of dW:
        min(rps, R)   a K group of a block adds the rows of its split in fp32, one rounding per row -- the products of two
                      bf16 values are exact (each group walks half of the rows of every K-step; the count stays with the
                      whole split, an upper bound)
        + 1           where the two K groups' sums meet, in the block's epilogue
        + S           the reducing kernel adds the S partials (the quarter sums and their two final additions included)
        + 1           the fp32 value the output is written from (the `out` term of bound() then rounds it to the output type)."""
    form = Form(False, out, "none", None)
    R = dy.shape[-2]
    n = min(rps, R) + 1 + S + 1
    A = dy.transpose(-1, -2)
    dw = {"A": A, "W": x.transpose(-1, -2), "bias": None, "residual": None, "alpha": 1.0, "roundings": n}
    ones = torch.ones((1, R), dtype=dy.dtype, device=dy.device)
    db = {"A": A, "W": ones, "bias": None, "residual": None, "alpha": 1.0, "roundings": n}
    return form, dw, db
