"""float64 reference of the time-mix front end (src/model.py:273-289; csrc/glue.hip: tmix_lora_down_kernel, tmix_lora_mix4_kernel,
tmix_lora_mix4_ws_kernel, decay_lora_kernel) and a derived per-element bound.  Plain torch, CPU or GPU, no kernels of this package.

From the bf16 operands AS A KERNEL RECEIVES THEM, per direction d (0 looks back, or forward with reverse0; 1 always looks forward):

    xx   = nb(x) - x                      nb = x_{t-1}, or x_{t+1} for a forward-looking direction; zero beyond a sequence end;
                                          `prev` (B, C) replaces that zero for the backward-looking direction ONLY
    xxx  = x + xx * maa_x
    t    = tanh(xxx W1)                   W1 = w1n^T, 128 LoRA columns = 4 maps x 32
    m_q  = t[:, 32q:32q+32] W2_q          q in {r, k, v, w}
    z_q  = x + xx * (maa_q + m_q)
    td   = tanh(z_w D1)
    w    = td D2 (+ time_decay)

`chain_exact` evaluates this in float64 without any intermediate rounding (the yardstick of a chained test).  `chain_rounded`
evaluates every op exactly in float64 and rounds to bf16 (nearest, ties to even: `rb`) wherever the module chain stores a bf16
tensor, which is where the kernels document a rounding too:

    xx, xx * maa_x, xxx | t | m_q, maa_q + m_q, xx * (.), z_q | td | w = rb(td D2), then rb(time_decay + w)

It is the specification of ONE kernel given its inputs: `t=` / `zw=` replace the chain's own t / z_w by the tensor a kernel was
actually given, and `stages` restricts the work to the stretch a kernel covers ("down": xx, xxx, t; "up": m, z; "decay": td, w).
Layouts are the kernels': xxx (ndir, rows, C), t (ndir, rows, 128), m (ndir, 4, rows, C), z (4, ndir, rows, C), td (ndir, rows, 64),
w (ndir, rows, C), rows = B T.

`bound(stage, ops, chain)` is the distance a correct kernel may have from `chain_rounded`, per element.  A correct kernel forms the
element-wise ops exactly as above (a sum, difference or product of two bf16 values is exact in fp32, or decided far away from
any bf16 midpoint) and its products with fp32 accumulation.  So before each rounding it holds the exact value a up to

    E    = (K + 8) u S       u = 2^-24, S = |A| |W|^T: fp32 accumulation over K in any order plus up to eight fp32 roundings in
                             the epilogue (as gemm_ref.bound; tanh has Lipschitz constant 1)
    act  = activation_term   tanh: 4 x the worst error of float32 torch's tanh against float64 over the case's own
                             pre-activations (as gemm_ref.activation_term: a number of torch's, not of the kernel)

and then rounds once.  Rounding is monotone, so the kernel's bf16 value lies in [rb(a - E - act), rb(a + E + act)]: that interval
IS the "one output rounding" term, 2^-8 (|ideal| + E) against the unrounded value, written against a reference that is itself
rounded.  It is never wider than one bf16 step beyond E, and it is zero wherever a - E .. a + E contains no bf16 midpoint:
such elements must be bit-identical.  Per stage:

    xxx          0: element-wise only (tests/test_fused_gpu.py::test_tmix_glue_matches_module_chain asserts bit-identity)
    t, td, m     the interval above with K = C (t, td) or 32 (m)
    z_q          m_q is an intermediate the kernel formed itself and may be one rounding step away from the reference's: its
                 interval is carried through the three exact, monotone ops that follow, rb(maa_q + .), rb(xx * .) (the order of
                 the end points follows the sign of xx: the sensitivity |xx|) and rb(x + .), each of which may turn a part of a
                 step into a whole step of its own grid.  Given m_q exactly the bound is zero.
    w            td likewise: each hidden value may be as far from the reference's as its interval allows (zero where no
                 midpoint is near), which moves td D2 by at most dev(td) |D2|^T (one rounding step of td times the row sums
                 of |D2|); to that the (64 + 8) u S of this product, then the interval of rb(.), then of rb(time_decay + .).

No element is excluded: every output element has to be within its own bound.  tests/test_tmix_ref.py checks on the CPU that the
same chain in float32 stays within it at every stage, and that each of a list of plausible kernel mistakes falls outside."""
import torch

U32 = 2.0 ** -24
N_LORA, N_DECAY = 128, 64
# (B, T) every kernel is run at: 1, 15, 16 and 17 rows (the edges of a 16-row tile), three sequences whose ends fall inside
# tiles, and T = 1 where every row is both first and last
SMALL_SHAPES = [(1, 1), (1, 15), (1, 16), (1, 17), (3, 21), (5, 1)]


def rb(v: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), as float64; no detour through float32.  On the
    bit pattern, so that it is exact on every device: the 45 low mantissa bits are rounded away, a carry goes into the exponent."""
    i = v.contiguous().view(torch.int64)
    i = (i + ((1 << 44) - 1) + ((i >> 45) & 1)) & -(1 << 45)
    return i.view(torch.float64)


def make_operands(B: int, T: int, C: int, ndir: int, seed: int, reverse0: bool = False, prev: bool = False, bias: bool = True,
                  device="cpu") -> dict:
    """Seeded bf16 operands at the scales of the kernel tests: tanh is not saturated (W1 1.5 / sqrt(C), D1 2 / sqrt(C), D2 0.3)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=g)
    ops = {"x": rnd(B, T, C), "maa_x": rnd(ndir, C) * 0.5, "w1n": rnd(ndir, N_LORA, C) * (1.5 / C ** 0.5),
           "w2t": rnd(ndir, 4, C, 32) * 0.2, "maa": rnd(ndir, 4, C) * 0.5, "d1n": rnd(ndir, N_DECAY, C) * (2.0 / C ** 0.5),
           "d2n": rnd(ndir, C, N_DECAY) * 0.3, "time_decay": rnd(ndir, C) - 3, "prev": rnd(B, C)}
    ops = {k: v.bfloat16().to(device) for k, v in ops.items()}
    if not prev:
        ops["prev"] = None
    if not bias:
        ops["time_decay"] = None
    ops["reverse0"] = bool(reverse0)
    return ops


def looks_forward(d: int, reverse0: bool) -> bool:
    return d == 1 or bool(reverse0)


def neighbour(x: torch.Tensor, forward: bool, prev=None) -> torch.Tensor:
    """x (B, T, C) -> x_{t+1} (forward) or x_{t-1}, zero beyond the sequence; prev (B, C) is the frame before a sequence."""
    nb = torch.zeros_like(x)
    if forward:
        nb[:, :-1] = x[:, 1:]
    else:
        nb[:, 1:] = x[:, :-1]
        if prev is not None:
            nb[:, 0] = prev.to(x.dtype).view(x.shape[0], x.shape[2])
    return nb


def _chain(ops: dict, r, t=None, zw=None, stages=("down", "up", "decay")) -> dict:
    x = ops["x"].double()
    B, T, C = x.shape
    rows, nd = B * T, ops["maa_x"].shape[0]
    xf = x.reshape(rows, C)
    out, aux = {}, {}
    put = lambda d_, k, v: d_.setdefault(k, []).append(v)
    for d in range(nd):
        xx = r(neighbour(x, looks_forward(d, ops["reverse0"]), ops["prev"]) - x).reshape(rows, C)
        if "down" in stages:
            xxx = r(xf + r(xx * ops["maa_x"][d].double()))
            w1 = ops["w1n"][d].double()
            pre = xxx @ w1.T
            put(out, "xxx", xxx)
            put(out, "t", r(torch.tanh(pre)))
            put(aux, "pre_t", pre)
            put(aux, "S_t", xxx.abs() @ w1.abs().T)
        if "up" in stages:
            td_ = (out["t"][d] if t is None else t[d].double()).reshape(rows, 4, 32).transpose(0, 1)     # (4, rows, 32)
            w2 = ops["w2t"][d].double().transpose(1, 2)                                                  # (4, 32, C)
            m_exact = torch.bmm(td_, w2)
            m = r(m_exact)
            z = r(xf + r(xx * r(ops["maa"][d].double().view(4, 1, C) + m)))
            put(out, "m", m)
            put(out, "z", z)
            put(aux, "m_exact", m_exact)
            put(aux, "S_m", torch.bmm(td_.abs(), w2.abs()))
            put(aux, "xx", xx)
        if "decay" in stages:
            z_w = out["z"][d][3] if zw is None else zw[d].double().reshape(rows, C)
            d1, d2 = ops["d1n"][d].double(), ops["d2n"][d].double()
            pre = z_w @ d1.T
            td = r(torch.tanh(pre))
            w_exact = td @ d2.T
            w = r(w_exact)
            if ops["time_decay"] is not None:
                w = r(ops["time_decay"][d].double() + w)
            put(out, "td", td)
            put(out, "w", w)
            put(aux, "pre_td", pre)
            put(aux, "S_td", z_w.abs() @ d1.abs().T)
            put(aux, "w_exact", w_exact)
    out = {k: torch.stack(v) for k, v in out.items()}
    if "z" in out:
        out["z"] = out["z"].transpose(0, 1).contiguous()           # (4, ndir, rows, C), as the kernels store it
    out["_aux"] = {k: torch.stack(v) for k, v in aux.items()}
    return out


def chain_rounded(ops: dict, t=None, zw=None, stages=("down", "up", "decay")) -> dict:
    """Every stage in float64, rounded to bf16 where the module chain stores a bf16 tensor.  t (ndir, rows, 128) / zw (ndir, rows,
    C): what the up-projection / the decay LoRA was given, in place of the chain's own."""
    return _chain(ops, rb, t, zw, stages)


def chain_exact(ops: dict) -> dict:
    """Every stage in float64 with no intermediate rounding."""
    return _chain(ops, lambda v: v)


def activation_term(pre: torch.Tensor) -> float:
    """4 x the worst |tanh in float32 - tanh in float64| over these pre-activations (measured with the CPU's float32 kernels,
    wherever the operands live)."""
    pre = pre.cpu()
    return 4.0 * float((torch.tanh(pre.float()).double() - torch.tanh(pre)).abs().max())


def _interval(a: torch.Tensor, d):
    """The bf16 values a kernel may hold that rounds, once, a value within d of a."""
    return rb(a - d), rb(a + d)


def _dev(ref, lo, hi):
    return torch.maximum(hi - ref, ref - lo)


def bound(stage: str, ops: dict, chain: dict = None) -> torch.Tensor:
    """Per-element distance a correct kernel may have from chain[stage] (see the module docstring); `chain` is what
    chain_rounded returned for the kernel's inputs (default: chain_rounded(ops), every stage fed by the chain itself)."""
    chain = chain_rounded(ops) if chain is None else chain
    aux = chain["_aux"]
    C = ops["x"].shape[-1]
    if stage == "xxx":
        return torch.zeros_like(chain["xxx"])
    if stage in ("t", "td"):
        pre = aux["pre_" + stage]
        lo, hi = _interval(torch.tanh(pre), (C + 8) * U32 * aux["S_" + stage] + activation_term(pre))
        return _dev(chain[stage], lo, hi)
    if stage in ("m", "z"):
        lo, hi = _interval(aux["m_exact"], (32 + 8) * U32 * aux["S_m"])                 # (ndir, 4, rows, C)
        if stage == "m":
            return _dev(chain["m"], lo, hi)
        maa = ops["maa"].double().unsqueeze(2)                                           # (ndir, 4, 1, C)
        xx = aux["xx"].unsqueeze(1)                                                      # (ndir, 1, rows, C)
        x = ops["x"].double().reshape(1, 1, -1, C)
        p0, p1 = rb(xx * rb(maa + lo)), rb(xx * rb(maa + hi))
        lo, hi = rb(x + torch.minimum(p0, p1)), rb(x + torch.maximum(p0, p1))
        return _dev(chain["z"], lo.transpose(0, 1), hi.transpose(0, 1))
    if stage == "w":
        pre = aux["pre_td"]
        tlo, thi = _interval(torch.tanh(pre), (C + 8) * U32 * aux["S_td"] + activation_term(pre))
        d2 = ops["d2n"].double().abs().transpose(1, 2)                                   # (ndir, 64, C)
        E = _dev(chain["td"], tlo, thi) @ d2 + (N_DECAY + 8) * U32 * (torch.maximum(tlo.abs(), thi.abs()) @ d2)
        lo, hi = _interval(aux["w_exact"], E)
        if ops["time_decay"] is not None:
            b = ops["time_decay"].double().unsqueeze(1)
            lo, hi = rb(b + lo), rb(b + hi)
        return _dev(chain["w"], lo, hi)
    raise ValueError(stage)
