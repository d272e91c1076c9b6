"""float64 reference of the forward subsampling convolutions (csrc/conv_sub.hip and the CONV instantiations of
csrc/gemm_ph.hip), and the cases their battery walks.  Plain torch, CPU or GPU, no kernels of this package.

A 3 x 3 stride-2 convolution on NHWC is the GEMM of its im2col matrix, so the reference and the bound are those of
tests/gemm_ref.py, unchanged:

    A = im2col(x)     (B T2 F2, 9 Ci)   row m = output position (b, t2, f2), column (kh, kw, ci) = x[b, 2 t2 + kh, 2 f2 + kw, ci]
    W = w_matrix(w)   (Co, 9 Ci)        from the (9, Co, Ci) tap-major weight the kernels take
    out = act(A W^T + bias)             T2 = (T1 - 3) // 2 + 1, F2 = (F1 - 3) // 2 + 1: with an even T1 (F1) the last input
                                        row (column) belongs to no window

Split operands (an fp32 image and fp32 weights as bf16 planes): for the reference A = [im2col(hi) | im2col(lo)] and
W = [W_hi | W_hi | W_lo] over the whole K = 9 Ci, which gemm_ref multiplies as hi W_hi + lo W_hi + hi W_lo.  (The kernels
receive the same planes per pixel, [hi Ci | lo Ci], and per tap, [hi | hi | lo]: tests/conv_launch.py lays them out.)

    entry point                                  kind       form                                  A and W
    pafc_conv3x3s2_nhwc_bf16 (every tile), _ph   "bf16"     Form(False, "bf16", none | relu)      the bf16 values
    pafc_conv3x3s2_nhwc_f32split                 "split"    Form(True, "f32", none | relu)        the planes
    pafc_conv3x3s2_nhwc_split_ph                 "split"    Form(True, "planes", none | relu)     the planes
    pafc_conv3x3s2_c1_nhwc_bf16                  "c1-bf16"  Form(False, "bf16", none | relu)      K = 9, the bf16 values
    pafc_conv3x3s2_c1_nhwc_f32split(_ps)         "c1-f32"   Form(False, "planes", none | relu)    K = 9, the fp32 values (fp32
                                                                                                  arithmetic, planes out)

The case tables are data (the way of glue_ref.CONV_*): the GPU tests walk them, tests/test_conv_ref.py checks that they meet
the conditions they were written for and that on every case a correctly formed result lies inside the bound while each
planted mistake falls outside it."""
from collections import namedtuple

import torch

from tests import gemm_ref
from tests.gemm_ref import Form

# an image (B, T1, F1, Ci) and Co output channels.  conv1: Ci = 1, (T1, F1) = the feature matrix (T, F), Co = C
Case = namedtuple("Case", "B T1 F1 Ci Co")

FORMS = {   # entry-point family -> (kind, a_split, out)
    "bf16": ("bf16", False, "bf16"),
    "bf16_ph": ("bf16", False, "bf16"),
    "f32split": ("split", True, "f32"),
    "split_ph": ("split", True, "planes"),
    "c1_bf16": ("c1-bf16", False, "bf16"),
    "c1_f32split": ("c1-f32", False, "planes"),
}
VARIANTS = [(1, True), (0, True), (1, False), (0, False)]      # (relu, bias present) -- every entry point takes all four


def form_of(family: str, relu) -> Form:
    _, a_split, out = FORMS[family]
    return Form(a_split, out, "relu" if relu else "none", None)


def out_size(n: int) -> int:
    return (n - 3) // 2 + 1


def rows_of(case: Case) -> int:
    return case.B * out_size(case.T1) * out_size(case.F1)


def im2col(x: torch.Tensor, dt: int = 0, df: int = 0, swap: bool = False) -> torch.Tensor:
    """(B, T1, F1, Ci) -> (B T2 F2, 9 Ci), tap-major (kh, kw) with the channels minor: the order of the (9, Co, Ci) weight.
    dt / df / swap form the WRONG matrices tests/test_conv_ref.py plants (windows one row / one column late -- only where the
    size is even, so that the late window still lies in the image -- and kh, kw exchanged)."""
    B, T1, F1, C = x.shape
    T2, F2 = out_size(T1), out_size(F1)
    taps = []
    for kh in range(3):
        for kw in range(3):
            r, c = ((kw, kh) if swap else (kh, kw))
            taps.append(x[:, r + dt:r + dt + 2 * T2 - 1:2, c + df:c + df + 2 * F2 - 1:2, :])
    return torch.stack(taps, dim=3).reshape(B * T2 * F2, 9 * C)


def w_matrix(taps: torch.Tensor) -> torch.Tensor:
    """(9, Co, Ci) -> (Co, 9 Ci): the weight the im2col matrix multiplies."""
    return taps.permute(1, 0, 2).reshape(taps.shape[1], 9 * taps.shape[2])


def split_a(x_hi, x_lo, **kw) -> torch.Tensor:
    return torch.cat([im2col(x_hi, **kw), im2col(x_lo, **kw)], dim=-1)


def split_w(taps_hi, taps_lo) -> torch.Tensor:
    return torch.cat([w_matrix(taps_hi), w_matrix(taps_hi), w_matrix(taps_lo)], dim=-1)


def seed_of(case: Case) -> int:
    return sum(v * p for v, p in zip(case, (7919, 104729, 1299709, 31, 15485863))) % (2 ** 31 - 1)


def make_problem(kind: str, case: Case, device="cpu", grid: bool = False) -> dict:
    """The operands of one case, seeded by the case, as the kernels receive them (x, taps / their planes, bias) and as
    gemm_ref reads them (A, W, bias): a randn image, weights scaled by K^-0.5 (conv1: 1 / 3), a bias of order 0.3 -- large
    enough for a missing one to exceed the bound (a bias near zero hides it).  `grid`: values from the grid of
    gemm_ref.make_grid_operands (integers in [-3, 3]; lo planes and lo weights integers in [-3, 3] 2^-6; the bias integers in
    [-31, 31] 2^-6; the fp32 conv1: x and w an integer of the first kind plus one of the second), for which fp32
    accumulation is exact in any order: see grid_bits()."""
    B, T1, F1, Ci, Co = case
    g = torch.Generator().manual_seed(seed_of(case) + (1 if grid else 0))
    if grid:
        ints = lambda lim, *s: torch.randint(-lim, lim + 1, s, generator=g).float()
        x, x2 = ints(3, B, T1, F1, Ci), ints(3, B, T1, F1, Ci) * 2.0 ** -6
        w, w2 = ints(3, 9, Co, Ci), ints(3, 9, Co, Ci) * 2.0 ** -6
        b = ints(31, Co) * 2.0 ** -6
    else:
        x = torch.randn((B, T1, F1, Ci), generator=g)
        w = torch.randn((9, Co, Ci), generator=g) * ((9 * Ci) ** -0.5 if Ci > 1 else 1.0 / 3)
        b = torch.randn((Co,), generator=g) * 0.3
    ops = {"case": case, "kind": kind}
    if kind == "bf16":
        ops["x"], ops["taps"], ops["bias"] = x.bfloat16(), w.bfloat16(), b.bfloat16()
        ops["A"], ops["W"] = im2col(ops["x"]), w_matrix(ops["taps"])
    elif kind == "split":
        (xh, xl), (wh, wl) = ((x.bfloat16(), x2.bfloat16()), (w.bfloat16(), w2.bfloat16())) if grid else \
            (gemm_ref.split_hi_lo(x), gemm_ref.split_hi_lo(w))
        ops["x_hi"], ops["x_lo"], ops["taps_hi"], ops["taps_lo"], ops["bias"] = xh, xl, wh, wl, b
        ops["A"], ops["W"] = split_a(xh, xl), split_w(wh, wl)
    else:
        assert Ci == 1, case
        if kind == "c1-f32" and grid:
            x, w = x + x2, w + w2
        cast = (lambda t: t.bfloat16()) if kind == "c1-bf16" else (lambda t: t)
        ops["x"] = cast(x.reshape(B, T1, F1))
        ops["w"] = cast(w.reshape(9, Co).t().contiguous())             # (C, 9), k = 3 kh + kw
        ops["bias"] = cast(b)
        ops["A"], ops["W"] = im2col(ops["x"].unsqueeze(-1)), ops["w"]
    if grid:                                     # the types hold the grid values exactly
        exact = {"x": x, "x_hi": x, "x_lo": x2, "taps": w, "taps_hi": w, "taps_lo": w2, "bias": b}
        assert all(torch.equal(ops[k].float().reshape(-1), v.reshape(-1)) for k, v in exact.items() if k in ops)
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}


def variant(family: str, ops: dict, relu, bias: bool):
    """-> (form, operands) of one (relu, bias) setting: the same A, W and float64 products, the bias kept or dropped."""
    out = dict(ops)
    if not bias:
        out["bias"] = None
    return form_of(family, relu), out


def grid_bits(form: Form, ops: dict) -> float:
    """Significand bits the sums of a grid problem need (< 24: every partial sum, in any order, is an fp32 number, so a
    correct kernel gives round_to(form, ideal) bit for bit).  The planes and weights of the bf16 / split kinds are multiples
    of 2^-6 whose products are multiples of 2^-7 at the coarsest (gemm_ref.grid_bits: K = 9 Ci, or the three plane products);
    the fp32 conv1 multiplies two multiples of 2^-6, so its sums are multiples of 2^-12."""
    import math
    if ops["kind"] != "c1-f32":
        return gemm_ref.grid_bits(form, ops)
    _, Sp, _ = gemm_ref.products(form, ops)
    S = Sp + (0.0 if ops.get("bias") is None else ops["bias"].double().abs().unsqueeze(-2))
    return math.log2(float(S.max()) * 2.0 ** 12)


# ---- the case tables ---------------------------------------------------------------------------------------------------
# Geometries every conv2 family walks: the one-pixel image (M = 1: all rows of a tile but one are beyond M), T1 and F1 both
# even, only T1 even -- with the model's F1 = 39 (F' = 19), three batch entries and M = 285 rows: more than one tile of every
# height, tiles that start in the middle of a frame (19 divides no tile height) and run across batch entries -- only F1 even.
COMMON_GEOMETRIES = [(1, 3, 3), (2, 8, 10), (3, 12, 39), (2, 7, 12)]

# M = B T2 F2 in {tile - 1, tile, tile + 1, 2 tile + 7} per tile height (M = 1 is the one-pixel image).  263 = 2 * 128 + 7
# and 127, 191, 193, 257 are primes: one frame of M positions or M frames of one; 391 = 17 * 23 and 519 = 3 * 173 give the
# multi-tile case B >= 2 and an F2 > 1 that does not divide the tile; for tile 128 the (3, 12, 39) geometry above does.  Some
# of them have an even T1 or F1 as well.
EDGE_GEOMETRIES = {
    128: [(1, 4, 255), (2, 17, 17), (3, 87, 4), (1, 3, 527)],          # M = 127, 128, 129, 263
    192: [(1, 3, 383), (2, 9, 50), (1, 388, 3), (17, 3, 47)],          # M = 191, 192, 193, 391
    256: [(3, 11, 35), (4, 18, 17), (1, 3, 516), (3, 4, 347)],         # M = 255, 256, 257, 519
}
EDGE_ROWS = {t: [t - 1, t, t + 1, 2 * t + 7] for t in EDGE_GEOMETRIES}

# (Ci, Co): the geometries run at the first pair, every pair runs at the 2 tile + 7 geometry.
# csrc/conv_sub.hip (Ci % 64, Co % 128): one, two, three, six and eight 64-channel K-blocks per tap
SUB_CHANNELS = [(192, 256), (64, 128), (128, 384), (384, 128), (512, 256), (64, 384), (128, 128)]
# the phase-pipelined forms (Ci % 128, Co % 8): 2 / 6 / 8 K-steps per tap (split: 6 / 18 / 24, shared fragments 4 / 12 / 16),
# one ragged N tile of 8 columns, a full one followed by 8 columns, 1.5 and 2 tiles
PH_CHANNELS = [(384, 264), (128, 8), (128, 512), (512, 264), (384, 384), (512, 8), (384, 512)]


def conv2_cases(tile: int, channels) -> list:
    geo = COMMON_GEOMETRIES + EDGE_GEOMETRIES[tile]
    cases = [Case(*g, *channels[0]) for g in geo]
    cases += [Case(*EDGE_GEOMETRIES[tile][-1], ci, co) for ci, co in channels[1:]]
    return cases


# family -> {tile height -> cases}.  "bf16" at tile 128: the default tile and PAFC_CONV_TILE = 1 (conv3x3s2_kernel<4, 4, 2, 2>);
# at tile 256: PAFC_CONV_TILE = 2, 3 (256 x 128 blocks) and 4 (256 x 256; Co % 256, else the default tile).
CONV2_CASES = {
    "bf16": {128: conv2_cases(128, SUB_CHANNELS), 256: conv2_cases(256, SUB_CHANNELS)},
    "f32split": {128: conv2_cases(128, SUB_CHANNELS)},
    "bf16_ph": {t: conv2_cases(t, PH_CHANNELS) for t in (128, 192, 256)},
    "split_ph": {t: conv2_cases(t, PH_CHANNELS) for t in (128, 192, 256)},
}
# the exact (grid) case of each: the multi-tile geometry with an even T1 and F1 = 39, Ci != Co
GRID_CASES = {"bf16": Case(3, 12, 39, 192, 256), "f32split": Case(3, 12, 39, 192, 256),
              "bf16_ph": Case(3, 12, 39, 384, 264), "split_ph": Case(3, 12, 39, 384, 264),
              "c1_bf16": Case(3, 7, 23, 1, 64), "c1_f32split": Case(3, 7, 23, 1, 64)}

# the dispatch boundary of pafc_conv3x3s2_nhwc_bf16: Co % 256 == 0 and ceil(M / 256) (Co / 256) >= 512 -> the phase-pipelined
# kernel.  Co = 512: 255 M-tiles stay (M = 3435 * 19 = 65 265), 256 go (M = 3436 * 19 = 65 284 >= 255 * 256 + 1)
DISPATCH_BELOW, DISPATCH_ABOVE = Case(1, 2 * 3435 + 1, 39, 128, 512), Case(1, 2 * 3436 + 1, 39, 128, 512)

# conv1 (one input channel; a thread owns 8 channels, a block pass covers ppi = 256 / (C / 8) positions of an output row, a
# block walks C1F_ROWS = 4 output rows (b, t1)).  C: both ends of the thread mapping (8: ppi = 256, 2048: ppi = 1) and what
# lies between; F: 3 and 4 (one position), 23 (F1 = 11), 80 and 83 (F1 = 39, 41: below and just above ppi = 32 and 64 ...);
# T: odd and even; B T1 is no multiple of 4 wherever B = 3, so a row group of a block crosses a batch boundary.
C1_CS = [8, 16, 64, 512, 1024, 2048]
C1_FS = [3, 4, 23, 80, 83]
C1_TS = [3, 4, 7, 8, 11]
C1_ROWS = 4


def c1_admitted(C: int) -> bool:
    """The C the ABI takes: C % 8 == 0, 256 % (C / 8) == 0, C <= 2048."""
    return C > 0 and C % 8 == 0 and 256 % (C // 8) == 0 and C <= 2048


def c1_cases() -> list:
    """Every C with every F, every T and both B: rotations, 30 cases."""
    cases = []
    for ci, C in enumerate(C1_CS):
        for fi, Fd in enumerate(C1_FS):
            T = C1_TS[(ci + fi) % 5]
            cases.append(Case(3 if (ci + fi) % 2 == 0 else 1, T, Fd, 1, C))
    return cases


C1_CASES = c1_cases()
