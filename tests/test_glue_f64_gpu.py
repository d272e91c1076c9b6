"""The conv-module and LayerNorm glue kernels (csrc/glue.hip: add_layernorm_kernel, split_planes_kernel; csrc/dwconv.hip:
dwconv_kernel ACT 0-3, dwconv_wgrad_kernel and its reduce) against the float64 specification of tests/glue_ref.py: every output
element within its derived bound (most bf16 elements: bit-identical), max(err / bound) <= 1 over ALL elements, the worst ratio
per kernel and form recorded with tests/parity_log.  The cases are those tests/test_glue_ref.py runs through float32 torch.

  add_layernorm   C 8 (one lane), 72, 504, 512 (one full iteration), 520 (one lane of the second), 1024; rows 1, 3, 4, 5 (four
                  waves make a block) and (3, 7) with lens [7, 3, 1]; fp32, bf16, fp32 -> bf16, planes (split1), fp32 + planes
                  (split2); every form of glue_ref.LN_FORMS; rows beyond lens of y (mask_y) and of x (zero_rows) are NaN
  split_planes    pafc_split_planes itself, with ldx > cols and lo_off > cols, bit-exact
  dwconv forward  glue_ref.conv_cases: K 3, 4, 7, 15, 31 x T_out, C (130: lanes return early, 514 / 1024: grid.y == 2), left_pad,
                  T_in, lens and bias; x a column slice of a NaN buffer, NaN beyond lens
  ACT 3           glue_ref.act3_cases through depthwise_conv1d_cl_ln_silu
  gradients       glue_ref.wgrad_cases through depthwise_conv1d_cl_wgrad (two calls bit-identical), dx through the autograd op"""
import pytest
import torch

from tests import glue_ref as R
from tests import parity_log

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
_WORST = {}


def _note(kernel, form, ratio):
    key = (kernel, form)
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    parity_log.record(f"glue f64/{kernel}", **{form: _WORST[key]})


def _run_ln(c):
    """One hip_ops.add_layernorm call -> its outputs by name."""
    from paper_accurate_fast_cheap_amd import hip_ops
    rows, C = c["x"].shape
    kw = dict(out_dtype=c["odt"], silu=c["silu"], zero_rows=c["zero_rows"], lens=c["lens"], T=c["T"] if c["lens"] is not None else 0,
              mask_y=c["mask_y"], gamma2=c["g2"], beta2=c["b2"], want_ln=c["want_ln"], want_x=c["want_x"], split1=c["split1"],
              split2=c["split2"])
    got = {}
    for k in ("stats_x", "stats_o1"):
        if c[k]:
            got[k] = torch.full((rows, 8, 2), float("nan"), dtype=F32, device=c["x"].device)
            kw["stats_out1" if k == "stats_o1" else k] = got[k]
    if c["slice"]:
        got["wide"] = torch.full((rows, C + 24), 7.0, dtype=c["odt"], device=c["x"].device)
        kw["out1"] = got["wide"][:, 8:8 + C]
    got["x_out"], got["o1"], got["o2"] = hip_ops.add_layernorm(c["x"], c["y"], c["alpha"], c["g1"], c["b1"], **kw)
    return got


def _planes_ratio(p, want, bnd, what):
    """A plane output [hi | lo] against the fp32 reference value."""
    C = want.shape[-1]
    assert p.dtype == BF16 and p.shape[-1] == 2 * C, what
    hi, lo = p[..., :C].double(), p[..., C:].double()
    ok = torch.isfinite(hi)
    assert bool((lo.abs()[ok] <= R.bf16_half_step(hi)[ok]).all()), what + ": |lo| above half a step of hi"
    return R.worst_ratio(hi + lo, want, R.planes_bound(want, bnd))


def _check_ln(c, got, ref):
    """-> {output: worst err / bound}; structural requirements are asserted here."""
    what = f"C={c['C']} B={c['B']} T={c['T']} {c['pair']} {c['form']}"
    res = {}
    if c["y"] is None:
        assert got["x_out"] is c["x"], what
    elif not c["want_x"]:
        assert got["x_out"] is None, what
    else:
        assert got["x_out"].dtype == c["xdt"], what
        res["x_new"] = R.worst_ratio(got["x_out"], ref["x_new"], R.bound(ref, "x_new"))
    if not c["want_ln"]:
        assert got["o1"] is None and got["o2"] is None, what
    else:
        if c["split1"]:
            res["o1"] = _planes_ratio(got["o1"], ref["o1"], R.bound(ref, "o1"), what)
        else:
            assert got["o1"].dtype == c["odt"], what
            res["o1"] = R.worst_ratio(got["o1"], ref["o1"], R.bound(ref, "o1"))
        if c["slice"]:
            w = got["wide"]
            assert bool((w[:, :8] == 7).all()) and bool((w[:, 8 + c["C"]:] == 7).all()), what + ": columns beside out1 touched"
        if c["g2"] is not None:
            if c["split1"] or c["split2"]:
                res["o2"] = _planes_ratio(got["o2"], ref["o2"], R.bound(ref, "o2"), what)
            else:
                res["o2"] = R.worst_ratio(got["o2"], ref["o2"], R.bound(ref, "o2"))
        else:
            assert got["o2"] is None, what
    for k in ("stats_x", "stats_o1"):
        if c[k]:
            res[k] = R.worst_ratio(got[k], ref[k], R.bound(ref, k))           # pairs 1-7: bound 0, exact zeros
    return res


@pytest.mark.parametrize("pair", R.LN_PAIRS)
@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_add_layernorm(hip, C, pair):
    bad = []
    for B, T in R.LN_ROWS:
        for form in R.ln_forms_of(pair):
            c = R.make_ln_case(C, B, T, pair, form, device=DEV)
            res = _check_ln(c, _run_ln(c), R.ln_reference(c))
            for k, v in res.items():
                _note(f"add_layernorm {pair}", f"{form}: {k}", v)
            if max(res.values(), default=0.0) > 1.0:
                bad.append((C, B, T, form, res))
    print(f"add_layernorm {pair} C={C}: worst err / bound", max((v for k, v in _WORST.items() if k[0] == f"add_layernorm {pair}"), default=0.0))
    assert not bad, bad


def test_add_layernorm_refuses_more_than_1024_channels(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd._lib import PafcError
    x = torch.zeros(2, 1032, device=DEV)
    with pytest.raises(PafcError):
        hip_ops.add_layernorm(x, None, 1.0, torch.ones(1032, device=DEV), torch.zeros(1032, device=DEV))


@pytest.mark.parametrize("triple", [False, True])
@pytest.mark.parametrize("cols", [8, 72, 520])
@pytest.mark.parametrize("rows", [1, 5])
def test_split_planes_is_bit_exact(hip, rows, cols, triple):
    """pafc_split_planes with ldx > cols and lo_off > cols; the columns between and beyond the planes stay as they were."""
    from paper_accurate_fast_cheap_amd import _lib
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-12, 12, (rows, cols), generator=g).float())
    special = torch.tensor([0.0, -0.0, 1.0, -1.5, 0.33984375, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(2 + 2.0 ** -7), -(2 + 3 * 2.0 ** -7),
                            1e30, -1e30, 1e-30, -1e-30, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20])
    flat = x.flatten()
    n = min(flat.numel(), special.numel())
    flat[:n] = special[:n]
    if flat.numel() > 2 * special.numel():
        flat[-special.numel():] = special
    buf = torch.full((rows, cols + 8), float("nan"), device=DEV)
    buf[:, :cols] = x.to(DEV)
    lo_off = cols + 8
    ldo = (3 * cols if triple else lo_off + cols) + 8
    out = torch.full((rows, ldo), 7.0, dtype=BF16, device=DEV)
    rc = hip.pafc_split_planes(rows, cols, _lib.ptr(buf), buf.stride(0), _lib.ptr(out), ldo, lo_off, int(triple), _lib.stream_of(buf))
    assert rc == 0
    want = R.split_planes_rounded(x, triple).to(BF16)
    bits = lambda t: t.contiguous().view(torch.int16).cpu()
    if triple:
        assert torch.equal(bits(out[:, :3 * cols]), bits(want))
        assert bool((out[:, 3 * cols:] == 7).all())
    else:
        assert torch.equal(bits(out[:, :cols]), bits(want[:, :cols])) and torch.equal(bits(out[:, lo_off:lo_off + cols]), bits(want[:, cols:]))
        assert bool((out[:, cols:lo_off] == 7).all()) and bool((out[:, lo_off + cols:] == 7).all())
    _note("split_planes", "triple" if triple else "double", 0.0)


def _ld(x):
    return x.shape[-1] if x.is_contiguous() else x.stride(1)


def _run_conv(hip, c):
    from paper_accurate_fast_cheap_amd import _lib, hip_ops
    if c["act"] in (0, 1):
        return hip_ops.depthwise_conv1d_cl(c["x"], c["w"], c["bias"], c["pad"], c["T_out"], glu=c["act"] == 1, lens=c["lens"])
    x = c["x"]
    y = torch.empty(c["B"], c["T_out"], c["C"], dtype=x.dtype, device=x.device)
    rc = hip.pafc_dwconv1d_cl_ex(_lib.dtype_code(x.dtype), c["B"], c["T_in"], c["C"], c["K"], c["pad"], c["T_out"], _lib.ptr(x), _ld(x),
                                 _lib.ptr(c["w"]), _lib.ptr(c["bias"]), _lib.ptr(y), c["act"], _lib.ptr(c["lens"]), _lib.stream_of(x))
    assert rc == 0
    return y


_DT = {F32: "fp32", BF16: "bf16"}


@pytest.mark.parametrize("K", R.CONV_KS)
def test_dwconv_forward(hip, K):
    bad = []
    for spec in (s for s in R.conv_cases() if s["K"] == K):
        c = R.make_conv_case(**spec, device=DEV)
        ref = R.conv_reference(c)
        got = _run_conv(hip, c)
        assert got.shape == ref["y"].shape and got.dtype == c["dtype"]
        ratio = R.worst_ratio(got, ref["y"], R.bound(ref, "y"))
        _note(f"dwconv ACT {c['act']} {_DT[c['dtype']]}", f"K={K}", ratio)
        if ratio > 1.0:
            bad.append(({k: v for k, v in spec.items()}, ratio))
    print({k: v for k, v in _WORST.items() if k[0].startswith("dwconv ACT") and k[1] == f"K={K}"})
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("glu", [False, True])
def test_dwconv_wrapper_takes_a_column_slice_and_refuses_other_layouts(hip, dtype, glu):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd._lib import PafcError
    c = R.make_conv_case(K=15, T_out=33, C=130, pad=7, tin="same", lens=17, bias=True, act=int(glu), dtype=dtype, wide=True, device=DEV)
    x = c["x"]
    assert not x.is_contiguous()
    args = (c["w"], c["bias"], 7, 33)
    got = hip_ops.depthwise_conv1d_cl(x, *args, glu=glu, lens=c["lens"])
    assert torch.equal(got, hip_ops.depthwise_conv1d_cl(x.contiguous(), *args, glu=glu, lens=c["lens"]))
    ref = R.conv_reference(c)
    assert R.worst_ratio(got, ref["y"], R.bound(ref, "y")) <= 1.0
    wide = x.contiguous()
    for wrong in (wide.transpose(1, 2).contiguous().transpose(1, 2),       # channel stride T
                  wide[:, ::2],                                            # frames two rows apart, sequences not T rows apart
                  torch.cat([wide, wide], -1)[..., 1:1 + wide.shape[-1]],  # a channel pair that straddles a dword
                  wide.cpu()):
        with pytest.raises(PafcError):
            hip_ops.depthwise_conv1d_cl(wrong, *args, glu=glu)


@pytest.mark.parametrize("K", [15, 31])
def test_dwconv_act3_layernorm_silu_epilogue(hip, K):
    from paper_accurate_fast_cheap_amd import hip_ops
    bad = []
    for spec in (s for s in R.act3_cases() if s["K"] == K):
        c = R.make_act3_case(spec, device=DEV)
        ref = R.conv_reference(c, gamma=c["gamma"], beta=c["beta"])
        got = hip_ops.depthwise_conv1d_cl_ln_silu(c["x"], c["w"], c["bias"], c["pad"], c["T_out"], c["gamma"], c["beta"], 1e-5,
                                                  lens=c["lens"])
        ratio = R.worst_ratio(got, ref["y"], R.bound(ref, "y"))
        _note("dwconv ACT 3 bf16", f"K={K} shift={spec['shift']:g}", ratio)
        if ratio > 1.0:
            bad.append((spec, ratio))
    print({k: v for k, v in _WORST.items() if k[0] == "dwconv ACT 3 bf16"})
    assert not bad, bad


@pytest.mark.parametrize("K", R.CONV_KS)
def test_dwconv_weight_gradient(hip, K):
    from paper_accurate_fast_cheap_amd import hip_ops
    bad = []
    for spec in (s for s in R.wgrad_cases() if s["K"] == K):
        c = R.make_wgrad_case(**spec, device=DEV)
        ref = R.dwconv_wgrad_rounded(c["x"], c["dy"], K, c["pad"])
        dw, db = hip_ops.depthwise_conv1d_cl_wgrad(c["x"], c["dy"], K, c["pad"], want_bias=c["want_bias"])
        dw2, db2 = hip_ops.depthwise_conv1d_cl_wgrad(c["x"], c["dy"], K, c["pad"], want_bias=c["want_bias"])
        assert dw.dtype == F32 and dw.shape == ref["dw"].shape and torch.equal(dw, dw2)
        res = {"dw": R.worst_ratio(dw, ref["dw"], R.bound(ref, "dw"))}
        if c["want_bias"]:
            assert torch.equal(db, db2)
            res["db"] = R.worst_ratio(db, ref["db"], R.bound(ref, "db"))
        else:
            assert db is None
        for k, v in res.items():
            _note(f"dwconv wgrad {_DT[spec['dtype']]}", f"K={K}: {k}", v)
        if max(res.values()) > 1.0:
            bad.append((spec, res))
    print({k: v for k, v in _WORST.items() if k[0].startswith("dwconv wgrad") and k[1].startswith(f"K={K}:")})
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("K,pad", [(4, 3), (31, 15)])
def test_dwconv_autograd_input_gradient(hip, K, pad, dtype):
    """dx of depthwise_conv1d_cl_autograd at T = 17: the forward kernel on dy with flipped taps and left_pad' = K - 1 - left_pad,
    against the float64 transpose convolution dx[s] = sum_k w[k] dy[s + left_pad - k]."""
    from paper_accurate_fast_cheap_amd import hip_ops
    B, T, C = 2, 17, 130
    g = torch.Generator().manual_seed(K)
    x = torch.randn(B, T, C, generator=g).to(dtype).to(DEV).requires_grad_()
    w = (0.2 * torch.randn(C, 1, K, generator=g)).to(dtype).float().to(DEV)          # master weights the cast keeps exactly
    gy = torch.randn(B, T, C, generator=g).to(dtype).to(DEV)
    hip_ops.depthwise_conv1d_cl_autograd(x, w, None, pad, T).backward(gy)
    ref = R.dwconv_rounded(gy, w.to(dtype).flip(-1), None, K - 1 - pad, T)
    G = gy.double()
    direct = torch.zeros(B, T, C, dtype=torch.float64, device=DEV)
    for k in range(K):
        for s in range(T):
            if 0 <= s + pad - k < T:
                direct[:, s] += w.double()[:, 0, k] * G[:, s + pad - k]
    assert float((ref["conv"] - direct).abs().max()) <= 1e-12
    assert x.grad.dtype == dtype
    ratio = R.worst_ratio(x.grad, ref["y"], R.bound(ref, "y"))
    _note(f"dwconv dx {_DT[dtype]}", f"K={K} left_pad={pad}", ratio)
    assert ratio <= 1.0, ratio
