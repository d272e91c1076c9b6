"""State carry of the uni-directional Mamba-2 slot, the parts that need no GPU: the stateful scan's place in the C ABI
(header, signature table, exported symbol, argument checks that answer before a launch), the DEFINITION of the two carries
-- "conv": the last d_conv - 1 pre-convolution xBC rows, "ssm": h after the last step, float32 (B, H, 128, 64)
[state dim][head channel] -- as a float64 restatement of the block (chunked == whole sequence for any cuts, whole sequence
== oracle/mamba2_oracle.py), and the refusals of a bidirectional encoder."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import mamba2_oracle as MO
from tests.test_abi import _header_prototypes, so_path  # noqa: F401  (so_path: the fixture that builds the library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pafc_mamba2_scan_state"
ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -4, -8


def test_stateful_scan_is_declared_bound_and_exported(so_path):  # noqa: F811
    from paper_accurate_fast_cheap_amd import _lib
    protos = _header_prototypes()
    assert NAME in protos, "include/pafc_encoder_ops.h does not declare the stateful scan"
    ret, params = protos[NAME]
    assert ret == "int" and [n for _, n in params] == [
        "B", "L", "H", "xbc", "ldx", "dt", "log_a", "D", "y_f32", "y_bf16", "s_in", "s_out", "reverse", "chunk_len",
        "workspace", "workspace_bytes", "stream"]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 17
    assert argtypes[4] is ctypes.c_long and argtypes[15] is ctypes.c_size_t and argtypes[10] is ctypes.c_void_p
    assert hasattr(ctypes.CDLL(so_path), NAME)


def test_stateful_scan_argument_checks_answer_before_any_launch(so_path):  # noqa: F811
    from paper_accurate_fast_cheap_amd import _lib
    L = ctypes.CDLL(so_path)
    fn = getattr(L, NAME)
    fn.restype, fn.argtypes = _lib.SIGNATURES[NAME]
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 63) & ~63
    one, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)            # 64-byte aligned / 4-byte aligned only
    NULL = None
    #            B  L   H  xbc   ldx  dt   la   D    y32   y16   s_in  s_out rev Lc ws    nws str
    assert fn(1, 64, 4, NULL, 512, one, one, NULL, one, NULL, NULL, NULL, 0, 0, NULL, 0, NULL) == ERR_NULL
    assert fn(1, 64, 4, one, 512, one, one, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, 0, NULL) == ERR_NULL     # no output
    assert fn(1, 64, 4, one, 512, one, one, one, one, one, NULL, NULL, 0, 0, NULL, 0, NULL) == ERR_NULL        # both outputs
    assert fn(1, 64, 4, one, 512, one, one, NULL, NULL, one, NULL, NULL, 0, 0, NULL, 0, NULL) == ERR_NULL      # bf16 form, no D
    assert fn(1, 64, 4, one, 100, one, one, NULL, one, NULL, one, one, 0, 0, NULL, 0, NULL) == ERR_DIMS        # row too short
    assert fn(0, 64, 4, one, 512, one, one, NULL, one, NULL, one, one, 0, 0, NULL, 0, NULL) == ERR_DIMS
    assert fn(1, 64, 4, one, 512, one, one, NULL, one, NULL, odd, NULL, 0, 0, NULL, 0, NULL) == ERR_ALIGN      # s_in
    assert fn(1, 64, 4, one, 512, one, one, NULL, one, NULL, one, odd, 0, 0, NULL, 0, NULL) == ERR_ALIGN       # s_out
    assert fn(1, 64, 4, one, 512, one, one, one, NULL, odd, NULL, NULL, 0, 0, NULL, 0, NULL) == ERR_ALIGN      # y_bf16 (8 bytes)
    # several chunks asked for, a workspace that is too small
    assert fn(1, 3000, 4, one, 512, one, one, NULL, one, NULL, one, one, 0, 256, one, 8, NULL) == ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------------------------
# the carries, defined in float64
# ---------------------------------------------------------------------------------------------------------------------
def block_f64(u, sd, p, conv_in=None, ssm_in=None, headdim=64, d_state=128, d_conv=4):
    """The Mamba-2 block on one chunk from its two carries, float64 -> (out, conv_out, ssm_out).
    conv_in (B, d_conv - 1, d_inner + 2 d_state): the pre-convolution xBC rows in front of the chunk (None: zero rows = the
    causal zero padding); ssm_in (B, H, d_state, headdim): h before the chunk's first step (None: zero)."""
    g = lambda n: sd[p + n].double()
    B, L, _ = u.shape
    d_inner = g("out_proj.weight").shape[1]
    H = d_inner // headdim
    zxbcdt = F.linear(u.double(), g("in_proj.weight"))
    z, xBC, dt = torch.split(zxbcdt, [d_inner, d_inner + 2 * d_state, H], dim=-1)
    if conv_in is None:
        conv_in = xBC.new_zeros(B, d_conv - 1, xBC.shape[-1])
    xp = torch.cat([conv_in.double(), xBC], dim=1)
    conv_out = xp[:, -(d_conv - 1):]
    xBC = F.silu(F.conv1d(xp.transpose(1, 2), g("conv1d.weight"), g("conv1d.bias"), groups=xp.shape[-1]).transpose(1, 2))
    x, Bm, Cm = torch.split(xBC, [d_inner, d_state, d_state], dim=-1)
    dt = F.softplus(dt + g("dt_bias"))
    A = -torch.exp(g("A_log"))
    x = x.reshape(B, L, H, headdim)
    h = ssm_in.double() if ssm_in is not None else torch.zeros(B, H, d_state, headdim, dtype=torch.float64)
    ys = []
    for t in range(L):
        a = torch.exp(dt[:, t] * A)                                                          # (B, H)
        h = h * a[:, :, None, None] + Bm[:, t, None, :, None] * (dt[:, t, :, None] * x[:, t])[:, :, None, :]
        ys.append(torch.einsum("bhnp,bn->bhp", h, Cm[:, t]) + g("D")[None, :, None] * x[:, t])
    y = torch.stack(ys, 1).reshape(B, L, d_inner)
    y = y * F.silu(z)
    y = y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + 1e-5) * g("norm.weight")
    return F.linear(y, g("out_proj.weight")), conv_out, h


def chunked_f64(u, sd, p, cuts):
    outs, conv, ssm, a = [], None, None, 0
    for n in cuts:
        o, conv, ssm = block_f64(u[:, a:a + n], sd, p, conv, ssm)
        outs.append(o)
        a += n
    assert a == u.shape[1]
    return torch.cat(outs, 1), conv, ssm


def _block(seed=3, d_model=128):
    from paper_accurate_fast_cheap_amd.transformer.mamba2 import Mamba2
    torch.manual_seed(seed)
    m = Mamba2(d_model, headdim=64).eval()
    with torch.no_grad():
        m.norm.weight.uniform_(0.5, 1.5)
        m.D.uniform_(0.5, 1.5)
        m.conv1d.weight.normal_(0, 0.3)
    return {"m." + k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("cuts", [(1, 2, 3, 50, 7, 1, 1, 40), (105,), (3, 3, 3, 96), (16,) * 6 + (9,), (64, 1, 40)])
def test_chunked_block_with_carries_is_the_whole_sequence(cuts):
    sd = _block()
    L = sum(cuts)
    u = torch.randn(2, L, 128, generator=torch.Generator().manual_seed(17), dtype=torch.float64)
    whole, conv_w, ssm_w = block_f64(u, sd, "m.")
    got, conv, ssm = chunked_f64(u, sd, "m.", cuts)
    assert conv.shape == (2, 3, 256 + 256) and ssm.shape == (2, 4, 128, 64)      # d_inner 256 = 4 heads of 64
    torch.testing.assert_close(got, whole, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(conv, conv_w, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ssm, ssm_w, rtol=1e-12, atol=1e-12)


def test_restatement_is_the_oracle_block():
    sd = _block(seed=5)
    u = torch.randn(2, 77, 128, generator=torch.Generator().manual_seed(18))
    want = MO.mamba2_forward(u, sd, "m.")
    got, _, _ = block_f64(u, sd, "m.")
    d = (got - want.double()).abs()
    print(f"float64 restatement vs fp32 oracle: max {float(d.max()):.3g} (|ref| max {float(want.abs().max()):.3g})")
    torch.testing.assert_close(got.float(), want, rtol=1e-4, atol=1e-5)
    got_c, _, _ = chunked_f64(u, sd, "m.", (5, 1, 70, 1))
    torch.testing.assert_close(got_c.float(), want, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# what stays refused
# ---------------------------------------------------------------------------------------------------------------------
def _encoder(direction, causal=True):
    from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder
    torch.manual_seed(2)
    return ConformerEncoder(80, output_size=128, attention_heads=2, linear_units=256, num_blocks=2, input_layer="conv2d",
                            cnn_module_kernel=15, causal=causal, cnn_module_norm="layer_norm", activation_type="swish",
                            pos_enc_layer_type="rel_pos", selfattention_layer_type="mamba_att", rnn_att_version="mamba2",
                            rnn_att_direction=direction).eval()


def test_bidirectional_mamba_has_no_state_carry():
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.encoder_layer import streamable_slot
    bi, uni = _encoder("bi"), _encoder("uni")
    assert not streamable_slot(bi.encoders[0].self_attn) and streamable_slot(uni.encoders[0].self_attn)
    x = torch.zeros(1, 8, 128)
    with pytest.raises(NotImplementedError, match="uni-directional"):
        bi.encoders[0].forward_carry(x, None)
    with pytest.raises(NotImplementedError):
        _encoder("bi", causal=False).encoders[0].forward_lookahead(x, None)
    with pytest.raises(NotImplementedError):
        bi.encoders[0].self_attn.forward_state(x)
    model = ASRModel(50, bi, CTC(50, 128)).eval()
    with pytest.raises(ValueError, match="uni-directional"):
        model._stream_windows(torch.zeros(1, 200, 80), 16, "stream_ctc_search")
    # the uni-directional model is accepted: the walk is built (running it needs the GPU: there is no CPU fallback)
    walk = ASRModel(50, uni, CTC(50, 128)).eval()._stream_windows(torch.zeros(1, 200, 80), 16, "stream_ctc_search")
    assert hasattr(walk, "__next__")
    with pytest.raises(NotImplementedError, match="GPU"):
        uni.encoders[0].self_attn.forward_state(x)
