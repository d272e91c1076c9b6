#!/usr/bin/env python3
"""Launch tracer for the five layer schedules of transformer/fused.py: run each schedule once on a seeded two-layer encoder and
print ONE JSON with, per case, every kernel-library call the executor made and a sha256 of every output and carry tensor.  Two
commits whose JSONs are identical issue the same launches with the same arguments and compute the same bits.

Recorded: every public function of hip_ops, wkv6_forward / wkv6_forward_bidir as bound in fused, and torch.bmm / torch.cat /
F.linear as fused sees them -- as [name, {argument: [shape, dtype, stride]}, {argument: scalar}] with the arguments bound to the
callee's signature (a default passed explicitly and a default left out are the same call).  A call without any tensor argument
(hip_ops.skinny_ok(rows, N, K) and the other shape questions) launches nothing and is not recorded.

    python tools/trace_fused_schedules.py > trace.json          (needs the GPU and the built library)"""
import functools
import hashlib
import inspect
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from paper_accurate_fast_cheap_amd import hip_ops
from paper_accurate_fast_cheap_amd.transformer import fused
from paper_accurate_fast_cheap_amd.transformer.encoder import ConformerEncoder

TRACE = []


def describe(v):
    if isinstance(v, torch.Tensor):
        return [list(v.shape), str(v.dtype), list(v.stride())]
    if isinstance(v, (tuple, list)):
        return [describe(e) for e in v]
    if isinstance(v, (bool, int, float, str, torch.dtype, type(None))):
        return v if not isinstance(v, torch.dtype) else str(v)
    return type(v).__name__                           # (sentinel defaults and the like: no addresses in the trace)


def has_tensor(v):
    return isinstance(v, torch.Tensor) or (isinstance(v, (tuple, list)) and any(has_tensor(e) for e in v))


def recorder(name, fn):
    try:
        sig = inspect.signature(fn)
    except (TypeError, ValueError):                   # builtins (torch.bmm, torch.cat): positional order as passed
        sig = None

    @functools.wraps(fn)
    def call(*a, **kw):
        if sig is not None:
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = dict(bound.arguments)
        else:
            args = dict({str(i): v for i, v in enumerate(a)}, **kw)
        if any(has_tensor(v) for v in args.values()):
            TRACE.append([name, {k: describe(v) for k, v in args.items() if has_tensor(v)},
                          {k: describe(v) for k, v in args.items() if not has_tensor(v)}])
        return fn(*a, **kw)
    return call


class Seen:
    """A module as fused sees it, with some attributes replaced."""

    def __init__(self, mod, **replaced):
        self.__dict__.update(replaced, _mod=mod)

    def __getattr__(self, name):
        return getattr(self._mod, name)


def install():
    for name, fn in list(vars(hip_ops).items()):
        if inspect.isfunction(fn) and fn.__module__ == hip_ops.__name__ and not name.startswith("_"):
            setattr(hip_ops, name, recorder("hip_ops." + name, fn))
    fused.wkv6_forward = recorder("wkv6_forward", fused.wkv6_forward)
    fused.wkv6_forward_bidir = recorder("wkv6_forward_bidir", fused.wkv6_forward_bidir)
    fused.torch = Seen(torch, bmm=recorder("torch.bmm", torch.bmm), cat=recorder("torch.cat", torch.cat))
    fused.F = Seen(F, linear=recorder("F.linear", F.linear))


def encoder(C, dtype, slot="rwkv_tmix60_bidirectional", direction="bi", kernel=15, causal=False, slot_bf16=True):
    torch.manual_seed(C + kernel)
    conf = dict(output_size=C, attention_heads=C // 64, linear_units=4 * C, num_blocks=2, input_layer="conv2d", normalize_before=True,
                cnn_module_kernel=kernel, causal=causal, use_cnn_module=True, cnn_module_norm="layer_norm", activation_type="swish",
                pos_enc_layer_type="rel_pos", selfattention_layer_type=slot, rnn_att_direction=direction,
                rnn_att_version="mamba2" if slot == "mamba_att" else "rwkv", rwkv_do_bfloat16=slot_bf16)
    enc = ConformerEncoder(80, **conf).eval()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("time_maa_rkvw_w1") or n.endswith("time_decay_w1"):       # zero at init: wake the LoRA branches up
                p.normal_(0, 0.02)
            if ".norm_" in n:
                p.uniform_(0.7, 1.3) if n.endswith("weight") else p.normal_(0, 0.1)
    return (enc.to(torch.bfloat16) if dtype == torch.bfloat16 else enc).cuda()


def rand(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def offline(enc, B, T, dtype, lens=None, fold_min_rows=None):
    """encoder_layers_forward on (B, T, C) rows; lens None = every row full length."""
    if fold_min_rows is not None:
        fused._LN_FOLD_MIN_ROWS = fold_min_rows
    C = enc.encoders[0].size
    masks = torch.arange(T).view(1, 1, T) < torch.tensor(lens or [T] * B).view(B, 1, 1)
    out, layers = fused.encoder_layers_forward(fused.EncoderPlan(enc.encoders), rand((B, T, C), dtype, 1), masks.cuda(),
                                               enc.after_norm, want_layers=True)
    fused._LN_FOLD_MIN_ROWS = hip_ops.DISPATCH["ln_fold_min_rows"]
    return [out] + layers


def chunk_steps(enc, B, T, step_fn, state, steps=3):
    """The layer loop of a streaming chunk step (encoder._fused_chunk_step), `steps` times; in place from the second step."""
    C, outs = enc.encoders[0].size, []
    plans = [fused.LayerPlan(l) for l in enc.encoders]
    for s in range(steps):
        x, h, pending = rand((B, T, C), torch.bfloat16, 10 + s), None, ([] if s > 0 or state[0] is not None else None)
        with hip_ops.chunk_step():
            for i, plan in enumerate(plans):
                plan.refresh()
                nxt = plans[i + 1].layer.norm_ff_macaron if i + 1 < len(plans) else enc.after_norm
                x, h, state[i] = step_fn(plan, x, state[i], h, nxt, pending)
            if pending:
                torch._foreach_copy_([d for d, _ in pending], [s_ for _, s_ in pending])
        outs += [x, h]
    return outs + [st[k] for st in state for k in sorted(st)]


def carry_step(plan, x, carry, h, nxt, pending):
    assert fused.carry_eligible(plan.layer, x)
    x, new, h = fused.layer_forward_carry(plan, x, carry, h0=h, next_norm=nxt, in_place=carry is not None, pending=pending)
    return x, h, new


def lookahead_step(plan, x, carry, h, nxt, pending):
    assert fused.lookahead_eligible(plan.layer, x)
    return fused.layer_forward_lookahead(plan, x, carry, h, nxt, pending) + (carry,)


def lookahead_steps(enc, T):
    """Steady-state look-ahead steps over seeded carry buffers: U, X2, shift, wkv per layer."""
    C, half = enc.encoders[0].size, (enc.encoders[0].conv_module.kernel_size - 1) // 2
    state = [dict(U=rand((1, 2 * half + T, C), torch.bfloat16, 20 + i), X2=rand((1, half + T, C), torch.bfloat16, 30 + i),
                  shift=rand((1, 1, C), torch.bfloat16, 40 + i), wkv=rand((1, C // 64, 64, 64), torch.float32, 50 + i) * 0.1)
             for i in range(len(enc.encoders))]
    return chunk_steps(enc, 1, T, lookahead_step, state)


def main():
    bf, f32 = torch.bfloat16, torch.float32
    uni = dict(slot="rwkv_tmix60", direction="uni")
    cases = {
        "a_general_masked_bf16": lambda: offline(encoder(128, bf), 2, 50, bf, [50, 37]),
        "b_general_fp32_slot": lambda: offline(encoder(128, f32, slot_bf16=False), 2, 50, f32, [50, 37]),
        "c_lnfold": lambda: offline(encoder(512, bf), 1, 320, bf, fold_min_rows=256),
        "d_split_masked": lambda: offline(encoder(256, f32), 2, 160, f32, [160, 101]),
        "e_split_unmasked": lambda: offline(encoder(256, f32), 2, 160, f32, fold_min_rows=256),
        "f_carry_B1": lambda: chunk_steps(encoder(512, bf, causal=True, **uni), 1, 16, carry_step, [None, None]),
        "f_carry_B3": lambda: chunk_steps(encoder(512, bf, causal=True, **uni), 3, 16, carry_step, [None, None]),
        "g_carry_mamba2": lambda: chunk_steps(encoder(128, bf, slot="mamba_att", direction="uni", causal=True), 1, 16, carry_step,
                                              [None, None]),
        "h_lookahead": lambda: lookahead_steps(encoder(512, bf, kernel=31, **uni), 32),
        "i_causal_general": lambda: offline(encoder(128, bf, causal=True), 2, 50, bf, [50, 37]),
        "i_causal_split": lambda: offline(encoder(256, f32, causal=True), 2, 160, f32, [160, 101]),
    }
    install()
    result = {}
    with torch.no_grad():
        for name, run in cases.items():
            del TRACE[:]
            tensors = run()
            torch.cuda.synchronize()
            result[name] = dict(trace=list(TRACE), sha256=[hashlib.sha256(
                t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest() if t is not None else None for t in tensors])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
