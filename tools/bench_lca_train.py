"""Training the Conformer baseline (limited_rel_selfattn) at the training-batch shape of the other training benches, B = 32,
T' = 499, 8 heads, w = 256: forward + backward of the attention alone on this package's kernels (pafc_mha_band_lse +
pafc_mha_band_bwd through hip_ops.mha_band_train) next to autograd through the same banded attention written with framework
ops (tools/bench_lca_encoder.framework_band_attention) on the same GPU, and one training step (forward + backward) of the
12-layer baseline encoder with its launch count and the attention kernels' share.  No pass mark: the numbers go into DESIGN.md
with the command that produced them.

    python tools/bench_lca_train.py
    python tools/bench_lca_train.py --steps attn_f32,attn_bf16 --batch 8

Every step runs in a process of its own under its own time limit and prints one JSON line; the first step that fails or
runs out of time ends the run (nothing more is started on a GPU that may have faulted)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_lca_encoder import DK, H, _time, framework_band_attention  # noqa: E402

STEPS = {"attn_f32": 240, "attn_bf16": 240, "step_f32": 420, "step_bf16": 420}            # step -> its time limit, seconds
BAND_KERNELS = ("mha_band_kernel", "mha_band_bwd_dq_kernel", "mha_band_bwd_dkv_kernel", "mha_band_bwd_reduce_kernel")


def step_attention(args, dtype_name):
    import torch
    from paper_accurate_fast_cheap_amd import hip_ops
    dtype = torch.float32 if dtype_name == "f32" else torch.bfloat16
    B, T, w, D = args.batch, args.frames, args.context, H * DK
    t_pad = -(-T // (2 * w)) * 2 * w
    g = torch.Generator(device="cuda").manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")                             # noqa: E731
    qkv = rnd(B * T, 3 * D).to(dtype).requires_grad_(True)                                   # one stacked projection
    p = rnd(T, D).to(dtype).requires_grad_(True)
    u, vb = (rnd(H, DK) * 0.5).to(dtype).requires_grad_(True), (rnd(H, DK) * 0.5).to(dtype).requires_grad_(True)
    dout = rnd(B * T, D).to(dtype)
    leaves = (qkv, p, u, vb)

    def ours():
        out = hip_ops.mha_band_train(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], p, u, vb, B, H, w, t_pad)
        return torch.autograd.grad(out, leaves, dout)

    def ours_forward():
        with torch.no_grad():
            return hip_ops.mha_band_lse(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], p, u, vb, B, H, w, t_pad)

    def framework():
        v4 = lambda t: t.reshape(B, T, H, DK)                                                # noqa: E731
        out = framework_band_attention(v4(qkv[:, :D]), v4(qkv[:, D:2 * D]), v4(qkv[:, 2 * D:]), p.view(T, H, DK), u, vb, w, t_pad)
        return torch.autograd.grad(out.reshape(B * T, D), leaves, dout)

    ms, ms_fwd = _time(ours, args.iters), _time(ours_forward, args.iters)
    ms_fw = _time(framework, max(1, args.iters // 4))
    diffs = [(a.float() - b.float()).abs().max().item() for a, b in zip(ours(), framework())]
    return dict(step=f"attn_{dtype_name}", B=B, T=T, heads=H, w=w, t_pad=t_pad, kernels_fwd_bwd_ms=round(ms, 4),
                kernels_fwd_ms=round(ms_fwd, 4), kernels_bwd_ms=round(ms - ms_fwd, 4), launches_fwd_bwd=4,
                framework_autograd_fwd_bwd_ms=round(ms_fw, 4), speedup_vs_framework=round(ms_fw / ms, 2),
                max_abs_diff_vs_framework=dict(zip(("dqkv", "dp", "du", "dvb"), diffs)))


def step_train(args, dtype_name):
    import torch
    from torch.profiler import ProfilerActivity, profile
    from paper_accurate_fast_cheap_amd.utils.init_model import init_model
    conf = dict(activation_type="swish", attention_dropout_rate=0.0, attention_heads=H, cnn_module_kernel=31,
                cnn_module_norm="layer_norm", dropout_rate=0.1, input_layer="conv2d", linear_units=2048, normalize_before=True,
                num_blocks=args.layers, output_size=H * DK, pos_enc_layer_type="rel_pos", positional_dropout_rate=0.1,
                use_cnn_module=True, selfattention_layer_type="limited_rel_selfattn",
                att_context_size=[args.context, args.context], global_tokens=0, global_tokens_spacing=1)
    configs = dict(encoder="conformer", encoder_conf=conf, input_dim=80, output_dim=5000, ctc="ctc", ctc_conf={"ctc_blank_id": 0},
                   model_conf={}, dataset_conf={})

    class A:
        checkpoint = None
    torch.manual_seed(777)
    model, _ = init_model(A(), configs)
    enc = model.encoder.cuda().train()
    frames = 4 * args.frames + 6                                            # -> args.frames frames after the 4x subsampling
    feats = torch.randn(args.batch, frames, 80, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    lens = torch.full((args.batch,), frames, device="cuda")

    def run():
        enc.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype_name == "bf16"):
            y = enc(feats, lens)[0]
        y.float().sum().backward()
        return y

    ms = _time(run, 3)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        y = run()
        torch.cuda.synchronize()
    kernels = [e for e in prof.key_averages() if e.device_time_total > 0]
    total = sum(e.device_time_total for e in kernels)
    band = {n: round(sum(e.device_time_total for e in kernels if n in e.key and (n != "mha_band_kernel" or "bwd" not in e.key))
                     / 1e3, 3) for n in BAND_KERNELS}
    finite = all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in enc.parameters())
    return dict(step=f"step_{dtype_name}", what="encoder forward + backward, sum-of-outputs loss", B=args.batch,
                frames_after_subsampling=int(y.shape[1]), layers=args.layers, w=args.context, ms_per_step=round(ms, 2),
                kernel_launches_per_step=int(sum(e.count for e in kernels)), device_ms_per_step=round(total / 1e3, 2),
                band_kernels_device_ms=band, band_kernels_share=round(sum(band.values()) * 1e3 / total, 4),
                gradients_finite=finite, peak_mem_GB=round(torch.cuda.max_memory_allocated() / 2**30, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--context", type=int, default=256, help="w = att_context_size[0] = att_context_size[1]")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=499, help="frames per batch row after subsampling")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20, help="timed attention passes")
    ap.add_argument("--steps", default=",".join(STEPS), help="comma-separated subset of " + ", ".join(STEPS))
    ap.add_argument("--step", help=argparse.SUPPRESS)                         # a child process: run this one step
    args = ap.parse_args()
    if args.step:
        kind, dtype_name = args.step.rsplit("_", 1)
        print(json.dumps((step_attention if kind == "attn" else step_train)(args, dtype_name)), flush=True)
        return 0
    for name in args.steps.split(","):
        if name not in STEPS:
            ap.error(f"unknown step {name!r}")
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--context", str(args.context), "--batch", str(args.batch),
               "--frames", str(args.frames), "--layers", str(args.layers), "--iters", str(args.iters)]
        try:
            rc = subprocess.run(cmd, timeout=STEPS[name]).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(step=name, error=f"no result within {STEPS[name]} s")), flush=True)
            return 124
        if rc != 0:
            print(json.dumps(dict(step=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
