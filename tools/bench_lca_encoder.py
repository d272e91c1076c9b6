"""The Conformer baseline (limited_rel_selfattn, conf/conformer/giga.conformer_ds4k31nc_12le.LCA256-GT-FT-LFXL.max.yaml) on the
shapes the recurrent encoders are measured on: the attention launch alone (pafc_mha_band) next to the same banded attention
written with framework ops on the same GPU, and the whole 12-layer encoder on the module path.  No pass mark: the numbers go
into DESIGN.md with the command that produced them.

    python tools/bench_lca_encoder.py                                # the 30-minute file: B = 1, T' = 44 998, w = 256
    python tools/bench_lca_encoder.py --batch 8 --chunk-size 2000    # a point of the RTF grid
    python tools/bench_lca_encoder.py --context 64 --steps attn_f32,attn_bf16

Every step runs in a process of its own under its own time limit and prints one JSON line; the first step that fails or
runs out of time ends the run (nothing more is started on a GPU that may have faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"attn_f32": 240, "attn_bf16": 240, "encoder_f32": 420, "encoder_bf16": 420}      # step -> its time limit, seconds
H, DK = 8, 64


def framework_band_attention(q, k, v, p, u, vb, w, t_pad):
    """The same attention with framework ops, blocked the way the reference blocks it: query blocks of 2 w, each against the
    4 w keys around it.  q, k, v (B, T, H, dk), p (T, H, dk) -> (B, T, H, dk).  Keys of [T, t_pad) are zero rows that stay
    unmasked, keys outside [0, t_pad) and outside the band are masked."""
    import torch
    B, T, Hh, dk = q.shape
    Q = 2 * w
    nb = -(-T // Q)
    pad = lambda t, lead: torch.nn.functional.pad(t, (0, 0, 0, 0, lead, nb * Q - T + (w if lead else 0)))   # noqa: E731
    qu = pad(q + u, 0).view(B, nb, Q, Hh, dk).permute(0, 3, 1, 2, 4)                        # (B, H, nb, Q, dk)
    qv = pad(q + vb, 0).view(B, nb, Q, Hh, dk).permute(0, 3, 1, 2, 4)
    blocks = lambda t: pad(t, w).unfold(-3, 2 * Q, Q)                                        # noqa: E731 (.., nb, H, dk, 4w)
    kb, vbk = blocks(k).permute(0, 2, 1, 3, 4), blocks(v).permute(0, 2, 1, 4, 3)             # (B, H, nb, dk, 4w) / (.., 4w, dk)
    pb = blocks(p).permute(1, 0, 2, 3)                                                       # (H, nb, dk, 4w)
    s = (torch.matmul(qu, kb) + torch.matmul(qv, pb)) * 0.125                                # (B, H, nb, Q, 4w)
    i = (torch.arange(nb, device=q.device) * Q).view(nb, 1, 1) + torch.arange(Q, device=q.device).view(1, Q, 1)
    j = (torch.arange(nb, device=q.device) * Q).view(nb, 1, 1) - w + torch.arange(2 * Q, device=q.device).view(1, 1, 2 * Q)
    hidden = ((j - i).abs() > w) | (j < 0) | (j >= t_pad)
    out = torch.matmul(torch.softmax(s.masked_fill(hidden, -float("inf")), dim=-1), vbk)     # (B, H, nb, Q, dk)
    return out.permute(0, 2, 3, 1, 4).reshape(B, nb * Q, Hh, dk)[:, :T]


def _time(fn, n):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def step_attention(args, dtype_name):
    import torch
    from paper_accurate_fast_cheap_amd import hip_ops
    dtype = torch.float32 if dtype_name == "f32" else torch.bfloat16
    B, T, w, D = args.batch, args.chunk_size, args.context, H * DK
    t_pad = -(-T // (2 * w)) * 2 * w
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(B * T, 3 * D, generator=g, device="cuda").to(dtype)                    # one stacked projection
    p = torch.randn(T, D, generator=g, device="cuda").to(dtype)
    u, vb = (torch.randn(H, DK, generator=g, device="cuda") * 0.5).to(dtype), (torch.randn(H, DK, generator=g, device="cuda") * 0.5).to(dtype)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    out = torch.empty(B * T, D, dtype=dtype, device="cuda")
    ms = _time(lambda: hip_ops.mha_band(q, k, v, p, u, vb, B, H, w, t_pad, out=out), args.iters)
    v4 = lambda t: t.reshape(B, T, H, DK)                                                    # noqa: E731
    fw = lambda: framework_band_attention(v4(q), v4(k), v4(v), p.view(T, H, DK), u, vb, w, t_pad)   # noqa: E731
    ms_fw = _time(fw, max(1, args.iters // 4))
    diff = (fw().reshape(B * T, D).float() - out.float()).abs().max().item()
    # what the algorithm has to move: q, k, v and out once per batch row, p once; 384 flop per (query, key) pair of the band
    nbytes = (4 * B + 1) * T * D * qkv.element_size()
    i = torch.arange(T)
    pairs = int(((i + w).clamp(max=T - 1) - (i - w).clamp(min=0) + 1).sum())                # real keys only
    return dict(step=f"attn_{dtype_name}", B=B, T=T, heads=H, w=w, t_pad=t_pad, ms_per_launch=round(ms, 4),
                algorithm_bytes_MB=round(nbytes / 1e6, 1), GBps_of_algorithm_bytes=round(nbytes / ms / 1e6, 1),
                band_GFLOP=round(384 * pairs * B * H / 1e9, 2), TFLOPs_of_band=round(384 * pairs * B * H / ms / 1e9, 2),
                framework_ops_ms=round(ms_fw, 4), max_abs_diff_vs_framework_ops=diff)


def step_encoder(args, dtype_name):
    import torch
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
    model = model.eval().cuda()
    frames = 4 * args.chunk_size + 6                                        # -> chunk_size frames after the 4x subsampling
    feats = torch.randn(args.batch, frames, 80, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    if dtype_name == "bf16":
        model, feats = model.to(torch.bfloat16), feats.to(torch.bfloat16)
    lens = torch.full((args.batch,), frames, device="cuda")
    with torch.no_grad():
        assert model.encoder._fused(feats) is None
        run = lambda: model.encoder(feats, lens)[0]                          # noqa: E731
        t0 = time.time()
        ms = _time(run, 3)
        y = run()
    audio = args.batch * frames * 0.01
    return dict(step=f"encoder_{dtype_name}", path="module path (no fused schedule for this slot)", B=args.batch,
                frames_after_subsampling=int(y.shape[1]), layers=args.layers, w=args.context, ms_per_pass=round(ms, 2),
                audio_sec_per_sec=round(audio / ms * 1e3, 1), finite=bool(torch.isfinite(y.float()).all()),
                peak_mem_GB=round(torch.cuda.max_memory_allocated() / 2**30, 2), wall_s=round(time.time() - t0, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--context", type=int, default=256, help="w = att_context_size[0] = att_context_size[1]")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--chunk-size", type=int, default=44998, help="frames per batch row after subsampling (44 998: 30 minutes)")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20, help="timed attention launches")
    ap.add_argument("--steps", default=",".join(STEPS), help="comma-separated subset of " + ", ".join(STEPS))
    ap.add_argument("--step", help=argparse.SUPPRESS)                         # a child process: run this one step
    args = ap.parse_args()
    if args.step:
        kind, dtype_name = args.step.rsplit("_", 1)
        print(json.dumps((step_attention if kind == "attn" else step_encoder)(args, dtype_name)), flush=True)
        return 0
    for name in args.steps.split(","):
        if name not in STEPS:
            ap.error(f"unknown step {name!r}")
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--context", str(args.context), "--batch", str(args.batch),
               "--chunk-size", str(args.chunk_size), "--layers", str(args.layers), "--iters", str(args.iters)]
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
