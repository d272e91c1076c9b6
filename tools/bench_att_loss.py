"""The attention term of the training objective at the training batch: B = 32, transcripts L <= 160, memories T' <= 499, d = 512,
8 heads, 2048 units, 3 + 3 blocks, V = 5000, reverse_weight 0.3, lsm_weight 0.1, bf16 autocast over fp32 master weights.
att_loss(backend="kernels") next to backend="framework" on the same GPU: forward + backward ms, kernel launches
(torch.profiler), peak memory of one forward + backward, and for the kernels backend the share of pafc_mha_rows_bwd and of
the loss kernels in its kernel time.  Random weights and transcripts; prints one JSON line."""
import json
import time

import torch
from torch.profiler import ProfilerActivity, profile

from paper_accurate_fast_cheap_amd import hip_ops
from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
from paper_accurate_fast_cheap_amd.transformer.attn_train import att_loss
from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder

torch.manual_seed(777)
dev = "cuda"
B, T, D, V, Lmax, rw = 32, 499, 512, 5000, 160, 0.3
g = torch.Generator().manual_seed(1)
text_lens = torch.randint(40, Lmax + 1, (B,), generator=g)
text_lens[0] = Lmax
mem_lens = torch.randint(200, T + 1, (B,), generator=g)
mem_lens[0] = T
text = torch.full((B, Lmax), -1, dtype=torch.int64)
for b, n in enumerate(text_lens.tolist()):
    text[b, :n] = torch.randint(1, V - 1, (n,), generator=g)
text_dev = text.to(dev)
mask = (torch.arange(T)[None, :] < mem_lens[:, None]).unsqueeze(1).to(dev)
enc = (torch.randn(B, T, D, generator=g) * 0.5).to(dev)
decoder = BiTransformerDecoder(V, D, attention_heads=8, linear_units=2048, num_blocks=3, r_num_blocks=3, dropout_rate=0.1,
                               positional_dropout_rate=0.1)
model = ASRModel(V, torch.nn.Identity(), CTC(V, D), decoder=decoder, reverse_weight=rw, lsm_weight=0.1).to(dev).train()


def step(backend):
    model.zero_grad(set_to_none=True)
    x = enc.clone().requires_grad_(True)
    with hip_ops.train_shadows(), torch.autocast("cuda", dtype=torch.bfloat16):
        loss, acc = att_loss(model, x, mask, text_dev, text_lens, backend=backend)
    loss.backward()
    return loss


def timed(fn, n=5):
    fn(); fn(); torch.cuda.synchronize(); t0 = time.time()
    for _ in range(n): r = fn()
    torch.cuda.synchronize(); return (time.time() - t0) / n, r


def kernels_of(fn):
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.key, e.count, e.device_time_total) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]


def peak(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(); torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


out = {"workload": f"B={B}, L<={Lmax} ({int(text_lens.sum()) + B} packed rows), T'<={T} ({int(mem_lens.sum())} of {B * T} memory "
                   f"rows), d={D}, 8 heads, 3+3 blocks, V={V}, reverse_weight {rw}, bf16 autocast, train mode (dropout 0.1)"}
for backend in ("kernels", "framework"):
    dt, loss = timed(lambda: step(backend))
    ks = kernels_of(lambda: step(backend))
    out[f"{backend}_fwd_bwd_ms"] = round(dt * 1e3, 2)
    out[f"{backend}_launches"] = sum(c for _, c, _ in ks)
    out[f"{backend}_peak_bytes"] = peak(lambda: step(backend))
    out[f"{backend}_loss"] = round(float(loss.detach()), 4)
    if backend == "kernels":
        total = sum(t for _, _, t in ks)
        share = lambda *words: round(100.0 * sum(t for k, _, t in ks if any(w in k for w in words)) / total, 1)    # noqa: E731
        out["kernels_kernel_ms"] = round(total / 1e3, 2)
        out["share_mha_rows_bwd_pct"] = share("mha_rows_bwd")
        out["share_mha_rows_fwd_pct"] = share("mha_rows_kernel")
        out["share_lsm_loss_pct"] = share("lsm_loss")
print(json.dumps(out))
