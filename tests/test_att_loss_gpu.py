"""The kernels backend of the attention loss (transformer/attn_train.py) on the GPU: packed rows under autograd through
pafc_mha_rows_lse / pafc_mha_rows_bwd / pafc_lsm_loss_rows(_bwd) and the training GEMMs, under bf16 autocast, against the
float64 restatement of tests/att_loss_ref.py.

Bound: loss and every compared gradient are within 4 x the error of the FRAMEWORK backend under bf16 autocast on the CPU for the
same case -- the padded modules as the reference runs them, in the precision the kernels run in.  Errors are max |diff| against
float64, per case and quantity."""
import pytest
import torch

from tests import att_loss_ref as REF
from tests import attn_rescore_cases as C
from tests import parity_log

pytestmark = pytest.mark.gpu

D = 128
GRADS = ("embed.0.weight", "decoders.0.src_attn.linear_k.weight", "decoders.0.norm2.weight", "output_layer.weight")


def _model(V, dropout=0.0, seed=7, normalize_before=True):
    """float32 ASRModel around a seeded BiTransformerDecoder: d = 128, 2 heads, 256 units, 1 + 1 blocks (the recipe of
    tests/attn_rescore_cases.model for another vocabulary)."""
    from paper_accurate_fast_cheap_amd.transformer.asr_model import ASRModel
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    from paper_accurate_fast_cheap_amd.transformer.decoder import BiTransformerDecoder
    torch.manual_seed(seed)
    dec = BiTransformerDecoder(V, D, attention_heads=2, linear_units=256, num_blocks=1, r_num_blocks=1, dropout_rate=dropout,
                               positional_dropout_rate=dropout, normalize_before=normalize_before)
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if "norm" in name:
                p.add_(torch.randn_like(p) * 0.1)
            elif name.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.05)
    return ASRModel(V, torch.nn.Identity(), CTC(V, D), decoder=dec, lsm_weight=0.1)


def _case(which):
    g = torch.Generator().manual_seed(41 if which == "A" else 43)
    if which == "A":
        V, text_lens, mem_lens = 53, [0, 1, 17, 40], [1, 5, 17, 40]
    else:                                                  # more than 256 rows: the training GEMMs take every projection
        V, text_lens, mem_lens = 56, [40, 38, 41, 45, 39, 40, 42, 37], [40] * 8
    B = len(text_lens)
    enc = torch.randn(B, 40, D, generator=g, dtype=torch.float64)
    texts = [[int(v) for v in torch.randint(1, V - 1, (n,), generator=g)] for n in text_lens]
    text = torch.full((B, max(text_lens)), -1, dtype=torch.int64)
    for b, t in enumerate(texts):
        text[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
    mask = (torch.arange(40)[None, :] < torch.tensor(mem_lens)[:, None]).unsqueeze(1)
    return V, enc, mask, texts, text, torch.tensor(text_lens), mem_lens


def _run(model, enc, mask, text, lens, backend, device):
    from paper_accurate_fast_cheap_amd.transformer.attn_train import att_loss
    model = model.to(device)
    model.zero_grad(set_to_none=True)
    x = enc.float().to(device).requires_grad_(True)
    with torch.autocast(device, dtype=torch.bfloat16):
        loss, acc = att_loss(model, x, mask.to(device), text.to(device), lens, backend=backend)
    loss.backward()
    left = dict(model.decoder.left_decoder.named_parameters())
    out = {"loss": loss.detach().double().cpu().reshape(1), "encoder_out": x.grad.double().cpu()}
    out.update({n: left[n].grad.double().cpu() for n in GRADS})
    return out, float(acc)


@pytest.fixture(scope="module")
def references():
    """Per (case, reverse_weight): the float64 restatement and the CPU bf16-autocast framework run, computed once."""
    refs = {}
    for which in ("A", "B"):
        V, enc, mask, texts, text, lens, mem_lens = _case(which)
        for rw in (0.0, 0.3):
            model = _model(V)
            model.reverse_weight = rw
            sd = {k: v.detach().double().requires_grad_(True) for k, v in model.decoder.state_dict().items()}
            x = enc.clone().requires_grad_(True)
            loss, acc = REF.att_loss(sd, C.ref_conf(True), x, mem_lens, texts, model.sos, model.eos, rw, 0.1, False)
            loss.backward()
            want = {"loss": loss.detach().reshape(1), "encoder_out": x.grad}
            want.update({n: sd["left_decoder." + n].grad for n in GRADS})
            cpu, cpu_acc = _run(model, enc, mask, text, lens, "framework", "cpu")
            refs[(which, rw)] = (want, acc, cpu)
    return refs


@pytest.mark.parametrize("reverse_weight", [0.0, 0.3])
@pytest.mark.parametrize("which", ["A", "B"])
def test_kernels_backend_against_the_float64_restatement(hip, references, which, reverse_weight):
    V, enc, mask, texts, text, lens, mem_lens = _case(which)
    want, want_acc, cpu = references[(which, reverse_weight)]
    model = _model(V)
    model.reverse_weight = reverse_weight
    got, acc = _run(model, enc, mask, text, lens, "kernels", "cuda")
    again, _ = _run(model, enc, mask, text, lens, "kernels", "cuda")
    assert acc == pytest.approx(want_acc, abs=1e-6)                                       # th_accuracy
    for b, n in enumerate(mem_lens):
        assert (got["encoder_out"][b, n:] == 0).all()                                     # padded memory rows: exactly zero
    failures = []
    for key in want:
        assert torch.isfinite(got[key]).all(), key
        assert torch.equal(got[key], again[key]), key                                     # two backward passes: the same bits
        ek, ec = (got[key] - want[key]).abs().max().item(), (cpu[key] - want[key]).abs().max().item()
        print(f"att_loss case {which} rw={reverse_weight} {key}: max|err| kernels {ek:.3e}, cpu bf16 framework {ec:.3e}, "
              f"ratio {ek / ec:.2f}")
        parity_log.record(f"att_loss_kernels_case{which}_rw{reverse_weight}_{key}", max_abs_err=ek, cpu_yardstick_err=ec)
        if not (ec > 0 and ek <= 4 * ec):
            failures.append((key, ek, ec))
    assert not failures, failures


def test_post_norm_decoder_on_the_kernels_backend(hip):
    """normalize_before: false (case A, reverse_weight 0.3): loss and encoder_out gradient under the same bound."""
    V, enc, mask, texts, text, lens, mem_lens = _case("A")
    model = _model(V, normalize_before=False)
    model.reverse_weight = 0.3
    sd = {k: v.detach().double() for k, v in model.decoder.state_dict().items()}
    x = enc.clone().requires_grad_(True)
    loss, want_acc = REF.att_loss(sd, C.ref_conf(False), x, mem_lens, texts, model.sos, model.eos, 0.3, 0.1, False)
    loss.backward()
    want = {"loss": loss.detach().reshape(1), "encoder_out": x.grad}
    cpu, _ = _run(model, enc, mask, text, lens, "framework", "cpu")
    got, acc = _run(model, enc, mask, text, lens, "kernels", "cuda")
    assert acc == pytest.approx(want_acc, abs=1e-6)
    for key in want:
        ek, ec = (got[key] - want[key]).abs().max().item(), (cpu[key] - want[key]).abs().max().item()
        print(f"att_loss post-norm case A rw=0.3 {key}: max|err| kernels {ek:.3e}, cpu bf16 framework {ec:.3e}, ratio {ek / ec:.2f}")
        parity_log.record(f"att_loss_kernels_postnorm_caseA_{key}", max_abs_err=ek, cpu_yardstick_err=ec)
        assert torch.isfinite(got[key]).all() and ec > 0 and ek <= 4 * ec, (key, ek, ec)


def test_case_b_runs_the_new_kernels_and_no_library_gemm(hip):
    from torch.profiler import ProfilerActivity, profile
    V, enc, mask, texts, text, lens, mem_lens = _case("B")
    model = _model(V)
    model.reverse_weight = 0.3
    _run(model, enc, mask, text, lens, "kernels", "cuda")                                 # (first use: library handles, caches)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _run(model, enc, mask, text, lens, "kernels", "cuda")
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    for kernel in ("mha_rows_kernel", "mha_rows_bwd_dq_kernel", "mha_rows_bwd_dkv_kernel", "lsm_loss_kernel", "lsm_loss_bwd_kernel"):
        assert any(kernel in n for n in names), (kernel, names)
    bad = [n for n in names if "Cijk_" in n or ("gemm" in n.lower() and "at::native" in n)
           or n in ("aten::mm", "aten::addmm", "aten::bmm", "aten::linear", "aten::matmul")]
    assert not bad, bad


def test_dropout_in_train_mode_changes_the_loss(hip):
    V, enc, mask, texts, text, lens, mem_lens = _case("A")
    plain, _ = _run(_model(V).train(), enc, mask, text, lens, "kernels", "cuda")
    torch.manual_seed(5)
    dropped, _ = _run(_model(V, dropout=0.1).train(), enc, mask, text, lens, "kernels", "cuda")
    assert torch.isfinite(dropped["loss"]).all() and torch.isfinite(dropped["encoder_out"]).all()
    assert dropped["loss"].item() != plain["loss"].item()


def test_kernels_backend_names_what_is_unmet(hip):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.transformer.attn_train import att_loss, att_loss_unmet
    V, enc, mask, texts, text, lens, mem_lens = _case("A")
    model = _model(V).cuda()
    x = enc.float().cuda()
    assert "bf16" in att_loss_unmet(model, x)                                             # no autocast, an fp32 module
    with pytest.raises(PafcError, match="bf16 autocast"):
        att_loss(model, x, mask.cuda(), text, lens, backend="kernels")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert att_loss_unmet(model, x) is None
        model.decoder.left_decoder.decoders[0].self_attn.dropout.p = 0.1
        assert "dropout" in att_loss_unmet(model, x)
        loss, _ = att_loss(model, x, mask.cuda(), text, lens)                             # backend None: the framework takes it
        assert torch.isfinite(loss)


class _LinearEncoder(torch.nn.Module):
    def __init__(self, idim, d):
        super().__init__()
        self.proj = torch.nn.Linear(idim, d)

    def output_size(self):
        return self.proj.out_features

    def forward(self, x, lens, *a, **k):
        mask = (torch.arange(x.shape[1], device=lens.device)[None, :] < lens[:, None]).unsqueeze(1)
        return self.proj(x), mask


def test_transducer_forward_trains_the_decoder_on_the_gpu(hip):
    """Transducer.forward at the YAMLs' weights (0.3 rnnt + 0.2 ctc + 0.5 attention, reverse_weight 0.3, lsm_weight 0.1): a
    finite loss_att from the kernels backend enters loss with weight 0.5, and the gradient reaches the encoder."""
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer import attn_train
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    V = 56
    torch.manual_seed(2)
    model = Transducer(V, 0, _LinearEncoder(16, D), RNNPredictor(V, 32, 48, 0.0, 48, 1, dropout=0.0), TransducerJoint(V, D, 48, 64),
                       ctc=CTC(V, D), attention_decoder=_model(V).decoder, ctc_weight=0.2, transducer_weight=0.3,
                       attention_weight=0.5, reverse_weight=0.3, lsm_weight=0.1).cuda().train()
    g = torch.Generator().manual_seed(3)
    batch = {"feats": torch.randn(3, 20, 16, generator=g), "feats_lengths": torch.tensor([20, 13, 6]),
             "target": torch.randint(1, V - 1, (3, 5), generator=g), "target_lengths": torch.tensor([5, 3, 0])}
    batch["target"][1, 3:] = -1
    batch["target"][2, :] = -1
    with torch.autocast("cuda", dtype=torch.bfloat16):
        enc_out, _ = model.encoder(batch["feats"].cuda(), batch["feats_lengths"].cuda())
        assert attn_train.att_loss_unmet(model, enc_out) is None                           # forward will take the kernels
        out = model(batch, torch.device("cuda"))
    assert torch.isfinite(out["loss_att"]) and out["loss_att"] > 0 and 0 <= float(out["th_accuracy"]) <= 1
    want = 0.3 * out["loss_rnnt"] + 0.2 * out["loss_ctc"].sum() + 0.5 * out["loss_att"]
    assert torch.allclose(out["loss"].float(), want.float(), rtol=1e-5)
    (0.5 * out["loss_att"]).backward()
    assert model.encoder.proj.weight.grad is not None and model.encoder.proj.weight.grad.abs().max() > 0
    assert torch.isfinite(model.encoder.proj.weight.grad).all()
    assert model.decoder.right_decoder.output_layer.weight.grad.abs().max() > 0
