"""pafc_lsm_loss_rows and pafc_lsm_loss_rows_bwd (include/pafc_attention.h) against float64 on the GPU.

Loss, lse and dlogits are held against float64 of what the kernel reads (fp32 logits: the values; bf16 logits: the rounded
values), at 4 x the error of the same formula in float32 on the CPU -- the reference's KL sum over the log-softmax for the
loss, logsumexp for lse, autograd through the float32 loss for dlogits.  A case whose yardstick rounds to zero joins the next
one, as in tests/test_mha_rows_gpu.py.  For bf16 logits dlogits is written in the logits' dtype, so there the float32 CPU
yardstick is rounded to bf16 as well: no bf16 result can be held to the error of a float32 one.  `correct` is exact."""
import pytest
import torch

from tests import parity_log
from tests.att_loss_ref import lsm_rows

pytestmark = pytest.mark.gpu


def _case(V, rows, g):
    x = torch.randn(rows, V, generator=g, dtype=torch.float64) * 3
    x[rows // 2, V // 3] = 80.0                                           # a row with one logit of 80
    t = torch.randint(0, V, (rows,), generator=g)
    t[0] = 0 if rows == 1 and V == 53 else V - 1                          # the first and the last column
    if rows > 1:
        t[1], t[2], t[rows // 2] = 0, V - 1, V // 3
        t[3], t[rows - 1] = -1, -1                                        # ignored rows
        x[5, 7] = x[5, 11] = x[5].max() + 1.0                             # an argmax tie: the lowest index wins
        t[5] = 7
        x[6, 7] = x[6, 11] = x[6].max() + 1.0
        t[6] = 11                                                         # ... so this row is NOT correct
    return x, t


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_lsm_loss_rows_against_float64(hip, smoothing):
    from paper_accurate_fast_cheap_amd import hip_ops
    g = torch.Generator().manual_seed(11)
    pending = {"loss": [], "lse": [], "dlogits": []}
    gscale = 0.37
    for V in (53, 5000):
        for rows in (1, 67):
            x, t = _case(V, rows, g)
            t32 = t.to(torch.int32).cuda()
            xb = x.to(torch.bfloat16)
            for tag, x64, dt in (("fp32", x, torch.float32), ("bf16", xb.double(), torch.bfloat16)):
                pitch = V + (3 if dt == torch.float32 else 11)
                buf = torch.full((rows, pitch), float("nan"), dtype=dt, device="cuda")          # a row pitch wider than V
                buf[:, :V] = x64.to(dt)
                xw = x64.clone().requires_grad_(True)
                want = lsm_rows(xw, t, smoothing)
                (want["loss"].sum() * gscale).backward()
                xc = x64.float().requires_grad_(True)
                cpu = lsm_rows(xc, t, smoothing)
                (cpu["loss"].sum() * gscale).backward()
                loss, lse, correct = hip_ops.lsm_loss_rows(buf[:, :V], t32, smoothing)
                gdev = torch.tensor([gscale], dtype=torch.float32, device="cuda")
                dbuf = torch.full((rows, pitch), float("nan"), dtype=dt, device="cuda")
                dl = hip_ops.lsm_loss_rows_bwd(buf[:, :V], t32, smoothing, lse, gdev, out=dbuf[:, :V], pad_to=pitch)
                torch.cuda.synchronize()
                assert torch.equal(correct.cpu().bool(), want["correct"]), (V, rows, tag)
                assert (dbuf[:, V:] == 0).all()                                                  # the padding columns
                ignored = t == -1
                assert (loss.cpu()[ignored] == 0).all() and (dl.cpu()[ignored] == 0).all()
                got = {"loss": loss.double().cpu(), "lse": lse.double().cpu(), "dlogits": dl.double().cpu()}
                ref = {"loss": want["loss"].detach(), "lse": want["lse"].detach(), "dlogits": xw.grad}
                yard = {"loss": cpu["loss"].detach().double(), "lse": cpu["lse"].detach().double(), "dlogits": xc.grad.to(dt).double()}
                for key in pending:
                    assert torch.isfinite(got[key]).all(), (V, rows, tag, key)
                    ek, ec = (got[key] - ref[key]).abs().max().item(), (yard[key] - ref[key]).abs().max().item()
                    print(f"lsm_loss_rows V={V} rows={rows} {tag} s={smoothing} {key}: kernel {ek:.3e}, cpu yardstick {ec:.3e}")
                    parity_log.record(f"lsm_loss_rows_V{V}_rows{rows}_{tag}_s{smoothing}_{key}", max_abs_err=ek, cpu_yardstick_err=ec)
                    pending[key].append(ek)
                    if ec > 0:
                        assert max(pending[key]) <= 4 * ec, (V, rows, tag, key, pending[key], ec)
                        pending[key] = []
    assert not any(pending.values()), pending


def test_lsm_loss_rows_in_place_and_bad_targets(hip):
    from paper_accurate_fast_cheap_amd import hip_ops
    x = torch.randn(4, 53, device="cuda")
    t = torch.tensor([3, 53, -2, -1], dtype=torch.int32, device="cuda")                 # in range, two out of range, ignored
    loss, lse, correct = hip_ops.lsm_loss_rows(x, t, 0.1)
    assert torch.isfinite(loss[0]) and torch.isnan(loss[1]) and torch.isnan(loss[2]) and loss[3] == 0
    assert correct[1:].sum() == 0 and torch.isfinite(lse).all()
    gdev = torch.ones(1, device="cuda")
    fresh = hip_ops.lsm_loss_rows_bwd(x, t, 0.1, lse, gdev).clone()
    buf = torch.zeros(4, 64, device="cuda")
    buf[:, :53] = x
    hip_ops.lsm_loss_rows_bwd(buf[:, :53], t, 0.1, lse, gdev, out=buf[:, :53], pad_to=64)            # over the logits
    assert torch.equal(buf[0, :53], fresh[0]) and (buf[:, 53:] == 0).all() and (buf[3] == 0).all()
    assert torch.isnan(buf[1, :53]).all() and torch.isnan(buf[2, :53]).all() and torch.isfinite(buf[0]).all()
