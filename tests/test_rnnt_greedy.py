"""RNN-T greedy search (transducer/search/greedy_search.py, hip_ops.rnnt_greedy_search, csrc/rnnt_greedy.hip): checks that need no
GPU -- the reference's tokens on CPU tensors (golden rnnt_greedy_c5.pt, captured from the reference's basic_greedy_search), the
model-level entry points, the C boundary's symbols and argument validation, the compiled kernels, and the conditions the kernel
path refuses."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc", "rnnt_greedy.hip")
ERR_NULL, ERR_DIMS, ERR_WS, ERR_DTYPE, ERR_UNSUP, ERR_ALIGN = -1, -2, -4, -6, -7, -8
V, D = 50, 128


class _FixedEncoder(torch.nn.Module):
    """Returns the golden's encoder output for any input (the search is what is under test)."""

    def __init__(self, enc_out):
        super().__init__()
        self.register_buffer("enc_out", enc_out)

    def output_size(self):
        return self.enc_out.shape[-1]

    def forward(self, x, lens, *a, **k):
        mask = (torch.arange(self.enc_out.shape[1], device=lens.device)[None, :] < lens[:, None]).unsqueeze(1)
        return self.enc_out[:x.shape[0]].to(x.device), mask


def golden_model(g, device="cpu", dtype=torch.float32):
    """The golden's predictor and joint inside a Transducer whose encoder returns the golden's encoder output."""
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    from paper_accurate_fast_cheap_amd.transducer.predictor import RNNPredictor
    from paper_accurate_fast_cheap_amd.transducer.transducer import Transducer
    from paper_accurate_fast_cheap_amd.transformer.ctc import CTC
    pred = RNNPredictor(V, embed_size=64, output_size=64, embed_dropout=0.1, hidden_size=64, num_layers=2, bias=True,
                        rnn_type="lstm", dropout=0.1)
    pred.load_state_dict(g["pred_sd"])
    joint = TransducerJoint(V, enc_output_size=D, pred_output_size=64, join_dim=64, prejoin_linear=True,
                            postjoin_linear=False, joint_mode="add", activation="tanh")
    joint.load_state_dict(g["joint_sd"])
    torch.manual_seed(0)
    model = Transducer(V, g["blank"], _FixedEncoder(g["enc_out"]), pred, joint, ctc=CTC(V, D)).eval()
    return model.to(device=device, dtype=dtype)


@pytest.fixture(scope="module")
def golden():
    return load_golden("rnnt_greedy_c5")


@pytest.mark.parametrize("n_steps", [64, 2])
def test_basic_greedy_search_matches_reference_golden(golden, n_steps):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import basic_greedy_search
    model = golden_model(golden)
    enc, lens = golden["enc_out"], golden["enc_lens"]
    with torch.no_grad():
        got = [basic_greedy_search(model, enc[b:b + 1], lens[b], n_steps=n_steps)[0] for b in range(enc.shape[0])]
    assert got == golden["tokens"][n_steps]


@pytest.mark.parametrize("n_steps", [64, 2])
def test_transducer_greedy_search_and_decode_match_golden_on_cpu(golden, n_steps):
    model = golden_model(golden)
    speech, lens = torch.zeros(3, 37, 80), golden["enc_lens"]
    assert model.greedy_search(speech, lens, n_steps=n_steps) == golden["tokens"][n_steps]
    for b in range(3):                                  # the reference's own call shape, B = 1
        one = golden_model(golden)
        one.encoder.enc_out = golden["enc_out"][b:b + 1]
        assert one.greedy_search(speech[b:b + 1], lens[b:b + 1], n_steps=n_steps) == [golden["tokens"][n_steps][b]]
    if n_steps == 64:
        res = model.decode(["rnnt_greedy_search"], speech, lens)["rnnt_greedy_search"]
        assert [r.tokens for r in res] == golden["tokens"][64]
        for r, T in zip(res, lens.tolist()):
            assert len(r.times) == len(r.tokens) and all(0 <= t < T for t in r.times) and r.times == sorted(r.times)
            assert r.score < 0.0


def test_batched_cpu_call_equals_single_calls(golden):
    from paper_accurate_fast_cheap_amd.transducer.search.greedy_search import basic_greedy_search, batch_greedy_search
    model = golden_model(golden)
    enc, lens = golden["enc_out"], golden["enc_lens"]
    with torch.no_grad():
        batch = batch_greedy_search(model, enc, lens, n_steps=2)
        single = [batch_greedy_search(model, enc[b:b + 1], lens[b:b + 1], n_steps=2)[0] for b in range(3)]
        ref = [basic_greedy_search(model, enc[b:b + 1], lens[b], n_steps=2)[0] for b in range(3)]
    assert [r.tokens for r in batch] == [r.tokens for r in single] == ref
    assert [r.times for r in batch] == [r.times for r in single]
    assert [r.score for r in batch] == [r.score for r in single]


def test_decode_with_every_other_method_is_unchanged(golden):
    from paper_accurate_fast_cheap_amd.transformer.search import ctc_greedy_search, ctc_prefix_beam_search
    model = golden_model(golden)
    speech, lens = torch.zeros(3, 37, 80), golden["enc_lens"]
    with torch.no_grad():
        res = model.decode(["ctc_greedy_search", "ctc_prefix_beam_search", "rnnt_beam_search"], speech, lens, beam_size=4)
        assert "rnnt_greedy_search" not in res
        logp = model.ctc.log_softmax(golden["enc_out"])
        assert [r.tokens for r in res["ctc_greedy_search"]] == [r.tokens for r in ctc_greedy_search(logp, lens, 0)]
        assert ([r.tokens for r in res["ctc_prefix_beam_search"]]
                == [r.tokens for r in ctc_prefix_beam_search(logp, lens, 4, None, 0)])
        beam = model.beam_search_decode(golden["enc_out"], lens, logp, beam_size=4, ctc_weight=0.0, transducer_weight=0.0)
        assert [r.tokens for r in res["rnnt_beam_search"]] == [r.tokens for r in beam]
        with pytest.raises(NotImplementedError):
            model.decode(["attention"], speech, lens)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
class _Net(ctypes.Structure):
    _PP = ctypes.POINTER(ctypes.c_void_p)
    _fields_ = [("dtype", ctypes.c_int), ("num_layers", ctypes.c_int), ("embed_dim", ctypes.c_int), ("hidden", ctypes.c_int),
                ("pred_dim", ctypes.c_int), ("join_dim", ctypes.c_int), ("vocab", ctypes.c_int), ("embed_rows", ctypes.c_int),
                ("embed", ctypes.c_void_p), ("w_ih", _PP), ("w_hh", _PP), ("b_ih", _PP), ("b_hh", _PP),
                ("proj_w", ctypes.c_void_p), ("proj_b", ctypes.c_void_p), ("pred_ffn_w", ctypes.c_void_p),
                ("pred_ffn_b", ctypes.c_void_p), ("out_w", ctypes.c_void_p), ("out_b", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    from paper_accurate_fast_cheap_amd.csrc import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(build.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    so = build.build() if os.path.exists("/opt/rocm/bin/hipcc") else build.OUT
    L = ctypes.CDLL(so)
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.pafc_rnnt_greedy_workspace_bytes.restype = Z
    L.pafc_rnnt_greedy_workspace_bytes.argtypes = [P, I, I, I]
    L.pafc_rnnt_greedy_init.argtypes = [P, I, I, I, I, P, P, Z, P]
    L.pafc_rnnt_greedy_step.argtypes = [P, I, I, I, I, P, P, Z, P, P]
    L.pafc_rnnt_greedy_finish.argtypes = [P, I, I, I, P, Z, I, P, P, P, P, P, P]
    return L


_ONE = 256        # aligned, never dereferenced: validation fails first


def _net(layers=2, **kw):
    arr = (ctypes.c_void_p * layers)(*([_ONE] * layers))
    pp = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
    f = dict(dtype=0, num_layers=layers, embed_dim=640, hidden=640, pred_dim=640, join_dim=640, vocab=5000, embed_rows=5000,
             embed=_ONE, w_ih=pp, w_hh=pp, b_ih=pp, b_hh=pp, proj_w=_ONE, proj_b=_ONE, pred_ffn_w=_ONE, pred_ffn_b=_ONE,
             out_w=_ONE, out_b=_ONE)
    f.update(kw)
    n = _Net(**f)
    n._keep = arr
    return n


def test_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "pafc_search.h")).read()
    for name in ("pafc_rnnt_greedy_workspace_bytes", "pafc_rnnt_greedy_init", "pafc_rnnt_greedy_step",
                 "pafc_rnnt_greedy_finish"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
    assert "pafc_rnnt_greedy_net" in hdr
    assert "pafc_rnnt_greedy_init" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_workspace_size(lib):
    n = _net()
    ws = lib.pafc_rnnt_greedy_workspace_bytes(ctypes.byref(n), 8, 250, 64)
    assert ws >= 2 * 8 * 250 * 64 * 4 + 2 * 2 * 2 * 8 * 640 * 4      # tokens + frames, two slots of (h, c)
    assert lib.pafc_rnnt_greedy_workspace_bytes(ctypes.byref(n), 0, 250, 64) == 0
    assert lib.pafc_rnnt_greedy_workspace_bytes(ctypes.byref(n), 257, 250, 64) == 0
    assert lib.pafc_rnnt_greedy_workspace_bytes(ctypes.byref(n), 8, 250, 0) == 0
    assert lib.pafc_rnnt_greedy_workspace_bytes(None, 8, 250, 64) == 0


def test_entry_points_validate_before_touching_the_device(lib):
    NULL = None
    big = 1 << 40

    def step(net=None, B=8, T=250, n=64, blank=0, E=_ONE, ws=_ONE, nbytes=big):
        net = net if net is not None else _net()
        return lib.pafc_rnnt_greedy_step(ctypes.byref(net), B, T, n, blank, E, ws, nbytes, NULL, NULL)

    def init(net=None, B=8, lens=_ONE, ws=_ONE, nbytes=big, blank=0):
        net = net if net is not None else _net()
        return lib.pafc_rnnt_greedy_init(ctypes.byref(net), B, 250, 64, blank, lens, ws, nbytes, NULL)

    assert lib.pafc_rnnt_greedy_step(None, 8, 250, 64, 0, _ONE, _ONE, big, NULL, NULL) == ERR_NULL
    assert step(E=NULL) == ERR_NULL
    assert step(ws=NULL) == ERR_NULL
    assert step(net=_net(out_w=None)) == ERR_NULL
    assert step(net=_net(w_ih=None)) == ERR_NULL
    assert step(B=0) == ERR_DIMS
    assert step(B=257) == ERR_DIMS
    assert step(T=0) == ERR_DIMS
    assert step(n=0) == ERR_DIMS
    assert step(blank=5000) == ERR_DIMS
    assert step(blank=-1) == ERR_DIMS
    assert step(net=_net(num_layers=0)) == ERR_DIMS
    assert step(net=_net(embed_rows=4999)) == ERR_DIMS
    assert step(net=_net(dtype=2)) == ERR_DTYPE
    assert step(net=_net(hidden=642)) == ERR_UNSUP
    assert step(net=_net(join_dim=4096)) == ERR_UNSUP
    assert step(nbytes=1024) == ERR_WS
    assert step(E=_ONE + 4) == ERR_ALIGN
    assert step(ws=_ONE + 16) == ERR_ALIGN
    assert step(net=_net(out_w=_ONE + 8)) == ERR_ALIGN
    assert init(lens=NULL) == ERR_NULL
    assert init(B=-1) == ERR_DIMS
    assert init(nbytes=16) == ERR_WS
    n = _net()
    assert lib.pafc_rnnt_greedy_finish(ctypes.byref(n), 8, 250, 64, _ONE, big, 10, NULL, NULL, _ONE, NULL, NULL, NULL) == ERR_NULL
    assert lib.pafc_rnnt_greedy_finish(ctypes.byref(n), 8, 250, 64, _ONE, big, 0, _ONE, NULL, _ONE, NULL, NULL, NULL) == ERR_DIMS
    assert lib.pafc_rnnt_greedy_finish(ctypes.byref(n), 8, 250, 64, _ONE, 8, 10, _ONE, NULL, _ONE, NULL, NULL, NULL) == ERR_WS


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("asm") / "rnnt_greedy.s"
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.dirname(SRC), "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def test_kernels_neither_spill_nor_use_scratch(asm):
    names = set(re.findall(r"\n(_ZN4pafc[^\n:]*greedy_(\w+?)_kernel[^\n:]*):", asm))
    kinds = {k for _, k in names}
    assert {"init", "lstm", "matvec", "joint", "update", "finish"} <= kinds, kinds
    assert len([n for n, k in names if k == "lstm"]) == 4          # fp32 / bf16 x embedding layer / upper layers
    assert "scratch_" not in asm
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)
    assert spills and all(int(v) == 0 for v in spills)
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm) and \
        all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm))


def test_no_float_atomics_in_the_source():
    src = re.sub(r"//[^\n]*", "", open(SRC).read())
    assert "atomic" not in src.lower()


# ---- what the kernel path refuses ---------------------------------------------------------------------------------------------------
def _unmet(model, enc=None, n_steps=64):
    from paper_accurate_fast_cheap_amd import hip_ops
    enc = enc if enc is not None else torch.zeros(2, 5, D)
    return hip_ops.rnnt_greedy_unmet(model.predictor, model.joint, enc, n_steps)


def test_unmet_names_each_unsupported_configuration(golden):
    from paper_accurate_fast_cheap_amd.transducer.joint import TransducerJoint
    model = golden_model(golden)
    assert "not on the GPU" in _unmet(model)
    m = golden_model(golden)
    m.joint = TransducerJoint(V, D, 64, 64, postjoin_linear=True).eval()
    assert "post-join" in _unmet(m)
    m.joint = TransducerJoint(V, D, 64, 64, activation="relu").eval()
    assert "tanh" in _unmet(m)
    m.joint = TransducerJoint(V, 64, 64, 64, prejoin_linear=False, postjoin_linear=True).eval()
    assert "pre-join" in _unmet(m)
    m = golden_model(golden)
    m.joint.hat_joint = True
    assert "hat_joint" in _unmet(m)
    m = golden_model(golden)
    m.predictor.rnn = torch.nn.GRU(64, 64, 2, batch_first=True)
    assert "LSTM" in _unmet(m)
    m = golden_model(golden)
    m.predictor.train()
    assert "dropout" in _unmet(m)
    m = golden_model(golden)
    m.joint.ffn_out.to(torch.bfloat16)
    assert "all fp32 or all bf16" in _unmet(m)


def test_gpu_entry_raises_instead_of_falling_back(golden):
    from paper_accurate_fast_cheap_amd import hip_ops
    from paper_accurate_fast_cheap_amd._lib import PafcError
    model = golden_model(golden)
    model.joint.hat_joint = True
    with pytest.raises(PafcError, match="hat_joint"):
        hip_ops.rnnt_greedy_search(model.predictor, model.joint, golden["enc_out"], golden["enc_lens"])
