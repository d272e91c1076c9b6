"""Capture the RNN-T greedy-search golden from the reference's own `basic_greedy_search`.

Run ONCE where the reference tree is available:
    python tests/golden/make_goldens_rnnt_greedy.py
It imports the reference through oracle/ref_shim.py, builds the search_c5 predictor and joint (synth weights from the specs and
seeds in search_c5.pt), ADJUSTS them as recorded below, runs the reference's basic_greedy_search per utterance on CPU for
n_steps = 64 and 2 and stores tokens, weights and inputs in rnnt_greedy_c5.pt.

Why the adjustments: with the raw synth weights the search is degenerate -- the predictor barely depends on its input, so a
frame either goes blank at once or repeats one token until the n_steps cap.  The fixture therefore wires two controls in:
  * the blank drive of a frame: encoder dimension 0 is projected by enc_ffn onto u = sign(ffn_out.weight[blank]) (times
    ENC_DRIVE), and enc_out[:, :, 0] is set per frame, uniform in [ENC_LO, ENC_HI) (seeded); utterance 2 gets EMPTY_DRIVE
    on every frame and emits nothing;
  * a blank push of the last emitted token: LSTM unit 0 of both layers is made memoryless (forget gate closed, input and
    output gates open, recurrent rows zero), layer 1's cell input reads unit 0 of layer 0 (times KAPPA), the projection's
    output 0 copies it and pred_ffn maps it onto u (times BETA) -- so after token y the blank logit moves by an amount
    that depends on y, and frames end in blank after 0, 1 or several symbols.
The script asserts that the fixture exercises every branch and that every decision's top-2 log-probability margin is at least
1e-3, so a different fp32 summation order cannot flip a golden token.  The reference source never leaves this container:
the fixture holds data only.
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import synth  # noqa: E402

V, D, H = 50, 128, 64
ENC_DRIVE, BETA, KAPPA = 1.0, 2.0, 3.0
ENC_LO, ENC_HI, ENC_SEED, EMPTY_DRIVE = -0.5, 2.0, 1, 6.0
N_STEPS = (64, 2)
MIN_MARGIN = 1e-3


def adjust(pred_sd, joint_sd):
    """The recorded adjustments, applied in place to the synth state dicts."""
    u = torch.sign(joint_sd["ffn_out.weight"][0])
    for l in (0, 1):
        wih, whh = pred_sd[f"rnn.weight_ih_l{l}"], pred_sd[f"rnn.weight_hh_l{l}"]
        bih, bhh = pred_sd[f"rnn.bias_ih_l{l}"], pred_sd[f"rnn.bias_hh_l{l}"]
        for gate, b in ((0, 10.0), (1, -10.0), (3, 10.0)):     # i open, f closed, o open: unit 0 forgets every step
            wih[gate * H] = 0.0
            bih[gate * H] = b
        for gate in range(4):
            whh[gate * H] = 0.0
            bhh[gate * H] = 0.0
        if l == 1:                                             # layer 1's unit 0 reads layer 0's unit 0
            wih[2 * H] = 0.0
            wih[2 * H, 0] = KAPPA
            bih[2 * H] = 0.0
    pred_sd["projection.weight"][0] = 0.0
    pred_sd["projection.weight"][0, 0] = 1.0
    pred_sd["projection.bias"][0] = 0.0
    joint_sd["pred_ffn.weight"][:, 0] = BETA * u
    joint_sd["enc_ffn.weight"][:, 0] = ENC_DRIVE * u


def encoder_rows(enc_out):
    enc = enc_out.clone()
    gen = torch.Generator().manual_seed(ENC_SEED)
    enc[:, :, 0] = torch.rand(enc.shape[:2], generator=gen) * (ENC_HI - ENC_LO) + ENC_LO
    enc[2, :, 0] = EMPTY_DRIVE
    return enc


def trace(model, enc, T, n_steps):
    """The decisions of the reference's loop, restated to record each frame's ending and each decision's top-2 margin."""
    cache = model.predictor.init_state(1, method="zero", device=enc.device)
    tok, t, k, need, ends, margins = torch.tensor([[model.blank]]), 0, 0, True, [], []
    while t < T:
        if need:
            po, nc = model.predictor.forward_step(tok, torch.zeros(1, 1), cache)
        lp = model.joint(enc[:, t:t + 1], po).log_softmax(-1).reshape(-1)
        top = lp.topk(2).values
        margins.append(float(top[0] - top[1]))
        y = int(lp.argmax())
        if y != model.blank:
            tok, cache, need, k = torch.tensor([[y]]), nc, True, k + 1
        if y == model.blank or k >= n_steps:
            ends.append(("blank", k) if y == model.blank else ("cap", k))
            need = need and y != model.blank
            t, k = t + 1, 0
    return ends, margins


def main():
    from oracle import ref_shim
    ref_shim.install()
    torch.set_grad_enabled(False)
    from wenet.transducer.joint import TransducerJoint
    from wenet.transducer.predictor import RNNPredictor
    from wenet.transducer.search.greedy_search import basic_greedy_search

    c5 = torch.load(os.path.join(HERE, "search_c5.pt"), weights_only=False)
    pred_sd = synth.synth_state_dict(c5["pred_spec"], c5["pred_seed"])
    joint_sd = synth.synth_state_dict(c5["joint_spec"], c5["joint_seed"])
    adjust(pred_sd, joint_sd)
    pred = RNNPredictor(V, embed_size=64, output_size=64, embed_dropout=0.1, hidden_size=H, num_layers=2, bias=True,
                        rnn_type="lstm", dropout=0.1).eval()
    pred.load_state_dict(pred_sd)
    joint = TransducerJoint(V, enc_output_size=D, pred_output_size=64, join_dim=64, prejoin_linear=True,
                            postjoin_linear=False, joint_mode="add", activation="tanh").eval()
    joint.load_state_dict(joint_sd)
    model = types.SimpleNamespace(predictor=pred, joint=joint, blank=0)
    enc, lens = encoder_rows(c5["enc_out"]), c5["enc_lens"]

    tokens, ends, margins = {}, {}, []
    for n in N_STEPS:
        tokens[n] = [basic_greedy_search(model, enc[b:b + 1], lens[b], n_steps=n)[0] for b in range(enc.shape[0])]
        ends[n] = []
        for b in range(enc.shape[0]):
            e, m = trace(model, enc[b:b + 1], int(lens[b]), n)
            ends[n] += e
            margins += m
    blank_after = [k for kind, k in ends[64] if kind == "blank"]
    assert 0 in blank_after and 1 in blank_after and any(k >= 2 for k in blank_after), blank_after
    assert any(kind == "cap" for kind, _ in ends[2]) and any(kind == "cap" for kind, _ in ends[64])
    assert any(len(t) == 0 for t in tokens[64]) and any(len(t) == 0 for t in tokens[2])
    assert all(len(t) > 0 for t in tokens[64][:2])
    assert min(margins) >= MIN_MARGIN, min(margins)

    path = os.path.join(HERE, "rnnt_greedy_c5.pt")
    torch.save(dict(pred_sd=pred_sd, joint_sd=joint_sd, enc_out=enc, enc_lens=lens, blank=0, tokens=tokens,
                    adjustments=dict(enc_drive=ENC_DRIVE, beta=BETA, kappa=KAPPA, enc_lo=ENC_LO, enc_hi=ENC_HI,
                                     enc_seed=ENC_SEED, empty_drive=EMPTY_DRIVE, unit=0),
                    source=dict(pred_spec=c5["pred_spec"], pred_seed=c5["pred_seed"], joint_spec=c5["joint_spec"],
                                joint_seed=c5["joint_seed"]),
                    min_margin=min(margins)), path)
    print(f"rnnt_greedy_c5: {os.path.getsize(path) / 1024:.1f} KiB; tokens per utterance",
          {n: [len(t) for t in tokens[n]] for n in N_STEPS}, "blank after", sorted(set(blank_after)),
          "min margin %.2e" % min(margins))


if __name__ == "__main__":
    main()
