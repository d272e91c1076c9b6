"""Capture the forced-alignment goldens from the reference's own code.

Run ONCE where the reference tree is available:
    python tests/golden/make_goldens_force_align.py
It imports the reference through oracle/ref_shim.py and runs, on CPU, its `force_align`, `gen_ctc_peak_time` and
`gen_timestamps_from_peak` (wenet/utils/ctc_utils.py) on small synthetic utterances.  force_align.pt holds data only:
  * cases: per case the log-probabilities lp (T, V) float32, the labels y, the blank id, the reference's frame-level
    alignment, its peaks and its (start, end) stamps for the frame periods of PERIODS (max_duration = T x period);
  * wrap: one case the reference gets WRONG, with its output as the record: for state 0 it reads log_alpha[t-1, -1], the last
    state, so its path can jump from the final blank back to the first one and emit the labels twice.  Its alignment does not
    collapse to y; the package's must.
A case is kept only when the reference's alignment collapses to y, and at least 20 must be: a fixture that pins nothing cannot
be written.  Constructions: "speech" -- a +6 logit bump on label i in one frame of its own, evenly spaced, a +3 blank bias,
unit noise, log-softmax; T from 8 to 40, L from 1 to the most that fits (L + adjacent repeats = T), repeated labels; "q" --
the log-probabilities rounded to multiples of 0.25, so that exact ties are frequent; "inf" -- -inf on label and blank entries
away from the bumps; "rand" -- no bumps at all, quantised: where the wrap shows.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

PERIODS = (0.04, 0.08)
#        T   L  V  repeats  kind          blank
SPEC = [(40, 6, 8, 0, "speech", 0), (40, 6, 8, 0, "speech q", 0), (40, 6, 8, 0, "speech q inf", 0), (40, 6, 8, 2, "speech q", 0),
        (8, 1, 5, 0, "speech", 0), (8, 4, 6, 0, "speech q", 0), (8, 8, 10, 0, "speech q", 0), (9, 6, 7, 3, "speech q", 0),
        (12, 3, 5, 1, "speech q inf", 0), (16, 8, 9, 0, "speech q", 8), (16, 5, 7, 2, "speech inf", 0), (20, 10, 12, 0, "speech", 0),
        (20, 20, 24, 0, "speech q", 0), (24, 7, 9, 3, "speech q inf", 0), (24, 12, 6, 0, "speech q", 5), (28, 4, 6, 1, "speech q", 0),
        (32, 16, 10, 4, "speech q", 0), (32, 9, 11, 0, "speech inf", 0), (36, 12, 8, 2, "speech q inf", 7), (40, 20, 12, 0, "speech q", 0),
        (40, 30, 9, 5, "speech q", 0), (40, 13, 10, 3, "speech q inf", 0), (13, 5, 6, 0, "rand", 0), (17, 4, 5, 1, "rand", 0),
        (23, 6, 6, 0, "rand inf", 0), (11, 3, 4, 0, "rand", 0), (19, 8, 7, 2, "rand", 0), (15, 2, 5, 0, "rand inf", 0),
        (21, 7, 6, 1, "rand", 0), (9, 2, 4, 0, "rand", 0), (27, 5, 5, 0, "rand", 0), (14, 6, 6, 0, "rand inf", 0)]


def labels(g, L, V, repeats, blank):
    toks = [v for v in range(V) if v != blank]
    y = []
    for i in range(L):
        if i > 0 and i <= repeats:
            y.append(y[-1])
        else:
            pick = [v for v in toks if not y or v != y[-1]]
            y.append(pick[int(torch.randint(0, len(pick), (1,), generator=g))])
    return y


def make_case(g, T, L, V, repeats, kind, blank):
    y = labels(g, L, V, repeats, blank)
    need = L + sum(1 for i in range(1, L) if y[i] == y[i - 1])
    assert need <= T, (T, L, repeats)
    if "speech" in kind:
        logits = torch.randn(T, V, generator=g)
        logits[:, blank] += 3.0
        # one frame per label, a blank frame between adjacent equal labels, spread evenly over T
        slots, pos = [], 0
        for i in range(L):
            if i > 0 and y[i] == y[i - 1]:
                pos += 1
            slots.append(pos)
            pos += 1
        centres = [int((s + 0.5) * T / need) if need < T else s for s in slots]
        for i, c in enumerate(centres):
            logits[c, y[i]] += 6.0
        lp = logits.log_softmax(-1)
    else:
        lp = -(torch.randint(0, 6, (T, V), generator=g).float() * 0.25)
        centres = None
    if "q" in kind.split() or "rand" in kind:
        lp = torch.round(lp * 4) / 4
    if "inf" in kind:
        kill = torch.rand(T, V, generator=g) < 0.15
        if centres is not None:            # keep the bumps' neighbourhood alive: the -inf lie off the true path
            for i, c in enumerate(centres):
                kill[max(0, c - 1):c + 2, y[i]] = False
                kill[max(0, c - 1):c + 2, blank] = False
        lp = lp.masked_fill(kill, -float("inf"))
    return lp.contiguous(), y


def main():
    from oracle import ref_shim
    ref_shim.install()
    from wenet.utils import ctc_utils as R

    g = torch.Generator().manual_seed(20)
    kept, wrap = [], None
    for T, L, V, repeats, kind, blank in SPEC:
        lp, y = make_case(g, T, L, V, repeats, kind, blank)
        ali = [int(v) for v in R.force_align(lp, torch.tensor(y, dtype=torch.long), blank)]
        case = dict(kind=kind, lp=lp, y=y, blank=blank, align=ali)
        if R.remove_duplicates_and_blank(ali, blank) != y:
            if wrap is None:
                wrap = case
            continue
        peaks = R.gen_ctc_peak_time(ali, blank)
        case["peaks"] = [int(p) for p in peaks]
        case["stamps"] = {p: [(float(a), float(b)) for a, b in R.gen_timestamps_from_peak(peaks, T * p, p, 1.0)] for p in PERIODS}
        kept.append(case)
    assert len(kept) >= 20, f"only {len(kept)} cases whose reference alignment collapses to the labels"
    assert wrap is not None, "no case shows the reference's wrap: add random quantised cases"
    out = os.path.join(HERE, "force_align.pt")
    torch.save(dict(cases=kept, wrap=wrap, periods=list(PERIODS)), out)
    print(f"{out}: {len(kept)} cases kept of {len(SPEC)}, wrap case T={wrap['lp'].shape[0]} L={len(wrap['y'])}, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
