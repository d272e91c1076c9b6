"""The yardstick of the CTC forced-alignment tests: the recursion of include/pafc_search.h (pafc_ctc_align) as a plain double
loop over (t, s) on numpy.float32 scalars, candidate order and tie rule spelt out.  Independent of the package."""
import numpy as np

NEG = np.float32(-np.inf)


def align_ref(lp, y, blank=0):
    """lp: (T, V) array-like of float32 log-probabilities (the utterance's own frames), y: its labels.
    -> (align [T], first [L], last [L], score (numpy.float32), ok)."""
    lp = np.asarray(lp, dtype=np.float32)
    T, V = lp.shape
    y = [int(c) for c in y]
    L = len(y)
    fail = ([-1] * T, [-1] * L, [-1] * L, NEG, 0)
    if T <= 0:
        return fail
    if any(c == blank or c < 0 or c >= V for c in y):
        return fail
    if L + sum(1 for i in range(1, L) if y[i] == y[i - 1]) > T:
        return fail
    S = 2 * L + 1
    ext = [blank if s % 2 == 0 else y[s // 2] for s in range(S)]
    alpha = [NEG] * S
    alpha[0] = lp[0, ext[0]]
    if S > 1:
        alpha[1] = lp[0, ext[1]]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        new = [NEG] * S
        for s in range(S):
            best, k = alpha[s], 0                                   # candidate 0: stay
            if s >= 1 and alpha[s - 1] > best:                      # candidate 1: strictly greater only
                best, k = alpha[s - 1], 1
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] and alpha[s - 2] > best:
                best, k = alpha[s - 2], 2
            new[s] = np.float32(best + lp[t, ext[s]])               # one fp32 add (-inf + x = -inf)
            back[t, s] = k
        alpha = new
    s = S - 1
    if S >= 2 and alpha[S - 2] > alpha[S - 1]:
        s = S - 2
    score = np.float32(alpha[s])
    if score == NEG:
        return fail
    align, first, last = [0] * T, [-1] * L, [-1] * L
    for t in range(T - 1, -1, -1):
        align[t] = ext[s]
        if s % 2 == 1:
            first[s // 2] = t                                       # the walk goes backwards: the last write is the first frame
            if last[s // 2] < 0:
                last[s // 2] = t
        s -= int(back[t, s])
    return align, first, last, score, 1
