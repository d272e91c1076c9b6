"""The resampler's definition in float64 numpy (test infrastructure; the product does not import it).

torchaudio's sinc_interp_hann resampler with lowpass_filter_width L = 6 and rolloff 0.99, restated from its definition --
torchaudio itself is not available to the tests, so parity with its code is not pinned here.  With g = gcd(f_in, f_out),
orig = f_in / g, new = f_out / g:  base = min(orig, new) * rolloff,  W = ceil(L orig / base),  `new` phases of 2 W + orig taps,
  t = clamp((-i / new + (j - W) / orig) base, -L, L),   k[i][j] = (t == 0 ? 1 : sin(pi t) / (pi t)) cos^2(pi t / (2 L)) base / orig,
and with x zero outside [0, S):  y[m new + i] = sum_j k[i][j] x[m orig - W + j]  for 0 <= m new + i < N = ceil(new S / orig)."""
import math

import numpy as np

L = 6
ROLLOFF = 0.99
# the rates the tests walk, all to 16 kHz: rate -> (orig, new, W, taps per phase, longest run of non-zero float32 taps)
RATES = {8000: (1, 2, 7, 15, 13), 11025: (441, 640, 7, 455, 13), 22050: (441, 320, 9, 459, 17), 24000: (3, 2, 10, 23, 19),
         32000: (2, 1, 13, 28, 25), 44100: (441, 160, 17, 475, 34), 48000: (3, 1, 19, 41, 37), 96000: (6, 1, 37, 80, 73)}


def ratio(f_in, f_out):
    g = math.gcd(int(f_in), int(f_out))
    return int(f_in) // g, int(f_out) // g


def width(orig, new):
    return int(math.ceil(L * orig / (min(orig, new) * ROLLOFF)))


def dense_table(orig, new):
    """(new, 2 W + orig) float64."""
    base = min(orig, new) * ROLLOFF
    W = width(orig, new)
    i = np.arange(new, dtype=np.float64)[:, None]
    j = np.arange(2 * W + orig, dtype=np.float64)[None, :]
    t = np.clip((-i / new + (j - W) / orig) * base, -L, L)
    pt = np.pi * t
    sinc = np.where(t == 0, 1.0, np.sin(pt) / np.where(t == 0, 1.0, pt))
    return sinc * np.cos(pt / (2 * L)) ** 2 * (base / orig)


def num_out(S, orig, new):
    return -((-new * S) // orig) if S > 0 else 0


def windows(x, orig, new):
    """(frames, 2 W + orig) float64: row m = x[m orig - W : m orig + W + orig], zero outside x; frames = ceil(N / new)."""
    W = width(orig, new)
    S = len(x)
    frames = -(-num_out(S, orig, new) // new)
    pad = np.zeros(W + frames * orig + W + orig, dtype=np.float64)
    pad[W:W + S] = x
    idx = np.arange(frames)[:, None] * orig + np.arange(2 * W + orig)[None, :]
    return pad[idx]


def resample(x, orig, new, table=None):
    """y (N) float64 = the dense sum of x (S) with `table` (default: the float64 dense table)."""
    k = dense_table(orig, new) if table is None else np.asarray(table, dtype=np.float64)
    N = num_out(len(x), orig, new)
    if N == 0:
        return np.zeros(0)
    return (windows(np.asarray(x, dtype=np.float64), orig, new) @ k.T).reshape(-1)[:N]


def abs_sum(x, orig, new, table):
    """(N) float64: sum_j |k[i][j] x[.]| per output, the scale of the fma chain's error bound."""
    N = num_out(len(x), orig, new)
    if N == 0:
        return np.zeros(0)
    return (np.abs(windows(np.asarray(x, dtype=np.float64), orig, new)) @ np.abs(np.asarray(table, dtype=np.float64)).T).reshape(-1)[:N]
