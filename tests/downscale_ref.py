"""Two restatements of bicubic decimation in the MATLAB imresize convention, for tests/test_downscale*.py (no test here).

(a) contributions / downscale_f64: the general imresize contribution algorithm in float64, written from the formula --
    per output index the centre u, the first candidate tap, P = 4 s + 2 candidates, weights c((u - j) / s) / s, normalised,
    indices through the symmetric map.
(b) derive_taps / downscale_exact: the same weights as Fractions, Python integers, one round-half-even on the exact
    rational.
"""
import math
from fractions import Fraction

import numpy as np


def cubic(x):
    """Keys cubic, a = -1/2 (float or Fraction)."""
    ax = abs(x)
    if ax <= 1:
        return (ax * ax * ax * 3) / 2 - (ax * ax * 5) / 2 + 1
    if ax < 2:
        return -(ax * ax * ax) / 2 + (ax * ax * 5) / 2 - 4 * ax + 2
    return ax * 0


def reflect(j, n):
    m = j % (2 * n)
    return m if m < n else 2 * n - 1 - m


# ---------------------------------------------------------------- (a) float64, general algorithm
def contributions(n_in, s):
    """-> (weights float64 [n_out][P], unreflected indices int [n_out][P]) of an axis of n_in = n_out s pixels."""
    n_out = n_in // s
    P = 4 * s + 2
    weights = np.zeros((n_out, P), np.float64)
    indices = np.zeros((n_out, P), np.int64)
    for i in range(n_out):
        u = (i + 0.5) * s - 0.5
        left = math.floor(u - 2 * s) + 1
        for p in range(P):
            j = left + p
            indices[i, p] = j
            weights[i, p] = cubic((u - j) / float(s)) / s
        weights[i] /= weights[i].sum()
    return weights, indices


def _matrix(n_in, s):
    w, idx = contributions(n_in, s)
    a = np.zeros((n_in // s, n_in), np.float64)
    for i in range(w.shape[0]):
        for p in range(w.shape[1]):
            a[i, reflect(int(idx[i, p]), n_in)] += w[i, p]
    return a


def downscale_f64(image, s):
    """uint8 (H, W, 3) -> float64 (H // s, W // s, 3), unrounded and unclipped."""
    h, w = image.shape[0] // s, image.shape[1] // s
    crop = image[:h * s, :w * s].astype(np.float64)
    rows, cols = _matrix(h * s, s), _matrix(w * s, s)
    return np.stack([rows @ crop[:, :, c] @ cols.T for c in range(3)], axis=2)


# ---------------------------------------------------------------- (b) exact
def derive_taps(s):
    """-> (D, first offset, integer numerators): the weights c((u - j) / s) / s of output 0's centre u = (s - 1) / 2 at
    offsets j, as Fractions over their common denominator, zero weights at both ends dropped."""
    u = Fraction(s - 1, 2)
    found = {j: cubic((u - j) / s) / s for j in range(-4 * s, 5 * s)}
    offsets = [j for j, w in found.items() if w != 0]
    first, last = min(offsets), max(offsets)
    ws = [found[j] for j in range(first, last + 1)]
    assert sum(ws) == 1
    D = 1
    for w in ws:
        D = D * w.denominator // math.gcd(D, w.denominator)
    return D, first, tuple(int(w * D) for w in ws)


def downscale_exact(image, s, clip=True):
    """uint8 (H, W, 3) -> (H // s, W // s, 3) int64: round_half_even of the exact rational double sum (Python's round on
    a Fraction), clipped to 0..255 unless clip is False."""
    D, first, taps = derive_taps(s)
    h, w = image.shape[0] // s, image.shape[1] // s
    H, W = h * s, w * s
    px = image[:H, :W].astype(np.int64).tolist()
    rows = [[(reflect(s * i + first + k, H), t) for k, t in enumerate(taps) if t] for i in range(h)]
    cols = [[(reflect(s * j + first + k, W), t) for k, t in enumerate(taps) if t] for j in range(w)]
    out = np.zeros((h, w, 3), np.int64)
    for i in range(h):
        for j in range(w):
            for c in range(3):
                n = sum(tr * tc * px[r][q][c] for r, tr in rows[i] for q, tc in cols[j])
                v = round(Fraction(n, D * D))
                out[i, j, c] = min(max(v, 0), 255) if clip else v
    return out
