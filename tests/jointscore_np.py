"""SRGR and L1 diversity restated in numpy (include/emogest.h, "Joint-space scores of whole tracks"), independent of
emotiongestures_amd.jointscore: fp32 subtractions with numpy float32 (one IEEE subtraction each), float64 additions of the widened absolute
values in the stated order, and math.fsum -- the exactly rounded sum -- wherever the library adds in a fixed order of its own.

The bounds, with u = 2^-53.  A float64 sum of count terms in any fixed order is within (count - 1) * u * sum |term| of the exact sum, to first
order; the scale, the division and fsum's own rounding add a few u on either side (the 8).
  srgr    the terms w[t] * c[t] are exact, of either sign:  |got - want| <= (n + 8) * u * sum_t |w[t]| c[t] * |scale| / (n J)
  mean    |got - want| <= (n + 8) * u * sum_t |x[t, c]| / n   per column
  l1_sum  n D terms |x - m|, each moved by the error of the mean it was taken from: with S = sum |x - m| and A = sum |x| over the row,
          |got - want| <= u * ((n D + 8) * S + 2 (n + 8) * A)   (a column's mean error, at most (n + 8) u * sum_t |x| / n, enters n terms)"""
import math

import numpy as np

U53 = 2.0 ** -53


def distance(r, g):
    """r, g [n, J, 3] float32 -> d [n, J] float64: (|rx - gx| + |ry - gy|) + |rz - gz|."""
    diff = np.asarray(r, np.float32) - np.asarray(g, np.float32)
    assert diff.dtype == np.float32
    a = np.abs(diff).astype(np.float64)
    return (a[..., 0] + a[..., 1]) + a[..., 2]


def srgr(r, g, w, frames, draws, threshold, scale):
    """r [rows, T, J, 3], g [rows / draws, T, J, 3], w [rows / draws, T] or None, frames [rows] -> hits [rows, J] int64, want [rows] (from
    the exactly rounded sum), bound [rows], recall [rows]."""
    rows, _T, J, _ = r.shape
    hits, want, bound, recall = np.zeros((rows, J), np.int64), np.zeros(rows), np.zeros(rows), np.zeros(rows)
    for b, n in enumerate(frames):
        u = b // draws
        hit = distance(r[b, :n], g[u, :n]) < threshold
        hits[b] = hit.sum(0)
        c = hit.sum(1).astype(np.float64)
        wt = np.ones(n) if w is None else np.asarray(w[u, :n], np.float32).astype(np.float64)
        terms = (wt * c).tolist()                                             # exact: 24 x 7 bits
        cells = float(n) * float(J)
        want[b] = math.fsum(terms) * scale / cells
        bound[b] = (n + 8) * U53 * math.fsum(abs(v) for v in terms) * abs(scale) / cells
        recall[b] = float(hits[b].sum()) / cells
    return hits, want, bound, recall


def l1div(x, frames):
    """x [rows, T, D] float32, frames [rows] -> mean [rows, D], mean_bound [rows, D], l1_sum [rows], l1_bound [rows]."""
    rows, _T, D = x.shape
    mean, mean_bound, l1, l1_bound = np.zeros((rows, D)), np.zeros((rows, D)), np.zeros(rows), np.zeros(rows)
    for b, n in enumerate(frames):
        v = np.asarray(x[b, :n], np.float32).astype(np.float64)
        for c in range(D):
            col = v[:, c].tolist()
            mean[b, c] = math.fsum(col) / n
            mean_bound[b, c] = (n + 8) * U53 * math.fsum(abs(e) for e in col) / n
        S = math.fsum(np.abs(v - mean[b]).reshape(-1).tolist())
        A = math.fsum(np.abs(v).reshape(-1).tolist())
        l1[b] = S
        l1_bound[b] = U53 * ((n * D + 8) * S + 2 * (n + 8) * A)
    return mean, mean_bound, l1, l1_bound
