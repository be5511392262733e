"""The motion statistics restated in numpy (include/emogest.h, "Motion statistics of whole tracks"), independent of emotiongestures_amd.kinematics:
fp32 differences with numpy float32 (one IEEE subtraction each), fp64 squares of the widened components, math.fsum -- the exactly rounded sum --
of the square roots, np.searchsorted(edges2, s2, side="right") - 1 for the bins.

The bound.  The terms sqrt(s2) are positive.  A float64 sum of count terms in any fixed order is within (count - 1) * u of the exact sum,
relatively, u = 2^-53; the square root and the two additions inside s2 are what else can round per term, and the scale, the division and
fsum's own rounding add a few u on either side: |got - want| <= (count + 8) * u * want."""
import math

import numpy as np

U53 = 2.0 ** -53


def edges2_of(edges, fps):
    q = np.asarray(edges, np.float64) / np.float64(fps)
    return q * q


def s2_of(p, n, k):
    """p [T, J, 3] float32, n valid frames -> s2_k [n - k, J] float64."""
    d = np.asarray(p, np.float32)[:n]
    for _ in range(k):
        d = d[1:] - d[:-1]
        assert d.dtype == np.float32
    w = d.astype(np.float64)
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


def stats(p, frames, edges2, fps):
    """p [rows, T, J, 3] float32, frames [rows] (each >= 4), edges2 [E] float64 -> mean [rows, 3, J] float64 (from the exactly rounded sums),
    count [rows, 3], hist [rows, J, E] int64 (the last column the overflow)."""
    rows, _T, J, _ = p.shape
    E = len(edges2)
    mean, count, hist = np.zeros((rows, 3, J)), np.zeros((rows, 3), np.int64), np.zeros((rows, J, E), np.int64)
    for b, n in enumerate(frames):
        for k in (1, 2, 3):
            s2 = s2_of(p[b], n, k)
            root = np.sqrt(s2)
            count[b, k - 1] = n - k
            for j in range(J):
                mean[b, k - 1, j] = math.fsum(root[:, j].tolist()) * float(fps) ** k / (n - k)
            if k == 1:
                pos = np.searchsorted(edges2, s2, side="right") - 1
                for j in range(J):
                    hist[b, j] = np.bincount(pos[:, j], minlength=E)
    return mean, count, hist


def within(got, want, count):
    """Every mean inside the bound: got, want [rows, 3, J], count [rows, 3] -> (ok, worst error / bound)."""
    bound = (count[:, :, None] + 8) * U53 * np.abs(want)
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    return bool((err <= bound).all()), ratio
