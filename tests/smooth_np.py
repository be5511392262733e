"""Float64 numpy restatement of the smoothing filter (include/emogest.h: eg_smooth_design / eg_smooth_tracks), written from the header's
definition and independent of emotiongestures_amd/smooth.py: the design by numpy's QR on the centred abscissae, the filter frame by frame
with explicit sums, and the a-priori fp32 bound of one output element."""
import math

import numpy as np

MAX_WINDOW = 31
U24 = 2.0 ** -24


def allowed():
    """Every (K, p, d) the header allows."""
    return [(K, p, d) for K in range(3, MAX_WINDOW + 1, 2) for p in range(1, min(5, K - 1) + 1) for d in range(0, min(2, p) + 1)]


def design(K, p, d, delta):
    """C [K, K] float64: row i gives the d-th derivative at window position i of the least-squares polynomial of degree p through K samples."""
    half = K // 2
    t = np.arange(K, dtype=np.float64) - half
    A = t[:, None] ** np.arange(p + 1)[None, :]                          # centred Vandermonde
    Q, R = np.linalg.qr(A)
    pinv = np.linalg.solve(R, Q.T)                                       # the polynomial's coefficients are pinv @ x
    C = np.zeros((K, K))
    for i in range(K):
        g = np.array([0.0 if q < d else math.factorial(q) / math.factorial(q - d) * t[i] ** (q - d) for q in range(p + 1)]) / delta ** d
        C[i] = g @ pinv
    return C


def terms(x, C, n):
    """For one row x [T, D] with n valid frames: (table row, first source frame) of every frame i < n."""
    K = C.shape[0]
    half = K // 2
    for i in range(n):
        if i < half:
            yield i, i, 0
        elif i < n - half:
            yield i, half, i - half
        else:
            yield i, K - (n - i), n - K


def smooth(v, C, frames=None):
    """v [B, T, D] -> (y [B, T, D] float64, mag [B, T, D] = sum_j |C[.][j]| |x[.]|).  Frames from frames[b] on: zeros, never read."""
    v = np.asarray(v)
    B, T, D = v.shape
    K = C.shape[0]
    y, mag = np.zeros((B, T, D)), np.zeros((B, T, D))
    for b in range(B):
        n = T if frames is None else frames[b]
        assert n >= K
        x = v[b, :n].astype(np.float64)
        for i, row, s in terms(x, C, n):
            y[b, i] = C[row] @ x[s:s + K]
            mag[b, i] = np.abs(C[row]) @ np.abs(x[s:s + K])
    return y, mag


def bound(mag, K):
    """|y - y64| <= (K + 2) 2^-24 sum_j |C[i][j]| |x[j]|: one 2^-24 per term for the table's rounding to fp32, K 2^-24 relative for the K-term
    fmaf chain, one more for second-order terms."""
    return (K + 2) * U24 * mag
