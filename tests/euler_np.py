"""Numpy restatement of the Euler channels (include/emogest.h: eg_articulate_euler / eg_articulate_rot6d_euler / eg_angle_unwrap), written
from the header and independent of emotiongestures_amd.skeleton and of the kernels.

  order     a code 0..5 = XYZ XZY YXZ YZX ZXY ZYX; (i, j, k) its axes; eps = +1 for the cyclic orders XYZ, YZX, ZXY, else -1.
  forward   R_j as in articulate_np (mean, blend, Gram-Schmidt, basis);  s = eps R[i][k];  b = atan2(s, sqrt(R[i][i]^2 + R[i][j]^2));
            1 - |s| >= 2^-20: a = atan2(-eps R[j][k], R[k][k]), c = atan2(-eps R[i][j], R[i][i]);  else a = atan2(eps R[k][j], R[j][j]), c = 0;
            (a, b, c) times 180 / pi for degrees.  Zeros from n_out on.
  inverse   the header's closed form of R_i(a) R_j(b) R_k(c); first two rows (columns) as a1 | a2, minus the mean; zeros from n on.
  unwrap    d_t = p_t - p_(t-1);  k_t = rint(float64(d_t) / P);  c_t = sum k;  out_t = fma(-c_t, P, p_t).

``dtype=np.float32``: every intermediate is rounded to fp32, as in articulate_np: the yardstick E32.  The unwrap in fp32 is exact: it is what
the device must give bit for bit (the fused multiply-add is rounded once, from the exact sum).
"""
import numpy as np

import articulate_np as AN
from skeleton_np import out_frames

ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")


def axes(code):
    i, j, k = ("XYZ".index(ch) for ch in ORDERS[int(code)])
    return i, j, k, (1 if j == (i + 1) % 3 else -1)


def euler_of_matrices(R, codes, degrees=True):
    """R [..., J, 9] row-major -> (a, b, c) [..., J, 3] in the dtype of R; also the s of every joint [..., J]."""
    dt = R.dtype
    out = np.zeros(R.shape[:-1] + (3,), dt)
    ss = np.zeros(R.shape[:-1], dt)
    for jt, code in enumerate(codes):
        i, j, k, eps = axes(code)
        e = dt.type(eps)
        m = lambda r, c: R[..., jt, 3 * r + c]
        s = e * m(i, k)
        free = dt.type(1) - np.abs(s) >= dt.type(2.0 ** -20)
        b = np.arctan2(s, np.sqrt(m(i, i) * m(i, i) + m(i, j) * m(i, j)))
        a = np.where(free, np.arctan2(-e * m(j, k), m(k, k)), np.arctan2(e * m(k, j), m(j, j)))
        c = np.where(free, np.arctan2(-e * m(i, j), m(i, i)), dt.type(0))
        out[..., jt, 0], out[..., jt, 1], out[..., jt, 2], ss[..., jt] = a, b, c, s
    if degrees:
        out = out * dt.type(180.0 / np.pi)
    assert out.dtype == dt
    return out, ss


def euler(track, codes, columns=False, frames=None, mean=None, L=1, M=1, degrees=True, dtype=np.float64, want=False):
    """track [B, T, 6J] -> [B, ceil(T L / M), J, 3] in ``dtype``; with want also (R [B, T_out, J, 9], s [B, T_out, J], (min |a1|, min |u2|))."""
    dt = np.dtype(dtype)
    B, T, D = track.shape
    J = D // 6
    t_out = out_frames(T, L, M)
    out = np.zeros((B, t_out, J, 3), dt)
    Rs, ss = np.zeros((B, t_out, J, 9), dt), np.zeros((B, t_out, J), dt)
    lo1 = lo2 = np.inf
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1:
            continue
        x = AN._blended(track[b], n, J, mean, L, M, dt)
        R, (n1, n2) = AN.matrices(x, columns, want_norms=True)
        lo1, lo2 = min(lo1, float(n1.min())), min(lo2, float(n2.min()))
        out[b, :len(x)], ss[b, :len(x)] = euler_of_matrices(R, codes, degrees)
        Rs[b, :len(x)] = R
    assert out.dtype == dt
    return (out, Rs, ss, (lo1, lo2)) if want else out


def matrices_of_euler(e, codes, degrees=True):
    """(a, b, c) [..., J, 3] -> R [..., J, 9] row-major in the dtype of e: the closed form of the header."""
    dt = e.dtype
    if degrees:
        e = e * dt.type(np.pi / 180.0)
    R = np.zeros(e.shape[:-1] + (9,), dt)
    for jt, code in enumerate(codes):
        i, j, k, eps = axes(code)
        sa, sb, sc = (dt.type(eps) * np.sin(e[..., jt, q]) for q in range(3))
        ca, cb, cc = (np.cos(e[..., jt, q]) for q in range(3))
        m = [cb * cc, -(cb * sc), sb, sa * sb * cc + ca * sc, ca * cc - sa * sb * sc, -(sa * cb), sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb]
        p = {i: 0, j: 1, k: 2}
        for r in range(3):
            for c in range(3):
                R[..., jt, 3 * r + c] = m[3 * p[r] + p[c]]
    assert R.dtype == dt
    return R


def matrices_of_euler_product(e, codes, degrees=True):
    """The same from three axis rotations multiplied, float64: the check of the closed form and what the tests rebuild matrices with."""
    e = np.asarray(e, np.float64)
    if degrees:
        e = np.radians(e)

    def rot(axis, th):
        m = np.zeros(th.shape + (3, 3))
        u, v = (axis + 1) % 3, (axis + 2) % 3
        m[..., axis, axis] = 1.0
        m[..., u, u], m[..., u, v], m[..., v, u], m[..., v, v] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
        return m
    R = np.zeros(e.shape[:-1] + (3, 3))
    for jt, code in enumerate(codes):
        i, j, k, _eps = axes(code)
        R[..., jt, :, :] = rot(i, e[..., jt, 0]) @ rot(j, e[..., jt, 1]) @ rot(k, e[..., jt, 2])
    return R.reshape(R.shape[:-2] + (9,))


def rot6d(e, codes, columns=False, frames=None, mean=None, degrees=True, dtype=np.float64):
    """e [B, T, J, 3] -> [B, T, 6J] in ``dtype``."""
    dt = np.dtype(dtype)
    B, T, J, _3 = e.shape
    out = np.zeros((B, T, 6 * J), dt)
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1:
            continue
        m = matrices_of_euler(np.asarray(e[b, :n], dt), codes, degrees).reshape(n, J, 3, 3)
        if columns:
            m = np.swapaxes(m, -1, -2)
        d = np.ascontiguousarray(m[..., :2, :]).reshape(n, 6 * J)
        out[b, :n] = d if mean is None else d - np.asarray(mean, dt)
    assert out.dtype == dt
    return out


def fma32(x, y, z):
    """fp32 arrays -> the correctly rounded fp32 of x y + z.  x y is exact in float64; the float64 sum s is rounded to fp32 by numpy (ties to
    even), which is wrong only where s lies exactly between two fp32 numbers and the sum's own rounding error (two-sum) says on which side of s
    the exact value is."""
    p = x.astype(np.float64) * y.astype(np.float64)
    z = z.astype(np.float64)
    s = p + z
    bb = s - p
    err = (p - (s - bb)) + (z - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > r64, np.inf, -np.inf).astype(np.float32))
    o64 = other.astype(np.float64)
    tie = (s != r64) & (s == (r64 + o64) * 0.5)
    toward_other = (err != 0) & (np.sign(err) == np.sign(o64 - r64))
    return np.where(tie & toward_other, other, r).astype(np.float32)


def unwrap(p, frames=None, period=360.0, dtype=np.float32):
    """p [B, T, C] -> the same shape in ``dtype``; frames from frames[b] on stay as they are (they may hold NaN)."""
    dt = np.dtype(dtype)
    out = np.array(p, dt)
    B, T, _C = out.shape
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 2:
            continue
        x = out[b, :n].copy()
        d = x[1:] - x[:-1]
        assert d.dtype == dt
        c = np.cumsum(np.rint(d.astype(np.float64) / float(period)).astype(np.int64), axis=0)
        if dt == np.float32:
            out[b, 1:n] = fma32(-c.astype(np.float32), np.full(c.shape, np.float32(period)), x[1:])
        else:
            out[b, 1:n] = x[1:] - c * float(period)
    return out


def orders_cyclic(J):
    """All six orders, one per joint cyclically."""
    return [j % 6 for j in range(J)]
