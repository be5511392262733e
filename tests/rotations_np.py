"""Numpy restatement of the rotation output (include/emogest.h: eg_skeleton_rest_check / eg_skeleton_levels / eg_skeleton_rotations), written
from the header and independent of emotiongestures_amd.skeleton and of the kernel, plus the inverse, forward kinematics and the generator of
test tracks from known swings.

A table is ``(parents [K], children [K], lengths [K])`` as in skeleton_np.  Quaternions are ``(w, x, y, z)`` on the last axis.
  rest      [K, 3]: every row normalised in float64 and rounded to fp32 (``unit_rest``); unit vectors from then on.
  pb(k)     the bone whose child is parents[k]; -1 at the root (``bone_parents``).
  x^_k      x_k / max(|x_k|, 1e-12), x_k = v[t, 3k:3k+3] (+ mean_k)
  arc(a,b)  c = a . b >= -1 + 1e-6: (1 + c, a x b) normalised; else (0, n), n = a x e_m normalised, e_m the first axis on which |a| is smallest.
  chain     P_k = G_pb(k) (identity at the root); v_k = conj(P_k) o x^_k; L_k = arc(rest_k, v_k); G_k = P_k (x) L_k, in table order.
  frames    as skeleton_np.joints, but the VECTORS are blended (after the mean): x = (x(lo+1) - x(lo)) f + x(lo); n = 1: frame 0; L = M: frame k'.
            Zeros from n_out on; source frames from n on are never touched.

``dtype=np.float32``: every intermediate is rounded to fp32 (numpy rounds each fp32 operation once; no fused multiply-add), which gives the
error an fp32 implementation of the definition has on the same inputs: the yardstick the GPU tests measure the kernel with.

``variant`` restates the chain WRONG on purpose, to show that the tolerance of the tests discriminates: "swapped" (L_k (x) P_k), "previous"
(pb(k) = k - 1) and "noconj" (v_k = P_k o x^_k).
"""
import numpy as np

from skeleton_np import out_frames, segments


def bone_parents(table):
    parents, children, _l = table
    owner = {}
    pb = []
    for k, (a, b) in enumerate(zip(parents, children)):
        pb.append(owner.get(int(a), -1))
        owner[int(b)] = k
    return pb


def unit_rest(rest):
    """[K, 3] any length -> fp32 unit rows (normalised in float64)."""
    r = np.asarray(rest, np.float64)
    return (r / np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])[:, None]).astype(np.float32)


# ---- quaternions ---------------------------------------------------------------------------------------------------------------------------
def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def qmul(p, q):
    pw, px, py, pz = (p[..., i] for i in range(4))
    qw, qx, qy, qz = (q[..., i] for i in range(4))
    return np.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)


def qconj(q):
    return np.concatenate([q[..., :1], -q[..., 1:]], -1)


def qrot(q, v):
    """q o v = v + 2 w (u x v) + 2 u x (u x v), u = q.xyz."""
    u, w = q[..., 1:], q[..., :1]
    t = cross(u, v)
    t = t + t
    return v + w * t + cross(u, t)


def arc(a, b):
    """a [3] unit, b [n, 3] unit or zero -> (q [n, 4], c [n]) in the dtype of b."""
    dt = b.dtype
    a = a.astype(dt)
    c = b[:, 0] * a[0] + b[:, 1] * a[1] + b[:, 2] * a[2]
    q = np.concatenate([(1 + c)[:, None], cross(np.broadcast_to(a, b.shape), b)], -1).astype(dt)
    nrm = np.sqrt((q * q).sum(-1, keepdims=True))
    half = c < dt.type(-1.0) + dt.type(1e-6)
    q = q / np.where(half[:, None], 1, nrm)
    if half.any():
        e = np.zeros(3, dt)
        e[int(np.argmin(np.abs(a)))] = 1                          # the first such axis on ties
        n = cross(a, e)
        n = n / np.sqrt((n * n).sum())
        q[half] = np.concatenate([np.zeros(1, dt), n])
    return q.astype(dt), c


def _blended(v, n, K, mean, L, M, dt):
    """The (blended) vectors of the output frames of a row of n frames: [n_out, K, 3]."""
    x = np.asarray(v[:n], dt).reshape(n, K, 3)
    if mean is not None:
        x = x + np.asarray(mean, dt).reshape(K, 3)
    if L == M:
        return x
    if n == 1:
        return np.repeat(x[:1], out_frames(1, L, M), 0)
    lo, f = segments(n, L, M)
    return (x[lo + 1] - x[lo]) * f.astype(dt)[:, None, None] + x[lo]


def rotations(track, table, rest, frames=None, mean=None, space="local", L=1, M=1, dtype=np.float64, variant=None, want_c=False):
    """track [B, T, 3K], rest [K, 3] fp32 unit rows -> [B, ceil(T L / M), K, 4] in ``dtype``; with want_c also min c over every bone and frame."""
    dt = np.dtype(dtype)
    B, T, D = track.shape
    K = D // 3
    pb = bone_parents(table)
    if variant == "previous":
        pb = [k - 1 for k in range(K)]
    r = np.asarray(rest, np.float32).astype(dt)
    out = np.zeros((B, out_frames(T, L, M), K, 4), dt)
    cmin = 1.0
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1:
            continue
        x = _blended(track[b], n, K, mean, L, M, dt)
        x = (x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), dt.type(1e-12))).astype(dt)
        G = np.zeros((len(x), K, 4), dt)
        loc = np.zeros((len(x), K, 4), dt)
        for k in range(K):
            if pb[k] < 0:
                loc[:, k], c = arc(r[k], x[:, k])
                G[:, k] = loc[:, k]
            else:
                P = G[:, pb[k]]
                loc[:, k], c = arc(r[k], qrot(P if variant == "noconj" else qconj(P), x[:, k]))
                G[:, k] = qmul(loc[:, k], P) if variant == "swapped" else qmul(P, loc[:, k])
            cmin = min(cmin, float(c.min()))
        out[b, :len(x)] = G if space == "global" else loc
    assert out.dtype == dt
    return (out, cmin) if want_c else out


def unit_vectors(track, table, frames=None, mean=None, L=1, M=1):
    """x^_k of every output frame in float64: [B, ceil(T L / M), K, 3] (zeros behind a row's end)."""
    B, T, D = track.shape
    K = D // 3
    out = np.zeros((B, out_frames(T, L, M), K, 3))
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1:
            continue
        x = _blended(track[b], n, K, mean, L, M, np.dtype(np.float64))
        out[b, :len(x)] = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
    return out


# ---- the inverse and forward kinematics ----------------------------------------------------------------------------------------------------
def globals_from_locals(table, loc):
    """L [..., K, 4] -> G [..., K, 4], float64."""
    pb = bone_parents(table)
    loc = np.asarray(loc, np.float64)
    G = np.zeros_like(loc)
    for k in range(loc.shape[-2]):
        G[..., k, :] = loc[..., k, :] if pb[k] < 0 else qmul(G[..., pb[k], :], loc[..., k, :])
    return G


def directions(G, rest):
    """Global rotations [..., K, 4] -> the bone directions G_k o rest_k [..., K, 3], float64: the inverse of the rotation output."""
    G = np.asarray(G, np.float64)
    return qrot(G, np.broadcast_to(np.asarray(rest, np.float64), G.shape[:-1] + (3,)))


def fk(table, rest, loc):
    """Forward kinematics of an avatar with bone offsets length_k rest_k and local rotations L [..., K, 4]: joints [..., J, 3], float64."""
    parents, children, lengths = table
    d = directions(globals_from_locals(table, loc), rest)
    p = np.zeros(d.shape[:-2] + (len(parents) + 1, 3))
    for k in range(len(parents)):
        p[..., children[k], :] = p[..., parents[k], :] + float(lengths[k]) * d[..., k, :]
    return p


# ---- test tracks from known swings ---------------------------------------------------------------------------------------------------------
def random_rest(K, seed):
    return unit_rest(np.random.default_rng(seed).standard_normal((K, 3)))


def swing_tracks(table, rest, T, cap_deg, seed, B=1, mean=None, smooth=False):
    """Tracks whose local rotations are known swings: per bone an axis perpendicular to rest_k and an angle <= cap_deg, composed down the tree,
    times random positive scales, minus the mean when one is used.  ``smooth``: the angles vary slowly in time and a bone keeps its scale (for interpolation
    tests), else both are independent per frame.  -> (track fp32 [B, T, 3K], locals float64 [B, T, K, 4])."""
    rng = np.random.default_rng(seed)
    r = np.asarray(rest, np.float64)
    K = len(r)
    a = rng.standard_normal((B, 1 if smooth else T, K, 3))
    a = a - (a * r).sum(-1, keepdims=True) * r / (r * r).sum(-1, keepdims=True)
    a = a / np.sqrt((a * a).sum(-1, keepdims=True))
    if smooth:
        t = np.arange(T)[None, :, None]
        th = 0.5 + 0.5 * np.sin(rng.uniform(0.02, 0.12, (B, 1, K)) * t + rng.uniform(0, 6.28, (B, 1, K)))
    else:
        th = rng.uniform(0, 1, (B, T, K))
    th = np.deg2rad(cap_deg) * th
    loc = np.concatenate([np.cos(th / 2)[..., None], np.sin(th / 2)[..., None] * np.broadcast_to(a, (B, T, K, 3))], -1)
    # positive scales: per frame, or one per bone (an extrapolated blend of two frames must not turn a vector round)
    x = directions(globals_from_locals(table, loc), r) * rng.uniform(0.5, 2.0, (B, 1 if smooth else T, K, 1))
    x = x.reshape(B, T, 3 * K)
    if mean is not None:
        x = x - np.asarray(mean, np.float64)
    return x.astype(np.float32), loc
