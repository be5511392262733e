"""Float64 numpy restatement of the skeleton conversions (include/emogest.h: eg_skeleton_joints / eg_skeleton_dir_vec), written from the
definition and independent of emotiongestures_amd.skeleton, plus the error bounds the GPU tests hold the fp32 kernels to.

A table is ``(parents [K], children [K], lengths [K])``; joint 0 is the root at the origin.
  forward   x_k = v[t, 3k:3k+3] (+ mean_k); unit: x_k / max(|x_k|, 1e-12); p[0] = 0, p[child_k] = p[parent_k] + length_k x_k in table order.
            A row of n valid frames at the rate L / M has n_out = ceil(n L / M) frames: frame k' = p(lo) + (p(lo+1) - p(lo)) f,
            lo = min(floor(k' M / L), n - 2), f = (k' M - lo L) / L from exact integers; n = 1: p(0); L = M: p(k').  Zeros from n_out on.
  inverse   d = p[child_k] - p[parent_k]; d / max(|d|, 1e-12) (- mean_k).  Zeros from n on.

Bounds (u = 2^-24, d = bones between the root and the joint, S = the sum along the joint's path of length_k |x_k| per coordinate).  Every
term length_k x_k carries the rounding of the fp32 length, of the mean's addition and of its product, every partial sum one more:
  native              (d + 3) u S,   S = sum length_k (|v_k| + |mean_k|)
  native, unit        (d + 6) u S,   S = sum length_k |x^_k|               (the normalisation: squares, square root and division, each within 1 ulp)
  interpolated        (d + 6 [+ 3 with unit]) u ((1 + |f|) S(lo) + |f| S(lo + 1))     (the difference, f and the final product-sum)
  inverse             5 u absolute per component (|component| <= 1: the difference, three squares and their sum, the root, the division)
FMA contraction only removes roundings.
"""
import numpy as np

U24 = 2.0 ** -24
INVERSE_BOUND = 5 * U24


def depth(table):
    parents, children, _l = table
    d = np.zeros(len(parents) + 1, np.int64)
    for a, b in zip(parents, children):
        d[b] = d[a] + 1
    return d


def chain(table, x):
    """x [..., K, 3] -> p [..., J, 3]."""
    parents, children, lengths = table
    p = np.zeros(x.shape[:-2] + (len(parents) + 1, 3))
    for k in range(len(parents)):
        p[..., children[k], :] = p[..., parents[k], :] + float(lengths[k]) * x[..., k, :]
    return p


def out_frames(n, L=1, M=1):
    return -(-int(n) * L // M)


def segments(n, L, M):
    """(lo [n_out], f [n_out]) of a row of n >= 2 frames, from integers."""
    k = np.arange(out_frames(n, L, M), dtype=np.int64)
    lo = np.minimum(k * M // L, n - 2)
    return lo, (k * M - lo * L) / L


def _vectors(v, n, K, mean, unit):
    x = np.asarray(v[:n], np.float64).reshape(n, K, 3)
    if mean is not None:
        x = x + np.asarray(mean, np.float64).reshape(K, 3)
    if unit:
        x = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
    return x


def joints(track, table, frames=None, mean=None, unit=False, L=1, M=1):
    """track [B, T, 3K] -> float64 [B, ceil(T L / M), J, 3].  Frames from frames[b] on are never touched (they may hold NaN)."""
    B, T, D = track.shape
    K = D // 3
    out = np.zeros((B, out_frames(T, L, M), K + 1, 3))
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1:
            continue
        p = chain(table, _vectors(track[b], n, K, mean, unit))
        if L == M:
            out[b, :n] = p
        elif n == 1:
            out[b, :out_frames(1, L, M)] = p[0]
        else:
            lo, f = segments(n, L, M)
            out[b, :len(lo)] = p[lo] + (p[lo + 1] - p[lo]) * f[:, None, None]
    return out


def joints_bound(track, table, frames=None, mean=None, unit=False, L=1, M=1):
    """The bound of the docstring for every element of joints(...): [B, T_out, J, 3] (zero where the output is a written zero)."""
    B, T, D = track.shape
    K = D // 3
    dep = depth(table)[None, :, None].astype(np.float64)
    out = np.zeros((B, out_frames(T, L, M), K + 1, 3))
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1:
            continue
        if unit:
            ax = np.abs(_vectors(track[b], n, K, mean, True))
        else:
            ax = np.abs(np.asarray(track[b, :n], np.float64).reshape(n, K, 3))
            if mean is not None:
                ax = ax + np.abs(np.asarray(mean, np.float64).reshape(K, 3))
        S = chain(table, ax)
        if L == M:
            out[b, :n] = (dep + (6 if unit else 3)) * U24 * S
            continue
        if n == 1:
            lo, f, hi = np.zeros(out_frames(1, L, M), np.int64), np.zeros(out_frames(1, L, M)), np.zeros(out_frames(1, L, M), np.int64)
        else:
            lo, f = segments(n, L, M)
            hi = lo + 1
        af = np.abs(f)[:, None, None]
        out[b, :len(lo)] = (dep + (9 if unit else 6)) * U24 * ((1 + af) * S[lo] + af * S[hi])
    return out


def dir_vec(pose, table, frames=None, mean=None):
    """pose [B, T, J, 3] -> float64 [B, T, 3K]."""
    parents, children, _l = table
    B, T = pose.shape[:2]
    K = len(parents)
    out = np.zeros((B, T, 3 * K))
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1:
            continue
        p = np.asarray(pose[b, :n], np.float64)
        d = p[:, np.asarray(children)] - p[:, np.asarray(parents)]
        d = (d / np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12)).reshape(n, 3 * K)
        out[b, :n] = d if mean is None else d - np.asarray(mean, np.float64)
    return out


# ---- tables beside the TED one -------------------------------------------------------------------------------------------------------------
def chain_table(K=5):
    return list(range(K)), list(range(1, K + 1)), [0.1 * (k + 1) for k in range(K)]


def star_table(K=5):
    return [0] * K, list(range(1, K + 1)), [0.3 - 0.04 * k for k in range(K)]


def random_table(K=63, seed=3):
    """K bones in a random topological order: every bone hangs off the root or off the child of an earlier bone; joint numbers are shuffled."""
    rng = np.random.default_rng(seed)
    label = np.concatenate([[0], 1 + rng.permutation(K)])            # position in creation order -> joint number
    parents = [int(label[rng.integers(0, k + 1)]) for k in range(K)]
    children = [int(label[k + 1]) for k in range(K)]
    return parents, children, [float(v) for v in rng.uniform(0.02, 0.5, K)]
