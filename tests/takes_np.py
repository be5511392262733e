"""Take diversity restated in numpy float64 (include/emogest.h: eg_take_meta, eg_track_rows_pack, eg_take_distance): the meta table, the packed
order, and the pairwise distance of the takes of one recording.  No GPU, no library: the in-tree reference of tests/test_takes.py and
tests/test_gpu_takes.py."""
import numpy as np


def meta_np(frames):
    """`frames | off`, int32, off the exclusive prefix sum."""
    f = np.asarray(frames, np.int64)
    return np.concatenate([f, np.concatenate([[0], np.cumsum(f)[:-1]])]).astype(np.int32)


def packed_index(frames, R):
    """(u, r, t) of every packed row: recording-major, then draw, then frame; row R*off[u] + r*frames[u] + t holds pose (u, r, t)."""
    us, rs, ts = [], [], []
    for u, f in enumerate(frames):
        for r in range(R):
            us.append(np.full(f, u)); rs.append(np.full(f, r)); ts.append(np.arange(f))
    return np.concatenate(us), np.concatenate(rs), np.concatenate(ts)


def pack_np(track, frames):
    """track [U, R, Tmax, D] -> rows [N, 4*ceil(D/4)]: the valid rows in packed order, zero pad columns."""
    U, R, _T, D = track.shape
    u, r, t = packed_index(frames, R)
    rows = np.zeros((u.size, (D + 3) // 4 * 4), track.dtype)
    rows[:, :D] = track[u, r, t]
    return rows


def takes_of(feat, frames, R, u):
    """Recording u's block of the packed features as [R, frames[u], K]."""
    off = int(np.sum(frames[:u]))
    return feat[R * off: R * (off + frames[u])].reshape(R, frames[u], feat.shape[1])


def take_distance_np(feat, frames, R, span=None):
    """feat [N, K] fp32 packed -> (distance [U, R, R], diversity [U]) float64: every operand widened before the subtraction,
    S = sum (a - b)^2 over the frames[u] x K block, distance = sqrt(S * scale), scale = 1 or span / frames[u]; diversity = the mean over the
    pairs r < r' in lexicographic order."""
    U = len(frames)
    dist = np.zeros((U, R, R), np.float64)
    div = np.zeros(U, np.float64)
    for u in range(U):
        a = takes_of(feat, frames, R, u).astype(np.float64)
        scale = 1.0 if span is None else float(span) / float(frames[u])
        acc = 0.0
        for r in range(R):
            for rp in range(r + 1, R):
                S = ((a[r] - a[rp]) ** 2).sum()
                d = np.sqrt(S * scale)
                dist[u, r, rp] = dist[u, rp, r] = d
                acc += d
        div[u] = 2.0 / (R * (R - 1)) * acc if R > 1 else 0.0
    return dist, div
