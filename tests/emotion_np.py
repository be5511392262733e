"""numpy restatement of the emotion recognition of whole tracks (include/emogest.h, emotiongestures_amd/emotion.py), written from the
definition: the window plan, the gather of the classifier windows and the votes.  Plain loops; nothing here imports the module under test."""
import math

import numpy as np

CHUNK = 64                                  # EG_EMOTION_CHUNK_WINDOWS


def starts_np(f, F, S=None, tail=True):
    """First pose of every classifier window of a recording with f valid poses: 0, S, 2S, ... while start + F <= f, and with `tail` one
    more at f - F when (f - F) % S != 0."""
    S = F if S is None else S
    assert f >= F and F >= 1 and S >= 1
    out, s = [], 0
    while s + F <= f:
        out.append(s)
        s += S
    if tail and (f - F) % S != 0:
        out.append(f - F)
    return out


def plan_np(frames, F, S=None, tail=True):
    """-> (meta `frames | off | C | coff` int32 [4U], starts per recording)."""
    starts = [starts_np(f, F, S, tail) for f in frames]
    counts = [len(s) for s in starts]
    off = np.concatenate([[0], np.cumsum(frames)[:-1]])
    coff = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return np.concatenate([frames, off, counts, coff]).astype(np.int32), starts


def clip_rows(frames, R, F, S=None, tail=True):
    """The packed pose row (takes.pack_rows' order: R*off[u] + r*frames[u] + t) of the first pose of every clip, in clip order
    (recording-major, then take, then window) -> int64 [N]."""
    meta, starts = plan_np(frames, F, S, tail)
    U = len(frames)
    rows = []
    for u, f in enumerate(frames):
        for r in range(R):
            rows += [R * int(meta[U + u]) + r * f + s for s in starts[u]]
    return np.asarray(rows, np.int64)


def embed_np(emb, pos, frames, R, F, S=None, tail=True):
    """x[c * F + f] = emb[row(c) + f] + pos[f] in fp32 -> [N * F, d_model]."""
    first = clip_rows(frames, R, F, S, tail)
    idx = (first[:, None] + np.arange(F)[None, :]).reshape(-1)
    return (emb[idx].reshape(len(first), F, -1) + pos[None, :F]).astype(np.float32).reshape(len(idx), -1)


def windows_of(track, frames, F, S=None, tail=True):
    """The classifier windows of track [U, R, Tmax, D] cut by slicing on the host, in clip order -> [N, F, D]."""
    U, R = track.shape[:2]
    out = []
    for u, f in enumerate(frames):
        for r in range(R):
            out += [track[u, r, s:s + F] for s in starts_np(f, F, S, tail)]
    return np.stack(out)


def votes_np(logits, counts, R, labels=None):
    """logits [N, C] float32 in clip order, counts [U] windows per recording, labels [U, R] class indices or None -> the dict of the
    definition (label figures only with labels)."""
    logits = np.asarray(logits, np.float32)
    N, C = logits.shape
    U = len(counts)
    assert N == R * sum(counts)
    wclass = np.zeros(N, np.int32)
    for i in range(N):
        row = logits[i]
        if not np.all(np.isfinite(row)):
            wclass[i] = -1
            continue
        best = 0
        for c in range(1, C):
            if row[c] > row[best]:
                best = c                    # strictly greater: the lowest index among the maxima
        wclass[i] = best
    votes = np.zeros((U, R, C), np.int32)
    invalid = np.zeros((U, R), np.int32)
    mean = np.full((U, R, C), np.nan, np.float64)
    pred = np.full((U, R), -1, np.int32)
    i0 = 0
    for u in range(U):
        n = counts[u]
        for r in range(R):
            total = np.zeros(C, np.float64)
            for w0 in range(0, n, CHUNK):
                part = np.zeros(C, np.float64)
                for w in range(w0, min(n, w0 + CHUNK)):
                    k = wclass[i0 + w]
                    if k < 0:
                        invalid[u, r] += 1
                        continue
                    votes[u, r, k] += 1
                    part = part + logits[i0 + w].astype(np.float64)
                total = total + part
            count = n - invalid[u, r]
            if count > 0:
                mean[u, r] = total / np.float64(count)
                best = 0
                for c in range(1, C):
                    if votes[u, r, c] > votes[u, r, best] or (votes[u, r, c] == votes[u, r, best] and mean[u, r, c] > mean[u, r, best]):
                        best = c
                pred[u, r] = best
            i0 += n
    out = {"window_class": wclass, "votes": votes, "invalid": invalid, "mean_logit": mean, "pred": pred,
           "unscored": np.int32(np.count_nonzero(pred == -1))}
    if labels is None:
        return out
    y = np.asarray(labels, np.int64).reshape(U, R)
    hit = np.zeros((U, R), np.int32)
    whits = np.zeros((U, R), np.int32)
    conf = np.zeros((C, C), np.int32)
    wconf = np.zeros((C, C), np.int32)
    for u in range(U):
        for r in range(R):
            hit[u, r] = int(pred[u, r] == y[u, r])
            whits[u, r] = votes[u, r, y[u, r]]
            if pred[u, r] >= 0:
                conf[y[u, r], pred[u, r]] += 1
            wconf[y[u, r]] += votes[u, r]
    out.update({"hit": hit, "window_hits": whits, "confusion": conf, "window_confusion": wconf,
                "accuracy": np.float64(100.0 * float(hit.sum()) / float(U * R)),
                "window_accuracy": np.float64(100.0 * float(whits.sum()) / float(N))})
    return out


def exact_mean_np(logits, counts, R, wclass):
    """The exactly rounded mean of the valid windows' logits per take (math.fsum) and sum |l| / count -> ([U, R, C], [U, R, C]); NaN
    where no window is valid."""
    logits = np.asarray(logits, np.float32)
    C = logits.shape[1]
    U = len(counts)
    mean, mag = np.full((U, R, C), np.nan), np.full((U, R, C), np.nan)
    i0 = 0
    for u in range(U):
        for r in range(R):
            rows = [i for i in range(i0, i0 + counts[u]) if wclass[i] >= 0]
            i0 += counts[u]
            if not rows:
                continue
            for c in range(C):
                vals = [float(logits[i, c]) for i in rows]
                mean[u, r, c] = math.fsum(vals) / len(rows)
                mag[u, r, c] = math.fsum(abs(v) for v in vals) / len(rows)
    return mean, mag
