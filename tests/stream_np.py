"""CPU restatement of the streaming session (include/emogest.h: eg_stream_*) for the tests: the audio ring written with wrap-around, the
window's offset in it, the symmetric padding rule of an ended row, and the per-step emission (rows, prior, tail).  Written from the
definition, independently of emotiongestures_amd.streaming: no code is shared with the functions it checks."""
import numpy as np

from rollout_np import default_alpha


class RingRow:
    """One row of a session.  push(chunk [hop], end) -> the row's clip [n] when a window is ready, else None."""

    def __init__(self, hop, n):
        self.hop, self.n = hop, n
        self.lag = (n + hop - 1) // hop
        self.ring = np.zeros(self.lag * hop, np.float32)
        self.c = self.w = 0
        self.total = -1

    def push(self, chunk, end=-1):
        hop, n, lag = self.hop, self.n, self.lag
        chunk = np.asarray(chunk, np.float32).copy()
        assert chunk.shape == (hop,)
        if self.total >= 0:
            chunk[:] = 0                                    # an ended row's audio is ignored, its ring is fed zeros
        elif end >= 0:
            chunk[end:] = 0
        slot = self.c % lag                                 # wrap-around write: nothing is moved
        self.ring[slot * hop: (slot + 1) * hop] = chunk
        self.c += 1
        if self.total < 0 and end >= 0:
            self.total = (self.c - 1) * hop + end
        ready = self.c >= self.w + lag if self.total < 0 else self.w * hop < self.total
        if not ready:
            return None
        oldest_first = np.roll(self.ring, -((self.c % lag) * hop))       # the newest lag*hop samples in time order
        offset = 0 if self.total < 0 else (self.w + lag - self.c) * hop
        assert offset >= 0 and self.c - self.w <= lag
        L = n if self.total < 0 else self.total - self.w * hop
        k = np.arange(n)
        if L < n:                                           # period 2L: the samples mirrored about the end, the last one repeated
            k = k % (2 * L)
            k = np.where(k >= L, 2 * L - 1 - k, k)
        self.w += 1
        return oldest_first[offset + k]


def feed(hop, n, audio, steps):
    """A recording fed hop by hop through a RingRow, ending in the push that holds its last sample: [(step, clip)] of the ready windows."""
    T = len(audio)
    last = max(1, -(-T // hop))
    padded = np.zeros((max(steps, last)) * hop, np.float32)
    padded[:T] = audio
    padded[T:] = 777.0                                      # what the caller sends past the end must never reach a window
    row, out = RingRow(hop, n), []
    for s in range(1, steps + 1):
        clip = row.push(padded[(s - 1) * hop: s * hop], T - (last - 1) * hop if s == last else -1)
        out.append(clip)
    return out


def emit(windows, prior_frames, seed_pose, alpha=None):
    """windows [W, F, D]: one row's raw per-window poses in step order -> ([W] rows [H, D], tail [P, D]) in fp32: for w >= 1 the first P rows
    are (1 - alpha[j]) * prior[j] + alpha[j] * pose[j] (two rounded products, one rounded sum), the rest raw; prior := pose[H:]."""
    windows = np.asarray(windows, np.float32)
    W, F, D = windows.shape
    P, H = prior_frames, F - prior_frames
    a = default_alpha(P) if alpha is None else np.asarray(alpha, np.float32)
    prior, rows = np.asarray(seed_pose, np.float32).copy(), []
    for w in range(W):
        r = windows[w, :H].copy()
        if w >= 1:
            old = (np.float32(1) - a)[:, None] * prior
            new = a[:, None] * windows[w, :P]
            r[:P] = old + new
        rows.append(r)
        prior = windows[w, H:].copy()
    return rows, prior
