"""float64 restatement of the polyphase resampler (include/emogest.h, "Polyphase resampler"): the plan, the filter in numpy terms, the
direct sum with `delay` and per-row lengths, and the chunked form with a history.  No scipy here: tests compare this against scipy."""
import math

import numpy as np

RATES = (48000, 44100, 32000, 24000, 22050, 11025, 8000, 96000)
# rate_in: (L, M, half, K, D, Hs) at rate_out = 16000
PLAN_TABLE = {48000: (1, 3, 30, 61, 10, 60), 44100: (160, 441, 4410, 56, 10, 56), 32000: (1, 2, 20, 41, 10, 40), 24000: (2, 3, 30, 31, 10, 30),
              22050: (320, 441, 4410, 28, 10, 28), 11025: (640, 441, 6400, 21, 15, 21), 8000: (2, 1, 20, 21, 20, 20),
              96000: (1, 6, 60, 121, 10, 120)}


def plan_np(rate_in, rate_out=16000):
    g = math.gcd(int(rate_in), int(rate_out))
    L, M = rate_out // g, rate_in // g
    half = 10 * max(L, M)
    K = -(-(2 * half + 1) // L)
    D = -(-half // M)
    Hs = -(-(D * M + half) // L)
    return dict(L=L, M=M, half=half, K=K, D=D, Hs=Hs)


def filter_np(rate_in, rate_out=16000):
    p = plan_np(rate_in, rate_out)
    half, fc = p["half"], 1.0 / max(p["L"], p["M"])
    k = np.arange(2 * half + 1)
    h = fc * np.sinc(fc * (k - half)) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * p["L"]


def out_length_np(n_in, rate_in, rate_out=16000):
    p = plan_np(rate_in, rate_out)
    return -(-int(n_in) * p["L"] // p["M"])


def _sum(x, h, p, n, delay, lo):
    """y[n], S[n] for the output indices `n` (array) of a signal whose sample i is x[i - lo] (zero outside x)."""
    L, M, half, K = p["L"], p["M"], p["half"], p["K"]
    pp = half + (n.astype(np.int64) - delay) * M
    ihi = np.floor_divide(pp, L)
    ph = pp - ihi * L
    y = np.zeros(len(n))
    S = np.zeros(len(n))
    x = np.asarray(x, np.float64)
    for j in range(K):
        i = ihi - j - lo
        k = ph + j * L
        ok = (k <= 2 * half) & (i >= 0) & (i < len(x))
        t = np.where(ok, x[np.clip(i, 0, len(x) - 1)] * h[np.clip(k, 0, 2 * half)], 0.0)
        y += t
        S += np.abs(t)
    return y, S


def resample_np(x, rate_in, rate_out=16000, delay=0, h=None):
    """One row x [n_in] (exactly its real samples) -> (y [n_out], S [n_out]) in float64; `h`: the taps to use (default filter_np)."""
    p = plan_np(rate_in, rate_out)
    h = filter_np(rate_in, rate_out) if h is None else np.asarray(h, np.float64)
    n = np.arange(out_length_np(len(x), rate_in, rate_out))
    return _sum(x, h, p, n, delay, 0)


def resample_rows_np(x, lengths, rate_in, rate_out=16000, delay=0, out_stride=None, h=None):
    """x [U, stride] with lengths -> (y, S) [U, out_stride], zeros behind every row's own output."""
    nout = [out_length_np(l, rate_in, rate_out) for l in lengths]
    stride = max(nout) if out_stride is None else out_stride
    y = np.zeros((len(lengths), stride))
    S = np.zeros((len(lengths), stride))
    for u, l in enumerate(lengths):
        y[u, :nout[u]], S[u, :nout[u]] = resample_np(np.asarray(x[u])[:l], rate_in, rate_out, delay, h)
    return y, S


class StreamNp:
    """The chunked form: every push is the same computation on [history | chunk] in local indices."""

    def __init__(self, rate_in, hop_out, rate_out=16000, h=None):
        self.p = plan_np(rate_in, rate_out)
        self.rates = (rate_in, rate_out)
        self.hop = int(hop_out)
        assert self.hop * self.p["M"] % self.p["L"] == 0
        self.hop_in = self.hop * self.p["M"] // self.p["L"]
        assert self.hop_in >= self.p["Hs"]
        self.h = filter_np(rate_in, rate_out) if h is None else np.asarray(h, np.float64)
        self.hist = np.zeros(self.p["Hs"])

    def reset(self):
        self.hist[:] = 0

    def push(self, chunk, end=-1):
        m = self.hop_in if end < 0 else min(int(end), self.hop_in)
        c = np.zeros(self.hop_in)
        c[:m] = np.asarray(chunk, np.float64)[:m]
        buf = np.concatenate([self.hist, c])
        real = self.hop if end < 0 else -(-m * self.p["L"] // self.p["M"])
        y = np.zeros(self.hop)
        y[:real], _S = _sum(buf, self.h, self.p, np.arange(real), self.p["D"], -self.p["Hs"])
        self.hist = buf[len(buf) - self.p["Hs"]:].copy()
        return y
