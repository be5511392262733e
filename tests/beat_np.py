"""Test-side numpy restatement of alignment.load_audio (model/Beat_score_v2.py:58-77) from librosa 0.10's documented routines, and the
decision margins of its beat picks.  A helper module of the beat tests (not collected: no test_ prefix).

  onset_strength(y, sr=16000): |STFT|^2 (n_fft 2048, hop 512, centred, zero pad, periodic Hann) -> Slaney mel (128, fmax 8000)
      -> power_to_db(ref=1.0, amin 1e-10, top_db 80 below the clip max) -> mean_m max(0, db[t] - db[t-1]), 3 leading zeros, T frames
  onset_detect(onset_envelope=oenv): x = (oenv - min) / (max + tiny); peak_pick(pre_max 1, post_max 1, pre_avg 4, post_avg 5, wait 1,
      delta 0.07) -- running sum fp32, mean and threshold fp64 with delta in fp32, as librosa's numba loop
  onset_backtrack(events, energy): minima = 1 + flatnonzero(e[1:-1] <= e[:-2] & e[1:-1] < e[2:]) plus frame 0; largest minimum <= event
  feature.rms(S=|X|): sqrt(2 sum_k P'[k] / 2048^2), DC and Nyquist bins halved
Spectra and dB are fp64 here; oenv is rounded to fp32 (librosa's dtype) before the picks.
"""
import numpy as np

from oracle import emogest_oracle as O

N_FFT, HOP, SR = 2048, 512, 16000
DELTA32 = float(np.float32(0.07))


def stft_power(y: np.ndarray) -> np.ndarray:
    """[n] -> |X|^2 [1025, T] fp64."""
    y = np.asarray(y, np.float64)
    x = np.pad(y, (N_FFT // 2, N_FFT // 2))
    T = 1 + y.size // HOP
    idx = np.arange(N_FFT)[None, :] + HOP * np.arange(T)[:, None]
    frames = x[idx] * O.hann_periodic(N_FFT).astype(np.float64)
    return (np.abs(np.fft.rfft(frames, axis=-1)) ** 2).T


def onset_strength(P: np.ndarray) -> np.ndarray:
    mel = O.mel_filterbank(SR, N_FFT, 128).astype(np.float64) @ P
    db = 10.0 * np.log10(np.maximum(1e-10, mel))
    db = np.maximum(db, db.max() - 80.0)
    flux = np.maximum(0.0, db[:, 1:] - db[:, :-1]).mean(axis=0)
    return np.concatenate([np.zeros(3), flux])[:P.shape[1]]


def rms(P: np.ndarray) -> np.ndarray:
    Q = P.copy()
    Q[0] *= 0.5
    Q[-1] *= 0.5
    return np.sqrt(2.0 * Q.sum(axis=0) / N_FFT ** 2)


def normalise(oenv32: np.ndarray) -> np.ndarray:
    x = oenv32 - oenv32.min()
    return (x / (x.max() + np.finfo(np.float32).tiny)).astype(np.float32)


def peak_pick(x: np.ndarray):
    """-> (events, candidate margins [T]): margin = min(|x[n] - x[n-1]|, |x[n] - (avg + delta)|), the distance of frame n's decision from
    flipping."""
    T = x.size
    if not x.any() or not np.all(np.isfinite(x)):
        return np.array([], np.int64), np.full(T, np.inf)
    cand = np.zeros(T, bool)
    margin = np.full(T, np.inf)
    for n in range(T):
        a0, a1 = max(0, n - 4), min(n + 5, T)
        s = np.float32(0)
        for i in range(a0, a1):
            s = np.float32(s + x[i])
        thr = float(s) / (a1 - a0) + DELTA32
        is_max = n == 0 or x[n] >= x[n - 1]
        cand[n] = is_max and float(x[n]) >= thr
        margin[n] = min(abs(float(x[n]) - thr), abs(float(x[n]) - float(x[n - 1])) if n else np.inf)
    ev, n = [], 0
    while n < T:
        if cand[n]:
            ev.append(n)
            n += 2
        else:
            n += 1
    return np.array(ev, np.int64), margin


def minima(e: np.ndarray):
    """onset_backtrack's minima flags [T] (frame 0 always) and each flag's margin relative to max |e|."""
    T = e.size
    flag = np.zeros(T, bool)
    flag[0] = True
    flag[1:-1] = (e[1:-1] <= e[:-2]) & (e[1:-1] < e[2:])
    scale = max(float(np.abs(e).max()), 1e-30)
    margin = np.full(T, np.inf)
    margin[1:-1] = np.minimum(np.abs(e[1:-1] - e[:-2]), np.abs(e[1:-1] - e[2:])) / scale
    return flag, margin


def backtrack(events: np.ndarray, flag: np.ndarray) -> np.ndarray:
    mins = np.flatnonzero(flag)
    return mins[np.searchsorted(mins, events, side="right") - 1].astype(np.int64)


def load_audio(y: np.ndarray) -> dict:
    """Everything load_audio computes for one clip, plus the margins."""
    P = stft_power(y)
    oenv = onset_strength(P).astype(np.float32)
    r = rms(P).astype(np.float32)
    x = normalise(oenv)
    raw, pm = peak_pick(x)
    fo, mo = minima(oenv)
    fr, mr = minima(r)
    return {"P": P, "oenv": oenv, "rms": r, "x": x, "raw": raw, "bt": backtrack(raw, fo), "bt_rms": backtrack(raw, fr), "peak_margin": pm,
            "min_flag": (fo, fr), "min_margin": (mo, mr)}


def counts(events: np.ndarray, T: int) -> np.ndarray:
    c = np.zeros(T, np.int64)
    np.add.at(c, events, 1)
    return c
