"""Audio at any common sample rate -> the model's rate (16 kHz) on the device: a polyphase resampler (csrc/resample.hip).

The mel front-end, the roll-out and the streams are defined on 16 kHz samples; microphones give 44.1 or 48 kHz, TTS voices 24 kHz.  This
module is the first step of "raw audio -> gesture track" without leaving the GPU:

``resample_audio(audio, rate_in)``            whole recordings ``[T]`` or ``[U, T]`` (with ``lengths``: of unequal length) in one launch
``StreamResampler(rows, rate_in, hop_out)``   the same signal push by push, with static buffers, for a captured graph

Definition (include/emogest.h): ``g = gcd(rate_in, rate_out)``, ``L = rate_out / g``, ``M = rate_in / g``, supported while
``max(L, M) <= 640``; the filter is ``scipy.signal.firwin(2*half + 1, 1 / max(L, M), window=("kaiser", 5.0)) * L`` with
``half = 10 * max(L, M)`` -- the filter of ``scipy.signal.resample_poly``'s defaults, designed by the library in float64 and rounded to
fp32 (scipy is not imported); ``n_out = ceil(n_in * L / M)`` and ``y[n] = sum_i x[i] * h[half + (n - delay)*M - i*L]``.  With ``delay=0``
that is ``resample_poly(x, L, M)``.

A live resampler cannot see the future: a stream's signal is the offline one delayed by ``D = stream_delay(rate_in)`` output samples (10 for
the down-sampling rates, 0.6 ms), cut to ``n_out`` samples -- ``resample_audio(x, rate_in, delay=D)`` bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._host import BoundedCache, host_ptr, int_list, ptr as _ptr, sized, stream as _stream

__all__ = ["ratio", "plan", "out_length", "stream_delay", "resample_audio", "StreamResampler", "TILE", "MAX_FACTOR"]

TILE = L.EG_RESAMPLE_TILE                   # output samples of one workgroup of the offline kernel
MAX_FACTOR = L.EG_RESAMPLE_MAX_FACTOR


def _rate(v, who: str) -> int:
    if isinstance(v, bool) or int(v) != v or not (0 < int(v) < 2 ** 31):
        raise L.EgError(f"{who}={v!r}: a sample rate is a positive integer (Hz)")
    return int(v)


def plan(rate_in: int, rate_out: int = 16000) -> Dict[str, int]:
    """``{L, M, half, K, D, Hs, pitch, bank_floats}`` of ``rate_in -> rate_out`` (eg_resample_plan; host only).  Refuses a rate <= 0 and a
    ratio with ``max(L, M) > 640`` by name."""
    p = L.EgResamplePlan()
    L.check(L.load().eg_resample_plan(_rate(rate_in, "rate_in"), _rate(rate_out, "rate_out"), C.byref(p)), "eg_resample_plan")
    return {n: int(getattr(p, n)) for n, _t in L.EgResamplePlan._fields_}


def ratio(rate_in: int, rate_out: int = 16000):
    """``(L, M)``: up by L, down by M."""
    p = plan(rate_in, rate_out)
    return p["L"], p["M"]


def out_length(n_in: int, rate_in: int, rate_out: int = 16000) -> int:
    """``ceil(n_in * L / M)``: the samples ``n_in`` input samples give."""
    Lf, M = ratio(rate_in, rate_out)
    if int(n_in) < 0:
        raise L.EgError(f"out_length: n_in={n_in} (need >= 0)")
    return -(-int(n_in) * Lf // M)


def stream_delay(rate_in: int, rate_out: int = 16000) -> int:
    """``D = ceil(half / M)`` output samples: how far a stream's signal lags the offline one."""
    return plan(rate_in, rate_out)["D"]


def filter_taps(rate_in: int, rate_out: int = 16000) -> np.ndarray:
    """The library's fp32 taps ``[2*half + 1]`` (eg_resample_filter; host only)."""
    p = plan(rate_in, rate_out)
    h = np.zeros(2 * p["half"] + 1, np.float32)
    L.check(L.load().eg_resample_filter(int(rate_in), int(rate_out), host_ptr(h), None), "eg_resample_filter")
    return h


class _Bank:
    """The plan and the uploaded polyphase bank of one (rate_in, rate_out, device)."""

    def __init__(self, rate_in, rate_out, device):
        self.plan = plan(rate_in, rate_out)
        h = np.zeros(self.plan["bank_floats"], np.float32)
        L.check(L.load().eg_resample_filter(rate_in, rate_out, None, host_ptr(h)), "eg_resample_filter")
        self.bank = torch.from_numpy(h).to(device)

    @classmethod
    def get(cls, rate_in, rate_out, device) -> "_Bank":
        return _BANKS.get((int(rate_in), int(rate_out), str(device)), lambda: cls(int(rate_in), int(rate_out), device))


class _Lengths:
    """Host int64 lengths and their upload for one (lengths, device)."""

    def __init__(self, lengths, device):
        self.host = np.ascontiguousarray(lengths, np.int64)
        self.h_ptr = host_ptr(self.host)
        self.dev = torch.from_numpy(self.host).to(device)


_BANKS, _LENGTHS = BoundedCache(), BoundedCache(16)


def _cuda_f32(t, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.EgError(f"{who} must be a CUDA tensor (emotiongestures_amd has no CPU fallback)")
    return t.detach().to(torch.float32).contiguous()


def resample_audio(audio: torch.Tensor, rate_in: int, rate_out: int = 16000, lengths=None, delay: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``audio [T]`` or ``[U, T]`` (fp32, CUDA) at ``rate_in`` -> ``[n_out]`` / ``[U, n_out]`` at ``rate_out``, ``n_out = out_length(T)``
    (eg_resample: one launch).  ``lengths`` (U sample counts at ``rate_in``): rows of unequal length -- row u gives its own
    ``out_length(lengths[u])`` samples followed by zeros; what follows ``lengths[u]`` in its input row is never read.  ``delay``: the signal
    delayed by that many output samples (``stream_delay(rate_in)``: what a stream produces).  ``rate_in == rate_out``: the input tensor
    itself, no launch.  ``out``: a preallocated ``[U, >= n_out]`` result (graph capture)."""
    rate_in, rate_out = _rate(rate_in, "rate_in"), _rate(rate_out, "rate_out")
    b_plan = plan(rate_in, rate_out)                                            # refuses an unsupported ratio before anything else
    x = _cuda_f32(audio, "resample_audio: audio")
    if x.dim() not in (1, 2) or x.shape[-1] < 1:
        raise L.EgError(f"resample_audio: audio shape {tuple(x.shape)} != (T,) or (U, T)")
    if int(delay) < 0:
        raise L.EgError(f"resample_audio: delay={delay} (need >= 0)")
    if rate_in == rate_out and int(delay) == 0 and out is None:
        return audio
    x2 = x if x.dim() == 2 else x[None]
    U, T = x2.shape
    if lengths is None:
        lens = [T] * U
    else:
        lens = int_list(lengths)
        if len(lens) != U:
            raise L.EgError(f"resample_audio: lengths has {len(lens)} entries for {U} rows")
        if any(v < 1 or v > T for v in lens):
            raise L.EgError(f"resample_audio: lengths {lens}: every value must be in [1, {T}]")
    dev = x2.device
    bank = _Bank.get(rate_in, rate_out, dev)
    lt = _LENGTHS.get((tuple(lens), str(dev)), lambda: _Lengths(lens, dev))
    n_out = -(-max(lens) * b_plan["L"] // b_plan["M"])
    if out is None:
        y = torch.empty(U, n_out, dtype=torch.float32, device=dev)
    else:
        y = out
        if not (y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and y.dim() == 2 and y.shape[0] == U and y.shape[1] >= n_out):
            raise L.EgError(f"resample_audio: out must be a contiguous fp32 CUDA tensor [{U}, >= {n_out}]")
    L.check(L.load().eg_resample(_ptr(x2), U, T, lt.h_ptr, _ptr(lt.dev), rate_in, rate_out, _ptr(bank.bank), int(delay), _ptr(y), y.shape[1],
                                 _stream(dev)), "eg_resample")
    return y if x.dim() == 2 or out is not None else y[0]


class StreamResampler:
    """``rows`` live signals at ``rate_in`` -> ``hop_out`` samples at ``rate_out`` per push.

    ``push(chunk_in [rows, hop_in], ends_in=None) -> out [rows, hop_out]`` with ``hop_in = hop_out * M / L`` (it must be an integer, and at
    least ``Hs``).  ``ends_in[u] = m in [0, hop_in]`` (host ints or a device int32 tensor; -1: the row goes on): only the first m samples of
    row u are real, what follows is never read; the row has ``out_length(m)`` real output samples in this push, zeros after.  The pushes of
    a recording, concatenated, are ``resample_audio(x, rate_in, delay=stream_delay(rate_in))`` bit for bit.

    The history, the input chunk, ``ends`` and the output are static device buffers (``.state``, ``.chunk``, ``.ends``, ``.out``) and the
    two launches of ``run()`` do not depend on the step index, so a caller may capture ``run()`` into a graph; ``push`` copies into the
    static buffers, calls ``run()`` and returns a clone of ``out``.  ``snapshot()`` / ``restore()`` save and bring back the history."""

    def __init__(self, rows: int, rate_in: int, hop_out: int, rate_out: int = 16000, device="cuda"):
        self.rate_in, self.rate_out = _rate(rate_in, "rate_in"), _rate(rate_out, "rate_out")
        self.plan = plan(self.rate_in, self.rate_out)
        self.U, self.hop_out = int(rows), int(hop_out)
        if self.U < 1 or self.hop_out < 1:
            raise L.EgError(f"StreamResampler: rows={rows} hop_out={hop_out} (need >= 1)")
        Lf, M = self.plan["L"], self.plan["M"]
        if self.hop_out * M % Lf:
            raise L.EgError(hop_message("StreamResampler", self.hop_out, self.rate_in, self.rate_out))
        self.hop_in = self.hop_out * M // Lf
        if self.hop_in < self.plan["Hs"]:
            raise L.EgError(f"StreamResampler: hop_in={self.hop_in} < Hs={self.plan['Hs']}: a push must carry at least the filter's history "
                            f"(hop_out >= {-(-self.plan['Hs'] * Lf // M)} at {self.rate_in} Hz)")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.EgError("StreamResampler: device must be a CUDA device (emotiongestures_amd has no CPU fallback)")
        self.device = dev
        self._lib = L.load()
        self._bank = _Bank.get(self.rate_in, self.rate_out, dev)
        self.state = torch.zeros(sized("eg_resample_stream_state_bytes", self.U, self.rate_in, self.rate_out), dtype=torch.uint8, device=dev)
        self.chunk = torch.zeros(self.U, self.hop_in, dtype=torch.float32, device=dev)
        self.ends = torch.full((self.U,), -1, dtype=torch.int32, device=dev)
        self.out = torch.zeros(self.U, self.hop_out, dtype=torch.float32, device=dev)

    def run(self) -> torch.Tensor:
        """The two launches on the current stream, reading ``chunk`` / ``ends``, writing ``out`` and the history."""
        L.check(self._lib.eg_resample_stream_push(_ptr(self.state), self.U, self.rate_in, self.rate_out, _ptr(self._bank.bank), _ptr(self.chunk),
                                                  self.hop_in, _ptr(self.ends), _ptr(self.out), self.hop_out,
                                                  _stream(self.device)), "eg_resample_stream_push")
        return self.out

    def host_ends(self, ends_in) -> list:
        if ends_in is None:
            return [-1] * self.U
        if isinstance(ends_in, int):
            ends_in = [ends_in] * self.U
        e = int_list(ends_in)
        if len(e) != self.U or any(v < -1 or v > self.hop_in for v in e):
            raise L.EgError(f"ends_in: {self.U} values, each -1 (the row goes on) or in [0, {self.hop_in}] (got {e})")
        return e

    def push(self, chunk_in: torch.Tensor, ends_in=None) -> torch.Tensor:
        x = _cuda_f32(chunk_in, "StreamResampler.push: chunk_in")
        if tuple(x.shape) != (self.U, self.hop_in):
            raise L.EgError(f"chunk_in shape {tuple(x.shape)} != ({self.U},{self.hop_in})")
        if isinstance(ends_in, torch.Tensor) and ends_in.is_cuda:
            self.ends.copy_(ends_in)
        else:
            self.ends.copy_(torch.tensor(self.host_ends(ends_in), dtype=torch.int32))
        self.chunk.copy_(x, non_blocking=True)
        return self.run().clone()

    def reset(self, rows: Optional[Sequence[int]] = None) -> None:
        """Rows ``rows`` (None: all) start a new signal: their history is zeroed."""
        mask = None
        if rows is not None:
            sel = sorted({int(r) for r in rows})
            if not sel or sel[0] < 0 or sel[-1] >= self.U:
                raise L.EgError(f"reset: rows {sel} of a resampler of {self.U}")
            m = torch.zeros(self.U, dtype=torch.int32)
            m[sel] = 1
            mask = m.to(self.device)
        L.check(self._lib.eg_resample_stream_reset(_ptr(self.state), self.U, self.rate_in, self.rate_out, _ptr(mask),
                                                   _stream(self.device)), "eg_resample_stream_reset")

    def snapshot(self) -> torch.Tensor:
        return self.state.clone()

    def restore(self, snap: torch.Tensor) -> None:
        self.state.copy_(snap)


def hop_message(who: str, hop_out: int, rate_in: int, rate_out: int = 16000) -> str:
    """The refusal of a hop that does not carry a whole number of input samples, with the nearest values that do."""
    Lf, M = ratio(rate_in, rate_out)
    step = Lf // np.gcd(Lf, M)                                                  # hop_out * M / L integer <=> hop_out a multiple of L (gcd(L, M) = 1)
    lo, hi = hop_out // step * step, -(-hop_out // step) * step
    near = f"{hi}" if lo < 1 else f"{lo} or {hi}"
    return (f"{who}: hop_samples={hop_out} at audio_rate={rate_in} is {hop_out} * {M} / {Lf} = {hop_out * M / Lf:.4f} input samples per push, not "
            f"an integer: hop_samples must be a multiple of {step} (nearest: {near})")
