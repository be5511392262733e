"""Smoothed output: a Savitzky-Golay filter along the time axis of whole gesture tracks (csrc/smooth.hip).

The generator emits 15 fps poses window by window; frame-to-frame jitter and the window seams show on an avatar, and the step every consumer
runs before a renderer sees a track is a temporal low-pass -- by convention ``scipy.signal.savgol_filter``.  Here it stays on the device:

``Smoother(window, polyorder, deriv=0, fps=15)``   the filter: the table ``C[K][K]`` in float64 (``.table``) and fp32, uploaded once per device
``smooth_tracks(track, smoother, frames=None)``    ``[T, D]``, ``[U, T, D]`` or ``[U, R, T, D]`` -> the same shape, every recording filtered over
                                                   its own ``frames[u]`` valid frames, zeros behind them
``StreamSmoother(rows, H, D, smoother)``           the same filter on tracks that arrive H frames per step (``GestureStream(smooth=)``)

Definition (include/emogest.h).  ``K`` odd, ``3 <= K <= 31``; ``1 <= polyorder <= min(5, K - 1)``; ``0 <= deriv <= min(2, polyorder)``;
``half = K // 2``.  Row i of the table holds the weights that give the ``deriv``-th derivative at window position i of the least-squares
polynomial through K equally spaced samples.  For a row with ``n >= K`` valid frames: ``y[i] = C[i] . x[0:K]`` for ``i < half``,
``y[i] = C[half] . x[i - half : i + half + 1]`` in the interior, ``y[i] = C[K - (n - i)] . x[n - K : n]`` for ``i >= n - half``: exactly
``scipy.signal.savgol_filter(x, K, polyorder, deriv=deriv, delta=1 / fps, axis=0, mode="interp")``.  Frames from n on are zeros in the output
and never read in the input (they may hold NaN).  A recording with fewer than K valid frames is refused by name: there is no shrinking window.

CUDA tensors go through the kernel (fp32, one launch; no eager-PyTorch fallback).  numpy arrays and CPU tensors take the definition in float64
numpy with the float64 table, as ``skeleton.joints_from_tracks`` does, so the filter can be checked and used without a GPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import _rows as RW
from ._host import BoundedCache, host_ptr, ptr as _ptr, sized, stream as _stream

__all__ = ["Smoother", "smooth_tracks", "launch_smooth", "StreamSmoother", "MAX_WINDOW", "TILE_FRAMES", "TILE_COLS"]

MAX_WINDOW = L.EG_SMOOTH_MAX_WINDOW
TILE_FRAMES = L.EG_SMOOTH_TILE_FRAMES        # frames of one workgroup
TILE_COLS = L.EG_SMOOTH_TILE_COLS            # columns of one workgroup


class Smoother:
    """The filter ``(window, polyorder, deriv, delta = 1 / fps)``; eg_smooth_design refuses a bad one by name.  ``table``: float64 ``[K, K]``;
    ``table32``: the same rounded once to fp32 -- what the device reads, uploaded once per device."""

    def __init__(self, window: int, polyorder: int, deriv: int = 0, fps: float = 15):
        for name, v in (("window", window), ("polyorder", polyorder), ("deriv", deriv)):
            if isinstance(v, bool) or int(v) != v:
                raise L.EgError(f"Smoother: {name}={v!r}: an integer")
        self.window, self.polyorder, self.deriv, self.fps = int(window), int(polyorder), int(deriv), float(fps)
        if not self.fps > 0:
            raise L.EgError(f"Smoother: fps={fps!r}: delta = 1 / fps must be finite and > 0")
        self.delta = 1.0 / self.fps
        K = self.window if 0 < self.window <= MAX_WINDOW else 1          # a refused window writes nothing
        self.table = np.zeros((K, K), np.float64)
        self.table32 = np.zeros((K, K), np.float32)
        L.check(L.load().eg_smooth_design(self.window, self.polyorder, self.deriv, self.delta, host_ptr(self.table), host_ptr(self.table32)),
                "eg_smooth_design")
        self.half = self.window // 2
        self._tables = BoundedCache()

    @classmethod
    def of(cls, smooth, who: str = "smooth", fps: float = 15) -> "Smoother":
        """A Smoother as it is; ``(window, polyorder)`` or ``(window, polyorder, deriv)``: one at ``fps``."""
        if isinstance(smooth, Smoother):
            return smooth
        try:
            args = tuple(smooth)
        except TypeError:
            args = ()
        if len(args) not in (2, 3):
            raise L.EgError(f"{who}={smooth!r}: a smooth.Smoother or (window, polyorder)")
        return cls(*args, fps=fps)

    def device_table(self, device) -> torch.Tensor:
        """fp32 ``[K, K]`` on ``device`` (16-byte aligned: an allocation of its own)."""
        return self._tables.get(str(device), lambda: torch.from_numpy(self.table32).to(device))

    def __repr__(self):
        return f"Smoother(window={self.window}, polyorder={self.polyorder}, deriv={self.deriv}, fps={self.fps:g})"


def _smooth64(v: np.ndarray, table: np.ndarray, frames: List[int]) -> np.ndarray:
    """The definition: v [B, T, D] float64, table [K, K] float64, frames [B] (each >= K) -> [B, T, D]."""
    K = table.shape[0]
    half = K // 2
    out = np.zeros_like(v)
    for b, n in enumerate(frames):
        x = v[b, :n]
        for i in range(half):
            out[b, i] = table[i] @ x[:K]
            out[b, n - half + i] = table[half + 1 + i] @ x[n - K:]
        win = np.lib.stride_tricks.sliding_window_view(x, K, axis=0)         # [n - K + 1, D, K]
        out[b, half:n - half] = win @ table[half]
    return out


def launch_smooth(track: torch.Tensor, sm: Smoother, frames: Optional[Sequence[int]] = None, d_frames: Optional[torch.Tensor] = None,
                  draws: int = 1, frame_unit: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_smooth_tracks on ``track [B, T, D]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``[B, T, D]``: one launch on the current stream,
    nothing else (the table is uploaded on first use per device: warm up before a capture).  ``frames``: host ints ``[B / draws]`` and
    ``d_frames`` their device int32 copy, both or neither."""
    B, T, D = track.shape
    if out is None:
        out = torch.empty_like(track)
    fr = RW.counts32(frames)
    L.check(L.load().eg_smooth_tracks(_ptr(track), B, T, D, sm.window, _ptr(sm.device_table(track.device)), host_ptr(fr), _ptr(d_frames),
                                      int(draws), int(frame_unit), _ptr(out), _stream(track.device)), "eg_smooth_tracks")
    return out


def smooth_tracks(track, smoother, frames=None):
    """``track [..., T, D]`` with up to two leading axes (``[T, D]``, ``[U, T, D]``, ``[U, R, T, D]``) -> the smoothed track (or, with
    ``smoother.deriv`` 1 or 2, its smoothed velocity / acceleration per second) in the same shape.

    ``smoother``: a ``Smoother`` or ``(window, polyorder)``.  ``frames``: valid frames per recording (``[U]`` host ints, shared by the R draws
    of a recording; one value for ``[T, D]``): frames from ``frames[u]`` on are never read, the output is zeros there.  A recording with
    fewer valid frames than the window is refused by name.

    A CUDA tensor: one kernel launch, fp32 CUDA result.  numpy or a CPU tensor: the definition in float64 (numpy in: numpy out; tensor in:
    float64 tensor out)."""
    who = "smooth_tracks"
    sm = Smoother.of(smoother, f"{who}: smoother")
    shape = tuple(track.shape)
    if len(shape) < 2 or shape[-2] < 1 or shape[-1] < 1:
        raise L.EgError(f"{who}: track shape {shape}: need [..., T >= 1, D >= 1]")
    return RW.front(track, 2, frames, who, lambda x, fr, d_frames, R: launch_smooth(x, sm, fr, d_frames, R),
                    lambda v, per_row: _smooth64(v, sm.table, per_row), sm.window,
                    f"window={sm.window} (there is no shrinking window)").res.reshape(shape)


class StreamSmoother:
    """The filter on ``rows`` tracks that arrive ``H`` frames per step (include/emogest.h: eg_smooth_stream_*).

    ``run(chunk [rows, H, D], valid int32 [rows] | None) -> out [rows, H, D]``: for a valid row in its s-th valid step the smoothed frames
    ``[sH - half, (s + 1)H - half)`` of its track -- the output runs ``delay = half`` frames behind the input, and the first ``half`` entries of
    step 0 are zeros; zeros for a row that is not valid, whose state stays.  ``tail(tail_rows [rows, P, D]) -> [rows, P + half, D]``: the last
    frames, given the last P raw ones.  The pushes of a row, concatenated after dropping step 0's leading zeros, followed by the tail, are
    ``smooth_tracks`` on the finished track bit for bit.

    The state and ``out`` are static device buffers and the two launches of ``run`` do not depend on the step index, so a caller may capture
    ``run`` into a graph (the device table is uploaded here, before any capture).  ``snapshot()`` / ``restore()`` save and bring back the state."""

    def __init__(self, rows: int, H: int, D: int, smoother, device="cuda"):
        self.sm = Smoother.of(smoother, "StreamSmoother: smoother")
        self.U, self.H, self.D = int(rows), int(H), int(D)
        if self.sm.deriv != 0:
            raise L.EgError(f"StreamSmoother: deriv={self.sm.deriv}: a stream smooths poses; take derivatives of the finished track with smooth_tracks")
        if self.sm.window > self.H:
            raise L.EgError(f"StreamSmoother: window={self.sm.window} > H={self.H} frames per step (the head rows need x[0 .. window) inside "
                            "the first chunk)")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.EgError("StreamSmoother: device must be a CUDA device (emotiongestures_amd has no CPU fallback)")
        self.device, self.delay = dev, self.sm.half
        self._lib = L.load()
        self.state = torch.zeros(sized("eg_smooth_stream_state_bytes", self.U, self.D, self.sm.window), dtype=torch.uint8, device=dev)
        self.out = torch.zeros(self.U, self.H, self.D, dtype=torch.float32, device=dev)
        self._table = self.sm.device_table(dev)

    def run(self, chunk: torch.Tensor, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The two launches on the current stream: ``out``, then the new history and counts."""
        L.check(self._lib.eg_smooth_stream_push(_ptr(self.state), self.U, self.H, self.D, self.sm.window, _ptr(self._table), _ptr(chunk),
                                                _ptr(valid), _ptr(self.out), _stream(self.device)), "eg_smooth_stream_push")
        return self.out

    def tail(self, tail_rows: torch.Tensor) -> torch.Tensor:
        P = int(tail_rows.shape[1])
        out = torch.empty(self.U, P + self.delay, self.D, dtype=torch.float32, device=self.device)
        L.check(self._lib.eg_smooth_stream_tail(_ptr(self.state), self.U, P, self.D, self.sm.window, _ptr(self._table),
                                                _ptr(tail_rows.contiguous()), _ptr(out), _stream(self.device)), "eg_smooth_stream_tail")
        return out

    def reset(self, rows: Optional[Sequence[int]] = None) -> None:
        """Rows ``rows`` (None: all) start a new track: history and count to zero."""
        mask = None
        if rows is not None:
            sel = sorted({int(r) for r in rows})
            if not sel or sel[0] < 0 or sel[-1] >= self.U:
                raise L.EgError(f"reset: rows {sel} of a smoother of {self.U}")
            m = torch.zeros(self.U, dtype=torch.int32)
            m[sel] = 1
            mask = m.to(self.device)
        L.check(self._lib.eg_smooth_stream_reset(_ptr(self.state), self.U, self.D, self.sm.window, _ptr(mask), _stream(self.device)),
                "eg_smooth_stream_reset")

    def snapshot(self) -> torch.Tensor:
        return self.state.clone()

    def restore(self, snap: torch.Tensor) -> None:
        self.state.copy_(snap)
