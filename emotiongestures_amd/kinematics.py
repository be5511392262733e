"""Motion statistics of whole tracks: mean speed, acceleration and jerk per joint and a histogram of the joint speeds (csrc/kinematics.hip).

The standard kinematic figures of the gesture-generation literature, in metres and seconds, from the joint positions the output stage already
holds on the device: how much a track jitters (jerk), how fast it moves (speed), and how its speeds are distributed -- compared between two
sets of tracks (generated against captured, raw against smoothed, one checkpoint against another) by the Hellinger distance of the histograms.

``SpeedBins(edges=None, fps=15)``                       the histogram's bin edges in m/s at a frame rate (default 0, 0.05 .. 2.0: 40 bins)
``kinematics_of_joints(joints, fps, frames=None, edges=None)``   ``[T, J, 3]``, ``[U, T, J, 3]`` or ``[U, R, T, J, 3]`` -> the dict below
``launch_kinematics(joints [rows, T, J, 3], bins, frames, ...)``  eg_kin_stats, nothing but the launches (capturable)
``hellinger(hist_a, hist_b, pool=False)``               the distance of two histograms over their last axis

Definition (include/emogest.h).  ``p [T, J, 3]`` fp32 metres with n valid frames.  Differences in fp32, one IEEE subtraction each:
``d1[t] = p[t+1] - p[t]`` (t < n - 1), ``d2[t] = d1[t+1] - d1[t]`` (t < n - 2), ``d3[t] = d2[t+1] - d2[t]`` (t < n - 3).  Squared magnitudes
``s2_k[t, j] = (x*x + y*y) + z*z`` in float64 of the widened components (every square exact).  ``speed``, ``accel``, ``jerk``:
``(sum_t sqrt(s2_k[t, j])) * fps**k / (n - k)`` for k = 1, 2, 3, in m/s, m/s^2, m/s^3, float64.  Histogram: ``edges2 = (edges / fps)**2`` on
the host; speed sample (t, j) falls into bin e when ``edges2[e] <= s2_1 < edges2[e+1]`` (on an edge: the upper bin) and into the overflow when
``s2_1 >= edges2[B]`` -- no square root and no division for binning, so the counts are exact: ``speed_hist[j].sum() + speed_over[j] == n - 1``.
Frames from n on are never read (they may hold NaN).  A recording with fewer than 4 valid frames is refused by name.

CUDA tensors go through the kernel (no eager-PyTorch fallback).  numpy arrays and CPU tensors take the definition in numpy, as every
output-stage function does, so the figures can be checked and used without a GPU; the histograms of the two paths are equal and the means agree
to the rounding of a float64 sum.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import _rows as RW
from ._host import BoundedCache, device_bytes, host_ptr, ptr as _ptr, stream as _stream

__all__ = ["SpeedBins", "kinematics_of_joints", "launch_kinematics", "hellinger", "MAX_JOINTS", "MAX_BINS", "TILE_FRAMES"]

MAX_JOINTS = L.EG_KIN_MAX_JOINTS
MAX_BINS = L.EG_KIN_MAX_BINS
TILE_FRAMES = L.EG_KIN_TILE_FRAMES           # difference indices of one workgroup
NAMES = ("speed", "accel", "jerk")


class SpeedBins:
    """The speed histogram's bins: ``edges`` (B + 1 ascending float64 values in m/s, ``edges[0] == 0``, 1 <= B <= 256; default
    ``k / 20`` for k = 0 .. 40) at ``fps`` frames per second.  eg_kin_edges2 refuses a bad one by name.  ``edges2``: float64
    ``(edges / fps) ** 2``, the squared per-frame steps the kernel compares against, uploaded once per device."""

    def __init__(self, edges=None, fps: float = 15):
        self.fps = float(fps)
        e = np.arange(41, dtype=np.float64) / 20.0 if edges is None else np.array(edges, dtype=np.float64).reshape(-1)
        self.edges = np.ascontiguousarray(e)
        self.edges2 = np.zeros_like(self.edges)
        L.check(L.load().eg_kin_edges2(host_ptr(self.edges), self.edges.size, self.fps, host_ptr(self.edges2)), "eg_kin_edges2")
        self.bins = self.edges.size - 1
        self._tables = BoundedCache()

    @classmethod
    def of(cls, kinematics, who: str = "kinematics", fps: float = 15) -> "SpeedBins":
        """A SpeedBins as it is -- its rate must be ``fps`` --; ``True`` or ``None``: the default edges at ``fps``; anything else: edges."""
        if isinstance(kinematics, SpeedBins):
            if kinematics.fps != float(fps):
                raise L.EgError(f"{who}: the SpeedBins are at fps={kinematics.fps:g}, the joints at fps={float(fps):g}")
            return kinematics
        if kinematics is False:
            raise L.EgError(f"{who}=False: None, True, bin edges or a kinematics.SpeedBins")
        return cls(None if kinematics is None or kinematics is True else kinematics, fps)

    def table(self, device) -> torch.Tensor:
        """float64 ``edges2 [B + 1]`` on ``device`` (an allocation of its own)."""
        return self._tables.get(str(device), lambda: torch.from_numpy(self.edges2).to(device))

    def __repr__(self):
        return f"SpeedBins(bins={self.bins}, {self.edges[0]:g}..{self.edges[-1]:g} m/s, fps={self.fps:g})"


def _stats_host(p: np.ndarray, frames: Sequence[int], edges2: np.ndarray, fps: float):
    """The definition: p [rows, T, J, 3] float32, frames [rows] (each >= 4) -> mean [rows, 3, J] float64, hist [rows, J, B + 1] int32."""
    rows, _T, J, _ = p.shape
    E = edges2.size
    mean = np.zeros((rows, 3, J), np.float64)
    hist = np.zeros((rows, J, E), np.int32)
    cols = np.arange(J)[None, :]
    for b, n in enumerate(frames):
        d = p[b, :n]
        for k in range(3):
            d = d[1:] - d[:-1]                                               # float32
            w = d.astype(np.float64)
            s2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
            mean[b, k] = np.sqrt(s2).sum(0) * fps ** (k + 1) / (n - 1 - k)
            if k == 0:
                at = cols * E + (np.searchsorted(edges2, s2, side="right") - 1)    # on an edge: the upper bin; from the last edge on: column B
                hist[b] = np.bincount(at.reshape(-1), minlength=J * E).reshape(J, E)
    return mean, hist


def launch_kinematics(joints: torch.Tensor, bins: SpeedBins, frames: Optional[Sequence[int]] = None, d_frames: Optional[torch.Tensor] = None,
                      draws: int = 1, frame_unit: int = 1, workspace: Optional[torch.Tensor] = None, out=None,
                      edges2: Optional[torch.Tensor] = None):
    """eg_kin_stats on ``joints [rows, T, J, 3]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``(mean [rows, 3, J] float64,
    hist [rows, J, B + 1] int32)``: three launches on the current stream (hist = 0, the tiles, the means), nothing else (the table is uploaded on first use
    per device, and the buffers are allocated unless given: warm up before a capture).  ``frames``: host ints ``[rows / draws]`` and
    ``d_frames`` their device int32 copy, both or neither.  ``workspace``: a uint8 tensor of eg_kin_workspace_bytes; ``out``: ``(mean,
    hist)`` to write into; ``edges2``: a device float64 table ``[B + 1]`` in place of ``bins.table(device)``."""
    rows, T, J, _three = joints.shape
    table = bins.table(joints.device) if edges2 is None else edges2
    B = int(table.numel()) - 1
    if workspace is None:
        workspace = device_bytes("eg_kin_workspace_bytes", joints.device, rows, T, J, B)
    if out is None:
        out = (torch.empty(rows, 3, J, dtype=torch.float64, device=joints.device),
               torch.empty(rows, J, B + 1, dtype=torch.int32, device=joints.device))
    mean, hist = out
    fr = RW.counts32(frames)
    L.check(L.load().eg_kin_stats(_ptr(joints), rows, T, J, host_ptr(fr), _ptr(d_frames), int(draws), int(frame_unit), bins.fps, _ptr(table), B,
                                  _ptr(workspace), int(workspace.numel()), _ptr(mean), _ptr(hist), _stream(joints.device)), "eg_kin_stats")
    return mean, hist


def kinematics_of_joints(joints, fps, frames=None, edges=None) -> dict:
    """``joints [..., T, J, 3]`` in metres with up to two leading axes (``[T, J, 3]``, ``[U, T, J, 3]``, ``[U, R, T, J, 3]``) at ``fps`` frames
    per second -> ``{"speed", "accel", "jerk"}`` each ``[..., J]`` float64 (m/s, m/s^2, m/s^3: the means over the recording's valid frames),
    ``"speed_hist" [..., J, B]`` and ``"speed_over" [..., J]`` int32 (the counts per bin and at or above the last edge) and ``"edges" [B + 1]``
    (float64 numpy, m/s).

    ``frames``: valid frames per recording (``[U]`` host ints, shared by the R draws of a recording; one value for ``[T, J, 3]``): frames
    from ``frames[u]`` on are never read.  A recording with fewer than 4 valid frames is refused by name.  ``edges``: bin edges in m/s or a
    ``SpeedBins`` at ``fps``; ``None``: 0, 0.05 .. 2.0.

    A CUDA tensor: one call of the kernel, CUDA results.  numpy or a CPU tensor: the definition in numpy (numpy in: numpy out; tensor in:
    tensors out)."""
    who = "kinematics_of_joints"
    bins = SpeedBins.of(edges, f"{who}: edges", fps)
    shape = tuple(joints.shape)
    if len(shape) < 3 or shape[-1] != 3 or not 1 <= shape[-2] <= MAX_JOINTS:
        raise L.EgError(f"{who}: joints shape {shape}: need [..., T, J, 3] with 1 <= J <= {MAX_JOINTS}")
    fe = RW.front(joints, 3, frames, who, lambda x, fr, d_frames, R: launch_kinematics(x, bins, fr, d_frames, R),
                  lambda x, per_row: _stats_host(x, per_row, bins.edges2, bins.fps), 4, "4 (the jerk reads four positions)", RW.host32)
    (mean, hist), lead, J = fe.res, fe.lead, shape[-2]
    res = {name: mean[:, k].reshape(lead + (J,)) for k, name in enumerate(NAMES)}
    res["speed_hist"] = hist[:, :, :bins.bins].reshape(lead + (J, bins.bins))
    res["speed_over"] = hist[:, :, bins.bins].reshape(lead + (J,))
    res["edges"] = bins.edges.copy()
    return res


def hellinger(hist_a, hist_b, pool: bool = False):
    """The Hellinger distance ``sqrt(max(0, 1 - sum_b sqrt(p_b q_b)))`` of two histograms of counts over their last axis, with
    ``p = hist / hist.sum()``: 0 for equal distributions, 1 for disjoint ones.  float64; tensors (any device, a few small ops there) or
    numpy arrays, of one shape ``[..., B]``.  ``pool=True``: the counts are summed over the joint axis (the one before the last) first.  An
    empty histogram on either side is refused by name."""
    who = "hellinger"
    if tuple(hist_a.shape) != tuple(hist_b.shape) or len(hist_a.shape) < (2 if pool else 1):
        raise L.EgError(f"{who}: histograms of shapes {tuple(hist_a.shape)} and {tuple(hist_b.shape)}: need one shape [..., {'J, ' if pool else ''}B]")
    on_torch = isinstance(hist_a, torch.Tensor)
    if on_torch != isinstance(hist_b, torch.Tensor):
        raise L.EgError(f"{who}: one histogram is a tensor and the other is not")
    xp = torch if on_torch else np
    a, b = (h.to(torch.float64) if on_torch else np.asarray(h, np.float64) for h in (hist_a, hist_b))
    if pool:
        a, b = a.sum(-2), b.sum(-2)
    na, nb = a.sum(-1), b.sum(-1)
    for name, n in (("hist_a", na), ("hist_b", nb)):
        if bool((n <= 0).any()):
            raise L.EgError(f"{who}: {name} holds an empty histogram (no counts: no distribution)")
    # sum_b sqrt(p_b q_b) with the two normalisations taken out of the sum: on counts, a histogram against itself gives exactly 1
    gap = 1.0 - xp.sqrt(a * b).sum(-1) / xp.sqrt(na * nb)
    return xp.sqrt(torch.clamp(gap, min=0.0) if on_torch else np.maximum(gap, 0.0))
