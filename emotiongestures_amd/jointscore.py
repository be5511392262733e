"""Joint-space scores of whole tracks: SRGR (semantic-relevant gesture recall) and L1 diversity, the two figures of the BEAT papers' table
that start from joint positions (the reference's ``model/Beat_score_v2.py``: ``SRGR``, ``L1div``), per track of a batch (csrc/jointscore.hip).

``srgr_of_joints(joints, targets, semantic=None, frames=None, threshold=0.1, scale=1/0.165)``   ``[T, J, 3]``, ``[U, T, J, 3]`` or ``[U, R, T, J, 3]``
``l1div_of_tracks(x, frames=None)``                         ``[T, D]``, ``[U, T, D]`` or ``[U, R, T, D]`` -> the dicts below
``launch_srgr`` / ``launch_l1div``                          eg_srgr_tracks / eg_l1div_tracks, nothing but the launches (capturable)
``SemanticTargets(joints, semantic=None, threshold=0.1)``   the ``srgr=`` argument of ``harness.synthesize`` / ``synthesize_takes``
``SRGR(threshold=0.1, joints=47)`` / ``L1div()``            the reference's classes: ``run`` ... ``avg``, and ``push`` for the dicts

Definition (include/emogest.h).  A row has n valid frames; frames from n on are never read (they may hold NaN).
SRGR: ``d[t, j] = (|rx - gx| + |ry - gy|) + |rz - gz|`` -- fp32 subtractions, the absolute values widened to float64 and added in that order --;
a hit is ``d < threshold`` (equal: a miss; NaN: a miss); ``hits[j] = sum_t hit``; ``srgr = (sum_t w[t] * sum_j hit[t, j]) * scale / (n J)`` in
float64, the sum over the frames of a tile of ``TILE_FRAMES`` in ascending order, then over the tiles; ``recall = hits.sum() / (n J)``.  With
``scale = 1 / 0.165`` (the default) ``srgr`` is the reference's rate.
L1 diversity: ``mean[c] = (sum_t x[t, c]) / n``, ``l1_sum = sum_t sum_c |x[t, c] - mean[c]|``, ``l1div = l1_sum / n``, in float64 of the fp32
values.  The input is never written (the reference's ``L1div.run`` overwrites its argument).

CUDA tensors go through the kernels (no eager-PyTorch fallback).  numpy arrays and CPU tensors take the definition in numpy, as every
output-stage function does: the hits of the two paths are equal, ``srgr`` is added in the kernel's order, and the L1 figures agree to the
rounding of a float64 sum.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import _rows as RW
from ._host import device_bytes, host_ptr, ptr as _ptr, stream as _stream

__all__ = ["srgr_of_joints", "l1div_of_tracks", "launch_srgr", "launch_l1div", "SemanticTargets", "SRGR", "L1div", "MAX_JOINTS", "MAX_COLS",
           "TILE_FRAMES", "SCALE"]

MAX_JOINTS = L.EG_SRGR_MAX_JOINTS
MAX_COLS = L.EG_L1DIV_MAX_COLS
TILE_FRAMES = L.EG_JOINTSCORE_TILE_FRAMES     # frames of one workgroup: the unit of the summation order
SCALE = 1 / 0.165                             # the reference's normaliser ("srgr == 0.165 when all success")


# ---- the definition in numpy ---------------------------------------------------------------------------------------------------------------
def _srgr_host(r: np.ndarray, g: np.ndarray, w: Optional[np.ndarray], frames: Sequence[int], draws: int, threshold: float, scale: float):
    """r [rows, T, J, 3], g [rows / draws, T, J, 3] float32, w [rows / draws, T] float32 or None, frames [rows] (each >= 1) ->
    srgr [rows], recall [rows] float64, hits [rows, J] int32."""
    rows, _T, J, _ = r.shape
    srgr, recall, hits = np.zeros(rows, np.float64), np.zeros(rows, np.float64), np.zeros((rows, J), np.int32)
    for b, n in enumerate(frames):
        u = b // draws
        a = np.abs(r[b, :n] - g[u, :n]).astype(np.float64)                   # float32 subtraction, then widened
        hit = ((a[..., 0] + a[..., 1]) + a[..., 2]) < threshold
        hits[b] = hit.sum(0)
        v = hit.sum(1).astype(np.float64) * (1.0 if w is None else w[u, :n].astype(np.float64))      # exact products
        tiles = -(-n // TILE_FRAMES)
        v = np.concatenate([v, np.zeros(tiles * TILE_FRAMES - n)]).reshape(tiles, TILE_FRAMES)
        weighted = np.cumsum(np.cumsum(v, 1)[:, -1])[-1]                     # ascending inside a tile, then ascending over the tiles
        srgr[b] = weighted * scale / (float(n) * float(J))
        recall[b] = float(hits[b].sum(dtype=np.int64)) / (float(n) * float(J))
    return srgr, recall, hits


def _l1_host(x: np.ndarray, frames: Sequence[int]):
    """x [rows, T, D] float32, frames [rows] (each >= 1) -> mean [rows, D], l1_sum [rows], l1div [rows] float64."""
    rows, _T, D = x.shape
    mean, l1 = np.zeros((rows, D), np.float64), np.zeros(rows, np.float64)
    for b, n in enumerate(frames):
        v = x[b, :n].astype(np.float64)
        mean[b] = v.sum(0) / n
        l1[b] = np.abs(v - mean[b]).sum()
    return mean, l1, l1 / np.asarray(frames, np.float64)


# ---- the launches --------------------------------------------------------------------------------------------------------------------------
def launch_srgr(joints: torch.Tensor, targets: torch.Tensor, semantic: Optional[torch.Tensor] = None, frames: Optional[Sequence[int]] = None,
                d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1, threshold: float = 0.1, scale: float = SCALE,
                workspace: Optional[torch.Tensor] = None, out=None):
    """eg_srgr_tracks on ``joints [rows, T, J, 3]``, ``targets [rows / draws, T, J, 3]`` and ``semantic [rows / draws, T]`` or ``None``
    (weights of 1) -- contiguous fp32 CUDA, 16-byte aligned -- -> ``(srgr [rows] float64, recall [rows] float64, hits [rows, J] int32)``:
    two launches on the current stream, nothing else (the buffers are allocated unless given: warm up before a capture).  ``frames``: host
    ints ``[rows / draws]`` and ``d_frames`` their device int32 copy, both or neither.  ``workspace``: a uint8 tensor of
    eg_srgr_workspace_bytes; ``out``: ``(srgr, recall, hits)`` to write into."""
    rows, T, J, _three = joints.shape
    dev = joints.device
    if workspace is None:
        workspace = device_bytes("eg_srgr_workspace_bytes", dev, rows, T, J)
    if out is None:
        out = (torch.empty(rows, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.float64, device=dev),
               torch.empty(rows, J, dtype=torch.int32, device=dev))
    srgr, recall, hits = out
    fr = RW.counts32(frames)
    L.check(L.load().eg_srgr_tracks(_ptr(joints), _ptr(targets), _ptr(semantic), rows, T, J, host_ptr(fr), _ptr(d_frames), int(draws),
                                    int(frame_unit), float(threshold), float(scale), _ptr(workspace), int(workspace.numel()), _ptr(srgr),
                                    _ptr(recall), _ptr(hits), _stream(dev)), "eg_srgr_tracks")
    return srgr, recall, hits


def launch_l1div(x: torch.Tensor, frames: Optional[Sequence[int]] = None, d_frames: Optional[torch.Tensor] = None, draws: int = 1,
                 frame_unit: int = 1, workspace: Optional[torch.Tensor] = None, out=None):
    """eg_l1div_tracks on ``x [rows, T, D]`` (contiguous fp32 CUDA, 16-byte aligned; never written) -> ``(mean [rows, D], l1_sum [rows],
    l1div [rows])`` float64: four launches on the current stream (column sums, means, deviations, finalise), nothing else.  ``frames``,
    ``d_frames``, ``workspace`` (eg_l1div_workspace_bytes) and ``out = (mean, l1_sum, l1div)`` as in ``launch_srgr``."""
    rows, T, D = x.shape
    dev = x.device
    if workspace is None:
        workspace = device_bytes("eg_l1div_workspace_bytes", dev, rows, T, D)
    if out is None:
        out = (torch.empty(rows, D, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.float64, device=dev),
               torch.empty(rows, dtype=torch.float64, device=dev))
    mean, l1_sum, l1div = out
    fr = RW.counts32(frames)
    L.check(L.load().eg_l1div_tracks(_ptr(x), rows, T, D, host_ptr(fr), _ptr(d_frames), int(draws), int(frame_unit), _ptr(workspace),
                                     int(workspace.numel()), _ptr(mean), _ptr(l1_sum), _ptr(l1div), _stream(dev)), "eg_l1div_tracks")
    return mean, l1_sum, l1div


# ---- the front ends ------------------------------------------------------------------------------------------------------------------------
def _finite(value, name: str, who: str) -> float:
    v = float(value)
    if not np.isfinite(v):
        raise L.EgError(f"{who}: {name}={v:g} is not finite")
    return v


def _same_side(a, b, name: str, who: str):
    if b is not None and RW.is_cuda(a) != RW.is_cuda(b):
        raise L.EgError(f"{who}: joints and {name} are not on one side (a CUDA tensor goes with CUDA tensors, host data with host data)")


def srgr_of_joints(joints, targets, semantic=None, frames=None, threshold: float = 0.1, scale: float = SCALE) -> dict:
    """``joints [..., T, J, 3]`` with up to two leading axes (``[T, J, 3]``, ``[U, T, J, 3]``, ``[U, R, T, J, 3]``) against ``targets``
    ``[T, J, 3]`` / ``[U, T, J, 3]`` -- one target per recording, shared by its R takes -- and the semantic weights ``semantic`` ``[T]`` /
    ``[U, T]`` (``None``: weights of 1) -> ``{"srgr", "recall"}`` each ``[...]`` float64, ``"hits" [..., J]`` int32 (the frames on which joint
    j lies within ``threshold`` of its target, in the L1 distance of the three coordinates) and ``"frames" [...]`` (host int64 numpy: the valid
    frames n of every row, the weight of the row in a pooled figure).  ``srgr = (sum_t semantic[t] * hits of frame t) * scale / (n J)``; with
    the default ``scale = 1 / 0.165`` it is the reference's ``SRGR.run`` rate of the track; ``recall`` is the unweighted share of hits.

    ``frames``: valid frames per recording (``[U]`` host ints, shared by the R takes; one value for ``[T, J, 3]``): frames from ``frames[u]``
    on are never read.  A recording without a valid frame is refused by name.

    CUDA tensors: one call of the kernel, CUDA results.  numpy or CPU tensors: the definition in numpy (numpy in: numpy out; tensor in:
    tensors out)."""
    who = "srgr_of_joints"
    shape = tuple(joints.shape)
    if len(shape) < 3 or shape[-1] != 3 or not 1 <= shape[-2] <= MAX_JOINTS or shape[-3] < 1:
        raise L.EgError(f"{who}: joints shape {shape}: need [..., T >= 1, J, 3] with 1 <= J <= {MAX_JOINTS}")
    lead, U, R = RW.lead_axes(shape, 3, who)
    T, J = shape[-3], shape[-2]
    want = lead[:1] + (T, J, 3)
    if tuple(targets.shape) != want:
        raise L.EgError(f"{who}: targets shape {tuple(targets.shape)}: joints {shape} take {want} (one target per recording)")
    if semantic is not None and tuple(semantic.shape) != lead[:1] + (T,):
        raise L.EgError(f"{who}: semantic shape {tuple(semantic.shape)}: joints {shape} take {lead[:1] + (T,)} (one weight per frame)")
    _same_side(joints, targets, "targets", who)
    _same_side(joints, semantic, "semantic", who)
    threshold, scale = _finite(threshold, "threshold", who), _finite(scale, "scale", who)
    def on_device(x, fr, d_frames, _R):
        g = RW.dev32(targets.to(x.device)).reshape(U, T, J, 3)
        w = None if semantic is None else RW.dev32(semantic.to(x.device)).reshape(U, T)
        return launch_srgr(x, g, w, fr, d_frames, R, 1, threshold, scale)

    def on_host(x, per_row):
        w = None if semantic is None else RW.host32(semantic).reshape(U, T)
        return _srgr_host(x, RW.host32(targets).reshape(U, T, J, 3), w, per_row, R, threshold, scale)

    fe = RW.front(joints, 3, frames, who, on_device, on_host, 1, "1", RW.host32)
    srgr, recall, hits = fe.res
    return {"srgr": srgr.reshape(lead), "recall": recall.reshape(lead), "hits": hits.reshape(lead + (J,)),
            "frames": np.asarray(fe.per_row, np.int64).reshape(lead)}


def l1div_of_tracks(x, frames=None) -> dict:
    """``x [..., T, D]`` with up to two leading axes (``[T, D]``, ``[U, T, D]``, ``[U, R, T, D]``; ``1 <= D <= MAX_COLS``), any column layout
    -- joints as ``J * 3`` columns (``joints.flatten(-2)``), a 126- or 282-column track, Euler channels -- -> ``{"l1div", "l1_sum"}`` each
    ``[...]`` float64, ``"mean" [..., D]`` float64 and ``"frames" [...]`` (host int64 numpy).  ``l1_sum`` is the summed absolute deviation of
    the row's valid frames from their mean frame and ``l1div = l1_sum / n``: the reference's ``L1div`` of one track.  ``x`` is not written.
    ``frames`` and the device rule as in ``srgr_of_joints``."""
    who = "l1div_of_tracks"
    shape = tuple(x.shape)
    if len(shape) < 2 or not 1 <= shape[-1] <= MAX_COLS or shape[-2] < 1:
        raise L.EgError(f"{who}: shape {shape}: need [..., T >= 1, D] with 1 <= D <= {MAX_COLS}")
    fe = RW.front(x, 2, frames, who, lambda v, fr, d_frames, R: launch_l1div(v, fr, d_frames, R), _l1_host, 1, "1", RW.host32)
    (mean, l1_sum, l1div), lead = fe.res, fe.lead
    return {"l1div": l1div.reshape(lead), "l1_sum": l1_sum.reshape(lead), "mean": mean.reshape(lead + (shape[-1],)),
            "frames": np.asarray(fe.per_row, np.int64).reshape(lead)}


class SemanticTargets:
    """The ``srgr=`` argument of ``harness.synthesize`` / ``synthesize_takes``: the target joints ``joints [U, T', J, 3]`` and the semantic
    weights ``semantic [U, T']`` (``None``: weights of 1) of U recordings at the output rate -- the joints made from the captured tracks with
    ``skeleton.joints_from_tracks`` / ``joints_from_rot6d`` and the arguments the call gives its own output stage -- and the ``threshold``.
    ``fit`` is the callers' check, by name, before anything runs."""

    def __init__(self, joints, semantic=None, threshold: float = 0.1):
        who = "SemanticTargets"
        shape = tuple(joints.shape)
        if len(shape) != 4 or shape[-1] != 3 or not 1 <= shape[-2] <= MAX_JOINTS or shape[1] < 1:
            raise L.EgError(f"{who}: joints shape {shape}: need [U, T', J, 3] with 1 <= J <= {MAX_JOINTS}")
        if semantic is not None and tuple(semantic.shape) != shape[:2]:
            raise L.EgError(f"{who}: semantic shape {tuple(semantic.shape)}: joints {shape} take {shape[:2]} (one weight per frame)")
        self.joints, self.semantic, self.threshold = joints, semantic, _finite(threshold, "threshold", who)

    def fit(self, who: str, U: Optional[int] = None, T: Optional[int] = None, J: Optional[int] = None) -> "SemanticTargets":
        """The targets against a call's recordings, output frames and joints (``None``: not known yet)."""
        u, t, j, _ = self.joints.shape
        for name, have, need in (("U", u, U), ("T'", t, T), ("J", j, J)):
            if need is not None and have != need:
                raise L.EgError(f"{who}: srgr=: the targets {tuple(self.joints.shape)} have {name}={have}, the call's joints have {name}={need}")
        return self

    def __repr__(self):
        return f"SemanticTargets({tuple(self.joints.shape)}, semantic={'None' if self.semantic is None else 'given'}, threshold={self.threshold:g})"


# ---- the reference's classes ---------------------------------------------------------------------------------------------------------------
class SRGR:
    """The reference's ``SRGR(threshold=0.1, joints=47)``: ``run(results, targets, semantic)`` scores one clip -- flat ``[N, J * 3]`` as
    upstream or ``[N, J, 3]``, numpy or tensors (CUDA tensors through the kernel), one weight per frame -- and returns its rate; ``avg()`` is
    ``sum rate * frames / sum frames`` over the clips so far, in host float64.  ``push(res)`` pools the rows of a ``srgr_of_joints`` dict the
    same way, each with its own valid frames."""

    def __init__(self, threshold: float = 0.1, joints: int = 47):
        self.threshold, self.pose_dimes = threshold, joints
        self.counter, self.sum = 0, 0.0

    def run(self, results, targets, semantic):
        J = self.pose_dimes
        res = srgr_of_joints(results.reshape(-1, J, 3), targets.reshape(-1, J, 3), semantic.reshape(-1), threshold=self.threshold)
        self.push(res)
        return float(res["srgr"])

    def push(self, res: dict) -> None:
        rate = np.asarray(res["srgr"].detach().cpu() if isinstance(res["srgr"], torch.Tensor) else res["srgr"], np.float64).reshape(-1)
        n = np.asarray(res["frames"], np.int64).reshape(-1)
        for r, k in zip(rate.tolist(), n.tolist()):
            self.counter += k
            self.sum += r * k

    def avg(self) -> float:
        return self.sum / self.counter


class L1div:
    """The reference's ``L1div()``: ``run(results)`` takes the frames of one clip ``[N, D]`` (numpy or tensors; CUDA tensors through the
    kernel) and leaves them as they are -- the reference overwrites its argument --; ``avg()`` is ``sum l1_sum / sum frames`` over the clips
    so far, in host float64.  ``push(res)`` pools the rows of an ``l1div_of_tracks`` dict the same way."""

    def __init__(self):
        self.counter, self.sum = 0, 0.0

    def run(self, results) -> None:
        self.push(l1div_of_tracks(results.reshape(results.shape[0], -1)))

    def push(self, res: dict) -> None:
        l1 = np.asarray(res["l1_sum"].detach().cpu() if isinstance(res["l1_sum"], torch.Tensor) else res["l1_sum"], np.float64).reshape(-1)
        n = np.asarray(res["frames"], np.int64).reshape(-1)
        for s, k in zip(l1.tolist(), n.tolist()):
            self.counter += k
            self.sum += s

    def avg(self) -> float:
        return self.sum / self.counter
