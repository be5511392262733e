"""Take diversity of whole tracks: FGD features and pairwise distances of the R takes ``synthesize(..., draws=R)`` returns per recording.

The eval loop's FGD and ``Div_score`` (model/FHD_score.py:159-217,247-311; ``harness.evaluate``) are defined on fixed-length clips and run in
float64 numpy on the host.  This module is their whole-track counterpart, on the device (csrc/takes.hip), for tracks of any and unequal
length whose tail is padding:

``track_features(fgd, track, frames)``   the FGD encoder (model/FGD.py:26-82, per frame) on the VALID rows only, in packed order
``take_distance(feat, frames, draws)``   fp64 distance of every pair of takes of one recording, and their mean: the take diversity
``take_diversity(fgd, track, frames)``   the two in one call

Packed order (include/emogest.h): recording-major, then draw, then frame; with ``off[u]`` the exclusive prefix sum of ``frames``, row
``R*off[u] + r*frames[u] + t`` holds pose ``(u, r, t)``; ``N = R * sum(frames)`` rows.

``distance[u, r, r'] = sqrt(scale_u * sum_{t < frames[u]} sum_k (feat[u,r,t,k] - feat[u,r',t,k])**2)`` in fp64, each fp32 feature widened
before the subtraction.  ``span=None``: ``scale_u = 1``, exactly the pair distance inside ``harness.calculate_diversity`` on activations of
``frames[u]`` rows.  ``span=S``: ``scale_u = S / frames[u]`` -- the same quantity at the scale of an S-frame clip (the mean squared distance
per frame times S), so takes of a 30 s and of a 60 s recording, and the clip metric at ``frames == S``, read in one unit.
``diversity[u]`` is the mean of ``distance[u]`` over the ``R (R - 1) / 2`` pairs.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._host import BoundedCache, host_ptr, ptr as _ptr, sized, stream as _stream
from ._rows import count_list

__all__ = ["track_features", "take_distance", "take_diversity", "pack_rows", "workspace_bytes", "FEATURE_DIM", "MAX_DRAWS"]

FEATURE_DIM = 512
MAX_DRAWS = L.EG_TAKE_MAX_DRAWS


class _TakesPlan:
    """Host frames vector, the uploaded ``frames | off`` table and (for draws >= 2) the workspace size of one (frames, draws, device)."""

    def __init__(self, lib, frames, draws, device):
        U = len(frames)
        self.U = U
        self.frames = np.ascontiguousarray(frames, np.int32)
        self.h_frames = host_ptr(self.frames)
        meta = np.zeros(max(int(lib.eg_take_meta_ints(U)), 1), np.int32)
        L.check(lib.eg_take_meta(self.h_frames, U, host_ptr(meta)), "eg_take_meta")
        self.off = meta[U:2 * U].copy()
        self.sum_frames = int(self.frames.astype(np.int64).sum())
        self.bytes = 0
        if draws >= 2:
            self.bytes = sized("eg_take_distance_workspace_bytes", self.h_frames, U, int(draws))
        self.meta = torch.from_numpy(meta).to(device)

    @classmethod
    def get(cls, lib, frames, draws, device) -> "_TakesPlan":
        return _PLANS.get((tuple(frames), int(draws), str(device)), lambda: cls(lib, frames, draws, device))


_PLANS = BoundedCache(16)


def _track4(track, who):
    if not (isinstance(track, torch.Tensor) and track.is_cuda):
        raise RuntimeError(f"{who}: track must be a CUDA tensor (there is no CPU fallback)")
    if track.dim() not in (3, 4):
        raise ValueError(f"{who}: track must be [U, Tmax, D] or [U, R, Tmax, D], got {tuple(track.shape)}")
    trk = track.detach().to(torch.float32).contiguous()
    return trk if trk.dim() == 4 else trk[:, None]


def pack_rows(track: torch.Tensor, frames=None):
    """The valid rows of ``track [U, (R,) Tmax, D]`` in packed order with the row length padded to ``4 * ceil(D / 4)`` by zero columns
    (eg_track_rows_pack, one launch).  Rows at or beyond ``frames[u]`` are never read.  -> (rows [N, Dpad], frames, off)."""
    trk = _track4(track, "pack_rows")
    U, R, Tmax, D = trk.shape
    frames = [Tmax] * U if frames is None else count_list(frames, U, "pack_rows")
    lib = L.load()
    plan = _TakesPlan.get(lib, frames, R, trk.device)
    rows = torch.empty(R * plan.sum_frames, (D + 3) // 4 * 4, dtype=torch.float32, device=trk.device)
    L.check(lib.eg_track_rows_pack(_ptr(trk), U, R, Tmax, D, plan.h_frames, _ptr(plan.meta), _ptr(rows),
                                   _stream(trk.device)), "eg_track_rows_pack")
    return rows, frames, plan.off.tolist()


def track_features(fgd, track: torch.Tensor, frames=None):
    """FGD features of whole tracks: ``fgd``'s encoder (``Encoder[0]``, ``[2]``, ``[4]``, no ReLU, as ``MLP_Reconstruct.forward`` runs them) on
    the valid rows of ``track [U, Tmax, D]`` or ``[U, R, Tmax, D]`` (fp32, CUDA), ``frames[u]`` real poses per recording (default Tmax; rows
    beyond them are never read and may hold anything).  The rows are packed by one kernel, zero pad columns included, and go through
    ``ops.linear`` with ``fgd``'s own packed weights and ``fgd.precision``: bit for bit ``fgd(rows)[1]`` on the same packed rows.

    Returns ``(feat [N, 512], frames, off)`` in packed order.  ``feat`` can go straight into ``harness.FrechetAccumulator.push``: pushing the
    features of generated tracks into one accumulator and those of the target tracks into another gives the FGD of whole tracks against
    whole tracks (``harness.calculate_frechet_distance(*acc_pred.stats(), *acc_target.stats())``) over valid frames only."""
    from .modules import _eval_only
    _eval_only(fgd)
    x, frames, off = pack_rows(track, frames)
    D = fgd.Encoder[0].weight.shape[1]
    pad = x.shape[1] - D
    if pad < 0 or pad > 3:
        raise ValueError(f"track_features: track has {track.shape[-1]} pose columns, the FGD encoder takes {D}")
    cache = fgd._cache
    for i, lin in enumerate((fgd.Encoder[0], fgd.Encoder[2], fgd.Encoder[4])):
        pk = pad if i == 0 else 0
        packed = cache.get(lin, x.device, pad_k=pk)
        x = ops.linear(x, cache.padded_weight(lin) if pk else lin.weight, lin.bias, precision=fgd.precision, packed=packed)
    return x, frames, off


def take_distance(feat: torch.Tensor, frames, draws: int, span: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
                  out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """Pairwise distances of the ``draws`` takes of every recording from packed features ``feat [N, K]`` (fp32, CUDA; K = 512 for the FGD
    encoder), ``N = draws * sum(frames)`` (eg_take_distance: two launches, fp64, fixed summation orders, no atomics).

    Returns ``{"distance": [U, R, R] fp64, "diversity": [U] fp64}`` on the device: ``distance`` symmetric with an exactly zero diagonal,
    ``diversity[u]`` its mean over the pairs r < r'.  ``span``: see the module docstring (None: the raw pair distance).
    ``workspace`` (uint8, at least the plan's size) / ``out`` (the dict of an earlier call with the same shapes): preallocated buffers, so that
    the call allocates nothing (graph capture).  The launches also read the plan's uploaded ``frames | off`` table, which the returned dict does
    not carry: whoever captures this call into a graph must keep ``_TakesPlan.get(lib, frames, draws, device)``, the cache of 16 may drop it."""
    R = int(draws)
    if R < 2:
        raise L.EgError(f"take_distance: draws={R}: a distance between takes needs draws >= 2")
    if R > MAX_DRAWS:
        raise L.EgError(f"take_distance: draws={R} (2..{MAX_DRAWS})")
    if not (isinstance(feat, torch.Tensor) and feat.is_cuda):
        raise RuntimeError("take_distance: feat must be a CUDA tensor (there is no CPU fallback)")
    if feat.dim() != 2:
        raise ValueError(f"take_distance: feat must be packed [N, K], got {tuple(feat.shape)}")
    frames = count_list(frames, len(frames), "take_distance")
    U = len(frames)
    N, K = feat.shape
    if N != R * sum(frames):
        raise ValueError(f"take_distance: feat has {N} rows, draws * sum(frames) = {R} * {sum(frames)}")
    if span is not None and int(span) < 1:
        raise ValueError(f"take_distance: span={span} (None or >= 1)")
    feat = feat.detach().to(torch.float32).contiguous()
    dev = feat.device
    lib = L.load()
    plan = _TakesPlan.get(lib, frames, R, dev)
    ws = workspace if workspace is not None else torch.empty(plan.bytes, dtype=torch.uint8, device=dev)
    if out is None:
        out = {"distance": torch.empty(U, R, R, dtype=torch.float64, device=dev), "diversity": torch.empty(U, dtype=torch.float64, device=dev)}
    L.check(lib.eg_take_distance(_ptr(feat), U, R, K, plan.h_frames, _ptr(plan.meta), 0 if span is None else int(span), _ptr(ws), ws.numel(),
                                 _ptr(out["distance"]), _ptr(out["diversity"]), _stream(dev)), "eg_take_distance")
    return out


def workspace_bytes(frames, draws: int) -> int:
    """Bytes of ``take_distance``'s workspace for (frames, draws) (eg_take_distance_workspace_bytes; host only)."""
    fr = np.ascontiguousarray(frames, np.int32)
    return sized("eg_take_distance_workspace_bytes", host_ptr(fr), len(fr), int(draws))


def take_diversity(fgd, track: torch.Tensor, frames=None, span: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
                   out: Optional[dict] = None, stride: Optional[int] = None, tail: bool = True) -> Dict[str, torch.Tensor]:
    """``take_distance(track_features(fgd, track, frames), frames, R, span)`` for ``track [U, R, Tmax, D]``: how far apart the R takes of
    every recording are in FGD feature space.  -> ``{"distance": [U, R, R], "diversity": [U]}`` fp64 on the device.

    With a ``model.motion_ae.MotionAE`` as the net (the TED feature space) the features are
    ``motionfeat.window_features(net, track, frames, stride, tail)``, one row of ``latent_dim`` floats per 34-frame window, and the distance
    runs over recording u's windows: ``frames = plan.counts``, ``K = latent_dim`` (a multiple of 4; anything else is refused by name) and
    ``span`` counts windows -- ``span=1`` is the RMS per-window feature distance, comparable across recording lengths.  ``stride`` and
    ``tail`` belong to this form alone."""
    if not isinstance(track, torch.Tensor) or track.dim() != 4 or track.shape[1] < 2:
        raise L.EgError(f"take_diversity: track must be [U, R, Tmax, D] with R >= 2 takes per recording, got "
                        f"{tuple(track.shape) if isinstance(track, torch.Tensor) else type(track).__name__}")
    from .model.motion_ae import MotionAE
    if isinstance(fgd, MotionAE):
        from . import motionfeat as MF
        latent = MF._encoder(fgd, "take_diversity")[2]
        if latent < 4 or latent % 4:
            raise L.EgError(f"take_diversity: the MotionAE's latent_dim={latent}: take_distance reads features in 16-byte groups "
                            "(a multiple of 4, >= 4)")
        feat, plan = MF.window_features(fgd, track, frames, stride, tail)
        return take_distance(feat, plan.counts.tolist(), track.shape[1], span=span, workspace=workspace, out=out)
    if stride is not None or not tail:
        raise L.EgError("take_diversity: stride= and tail= are the window arguments of a MotionAE; the FGD encoder is per frame")
    feat, frames, _off = track_features(fgd, track, frames)
    return take_distance(feat, frames, track.shape[1], span=span, workspace=workspace, out=out)
