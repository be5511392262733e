"""Motion-clip features of whole tracks: ``MotionAE``'s encoder (model/motion_ae.py, the feature net behind the TED-style Frechet gesture
distance and diversity, model/embedding_space_evaluator.py) on every 34-frame window of tracks of any and unequal length with R takes each.

``window_rows(ae, track, frames=None, stride=None, tail=True, clips=None)``            the convolutional tower, one launch -> ``(rows [n, 384], plan)``
``window_features(ae, track, frames=None, stride=None, tail=True, chunk_clips=4096)``  the encoder -> ``(feat [N, latent_dim], plan)``
``clip_index(plan, draws)``                                                            host only: ``(u, r, start)`` of every clip, in clip order

Windows and clip order are those of ``emotion.window_plan(frames, 34, stride, tail)`` (include/emogest.h): windows at ``0, S, 2S, ...`` while
they fit (``S`` defaults to 34), with ``tail=True`` one more at ``frames[u] - 34`` when that is on no stride; recording-major, then take, then
window; ``N = R * plan.total``.  Poses at or beyond ``frames[u]`` are never read and may hold NaN; a recording shorter than 34 poses is
refused by name.

The tower is eg_motion_window_rows (csrc/motionfeat.hip): the windows are gathered straight from the ragged track, the four convolutions
(BatchNorm folded in, the tensors ``motion_ae._conv_pack`` caches) run in one launch with the activations in LDS, and the two stride-1
layers run once per pose of a run of windows instead of once per window.  Every sum is added in ``ops.conv1d``'s order, so
``window_rows`` equals ``PoseEncoderConv.net`` layer by layer on host-cut windows bit for bit, and ``window_features`` equals
``ae.encoder(windows)`` run in the same ranges.  ``feat`` goes straight into ``harness.FrechetAccumulator(dim=latent_dim).push`` -- the FGD
of whole TED tracks against whole TED tracks -- and into ``takes.take_distance(feat, plan.counts, R)``.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import int_list, ptr as _ptr, stream as _stream

__all__ = ["window_rows", "window_features", "out_net", "clip_index", "run_windows", "WINDOW", "ROW_FLOATS", "RUN_FRAMES", "MAX_POSE_DIM"]

WINDOW = L.EG_MOTION_WINDOW                     # 34: PoseEncoderConv's out_net is sized for it
ROW_FLOATS = L.EG_MOTION_ROW_FLOATS             # 32 channels * 12 positions: out_net's input
RUN_FRAMES = L.EG_MOTION_RUN_FRAMES             # the most poses one workgroup stages
MAX_POSE_DIM = L.EG_MOTION_MAX_POSE_DIM


def run_windows(stride: int) -> int:
    """Strided windows of one take that one workgroup owns at this stride (eg_motion_run_windows; host only)."""
    n = int(L.load().eg_motion_run_windows(int(stride)))
    if n < 1:
        raise L.EgError(f"run_windows: stride={stride} (need >= 1)")
    return n


def clip_index(plan, draws: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Recording, take and first pose of every clip of a window plan with ``draws`` takes, int64 ``[N]`` each, in clip order."""
    R = int(draws)
    u = np.concatenate([np.full(R * int(plan.counts[i]), i, np.int64) for i in range(plan.U)])
    r = np.concatenate([np.repeat(np.arange(R, dtype=np.int64), int(plan.counts[i])) for i in range(plan.U)])
    s = np.concatenate([np.tile(plan.starts(i).astype(np.int64), R) for i in range(plan.U)])
    return u, r, s


def _encoder(ae, who):
    """PoseEncoderConv of a MotionAE (or the encoder itself); anything else is refused by name.  -> (encoder, pose_dim, latent_dim)"""
    enc = getattr(ae, "encoder", ae)
    try:
        net, out = enc.net, enc.out_net
        D, latent = int(net[0][0].weight.shape[1]), int(out[6].weight.shape[0])
        ok = tuple(net[3].weight.shape) == (32, 64, 3) and int(out[0].weight.shape[1]) == ROW_FLOATS
    except (AttributeError, IndexError, TypeError):
        ok = False
    if not ok:
        raise L.EgError(f"{who}: the feature net must be a model.motion_ae.MotionAE (or its PoseEncoderConv), got {type(ae).__name__}")
    return enc, D, latent


def _front(ae, track, frames, stride, tail, who):
    """The host checks of both calls, in this order before anything touches the device: -> (encoder, latent_dim, plan)."""
    from . import emotion as EM
    enc, D, latent = _encoder(ae, who)
    if enc.training or getattr(ae, "training", False):
        raise L.EgError(f"{who}: the feature net is not in eval mode (call .eval()): its BatchNorm is folded into the weights")
    if not isinstance(track, torch.Tensor) or track.dim() not in (3, 4):
        raise ValueError(f"{who}: track must be [U, Tmax, D] or [U, R, Tmax, D], got "
                         f"{tuple(track.shape) if isinstance(track, torch.Tensor) else type(track).__name__}")
    if int(track.shape[-1]) != D:
        raise L.EgError(f"{who}: track has {int(track.shape[-1])} pose columns, the feature net takes pose_dim={D}")
    if D > MAX_POSE_DIM:
        raise L.EgError(f"{who}: pose_dim={D} (1..{MAX_POSE_DIM})")
    U, Tmax = int(track.shape[0]), int(track.shape[-2])
    if track.dim() == 4 and not 1 <= int(track.shape[1]) <= L.EG_TAKE_MAX_DRAWS:
        raise L.EgError(f"{who}: draws={int(track.shape[1])} (1..{L.EG_TAKE_MAX_DRAWS})")
    if stride is not None and int(stride) < 1:
        raise L.EgError(f"{who}: stride={stride} (None or >= 1)")
    frames = [Tmax] * U if frames is None else int_list(frames)
    if len(frames) != U:
        raise ValueError(f"{who}: frames has {len(frames)} entries for {U} recordings")
    for u, f in enumerate(frames):
        if f < WINDOW:
            raise L.EgError(f"{who}: frames[{u}]={f} < window={WINDOW} (the encoder takes whole windows: no padding, no resampling)")
        if f > Tmax:
            raise L.EgError(f"{who}: frames[{u}]={f} > Tmax={Tmax}")
    return enc, latent, EM.window_plan(frames, WINDOW, stride, tail)


def _cuda4(track, who):
    """track -> [U, R, Tmax, D] fp32, contiguous, on its GPU."""
    if not track.is_cuda:
        raise RuntimeError(f"{who}: track must be a CUDA tensor (there is no CPU fallback)")
    trk = track.detach().to(torch.float32).contiguous()
    return trk if trk.dim() == 4 else trk[:, None]


def _tower_weights(enc, device):
    from .model.motion_ae import _conv_pack
    packs = [_conv_pack(blk[0], device, blk[1]) for blk in (enc.net[0], enc.net[1], enc.net[2])] + [_conv_pack(enc.net[3], device)]
    return [t for wb in packs for t in wb]                                    # w1, b1, ..., w4, b4


def _launch(enc, trk, plan, c0, c1, out):
    U, R, Tmax, D = trk.shape
    dev = trk.device
    L.check(L.load().eg_motion_window_rows(_ptr(trk), U, R, Tmax, D, WINDOW, plan.stride, int(plan.tail), plan.h_frames, _ptr(plan.table(dev)),
                                           *[_ptr(t) for t in _tower_weights(enc, dev)], int(c0), int(c1), _ptr(out), _stream(dev)),
            "eg_motion_window_rows")
    return out


def window_rows(ae, track: torch.Tensor, frames=None, stride: Optional[int] = None, tail: bool = True, clips=None,
                out: Optional[torch.Tensor] = None):
    """The convolutional tower of ``ae`` (an eval-mode ``MotionAE``) on the windows ``clips = (c0, c1)`` (default: all) of ``track
    [U, Tmax, D]`` or ``[U, R, Tmax, D]`` (fp32, CUDA) -> ``(rows [c1 - c0, 384] fp32, plan)``: row ``c - c0`` is ``net(window c).flatten()``,
    channel-major, what ``out_net`` consumes.  One launch; ``out`` (fp32 ``[c1 - c0, 384]``, contiguous) makes the call allocation-free for
    graph capture after one eager call (whoever captures keeps ``plan``, whose uploaded table the launch reads).  A row does not depend on
    the range it was computed in."""
    who = "window_rows"
    enc, _latent, plan = _front(ae, track, frames, stride, tail, who)
    N = (int(track.shape[1]) if track.dim() == 4 else 1) * plan.total
    c0, c1 = (0, N) if clips is None else (int(clips[0]), int(clips[1]))
    if not 0 <= c0 < c1 <= N:
        raise L.EgError(f"{who}: clips [{c0}, {c1}) (need 0 <= c0 < c1 <= N={N})")
    trk = _cuda4(track, who)
    if out is None:
        out = torch.empty(c1 - c0, ROW_FLOATS, dtype=torch.float32, device=trk.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (c1 - c0, ROW_FLOATS)):
        raise L.EgError(f"{who}: out= must be a contiguous fp32 CUDA tensor [{c1 - c0}, {ROW_FLOATS}]")
    with torch.no_grad():
        return _launch(enc, trk, plan, c0, c1, out), plan


def out_net(ae, rows: torch.Tensor) -> torch.Tensor:
    """``PoseEncoderConv.out_net`` on tower rows ``[n, 384]`` as ``PoseEncoderConv.forward`` runs it: three products with the BatchNorms
    folded in, on the packs cached on the layers."""
    from .model.motion_ae import _dense
    enc = _encoder(ae, "out_net")[0]
    o = enc.out_net
    with torch.no_grad():
        return _dense(_dense(_dense(rows, o[0], o[1]), o[3], o[4]), o[6])


def window_features(ae, track: torch.Tensor, frames=None, stride: Optional[int] = None, tail: bool = True, chunk_clips: int = 4096):
    """``ae.encoder`` on every 34-frame window of ``track [U, Tmax, D]`` or ``[U, R, Tmax, D]`` (fp32, CUDA), ``frames[u]`` valid poses per
    recording (default Tmax) -> ``(feat [N, latent_dim] fp32 in clip order, plan)``.  For every range of at most ``chunk_clips`` clips: one
    launch of the tower, then ``out_net`` into the range's rows of ``feat`` -- the range bounds the workspace (1.5 KB of rows per clip).
    Bit for bit ``ae.encoder(windows)`` on host-cut windows of the same range (the products choose their tiles by row count, so ``feat`` may
    differ in rounding between values of ``chunk_clips``; the rows do not)."""
    who = "window_features"
    if int(chunk_clips) < 1:
        raise L.EgError(f"{who}: chunk_clips={chunk_clips} (need >= 1)")
    enc, latent, plan = _front(ae, track, frames, stride, tail, who)
    trk = _cuda4(track, who)
    N, step = trk.shape[1] * plan.total, int(chunk_clips)
    feat = torch.empty(N, latent, dtype=torch.float32, device=trk.device)
    rows = torch.empty(min(step, N), ROW_FLOATS, dtype=torch.float32, device=trk.device)
    with torch.no_grad():
        for c0 in range(0, N, step):
            c1 = min(N, c0 + step)
            feat[c0:c1].copy_(out_net(enc, _launch(enc, trk, plan, c0, c1, rows[:c1 - c0])))
    return feat, plan
