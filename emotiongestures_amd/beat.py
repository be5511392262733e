"""Beat-alignment score (model/Beat_score_v2.py:51-197, ``alignment(sigma=0.3, order=2)``), the seventh metric of the eval loop's summary
line (test_emotion_gesture_diversity_iterative.py:241-248,258-261).

Whole recordings: ``beat_alignment_tracks(audio, track, lengths, frames)`` scores roll-outs of any and unequal length, several draws per
recording, with the per-frame arrays in a workspace instead of one workgroup's LDS (csrc/beat_tracks.hip); where a recording fits the clip
call it returns the clip call's bits.

Batched GPU path (clips up to 32 s): ``beat_alignment(audio, pose)`` runs load_audio + load_pose + calculate_align for a whole batch in two HIP kernels
(csrc/mel.hip: beat_stft_kernel, beat_align_kernel) and returns the fp64 per-clip scores.  Drop-in path: ``alignment`` has the reference's
constructor and methods; ``load_audio`` runs the kernels' audio-only mode on one clip, ``load_pose`` / ``calculate_align`` are host numpy /
scipy following the reference line by line (they are also the in-package reference the GPU's fused stages are tested against).

The audio half restates librosa 0.10's documented onset_strength / onset_detect / onset_backtrack / feature.rms chain (include/emogest.h,
eg_beat_align); librosa is not installed here, so it is not pinned against librosa itself -- the same caveat as the mel front-end.
Two quirks of the reference are kept on purpose: audio beat times use librosa's default sr 22050 on 16 kHz audio, and only the
right-side pose curves are sliced to [t_start*fps : t_end*fps].  There is no CPU fallback for the audio half.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._host import BoundedCache, host_ptr, ptr as _ptr, sized, stream as _stream
from ._rows import count_list

__all__ = ["beat_alignment", "beat_alignment_tracks", "alignment", "L1div", "SRGR", "BeatScoreUnavailable", "MAX_FRAMES", "SAMPLE_RATE"]

SAMPLE_RATE = 16000
HOP = 512
LIBROSA_DEFAULT_SR = 22050          # onset_detect / frames_to_time / times_like are called without sr upstream
MAX_FRAMES = 1024                   # EG_BEAT_MAX_FRAMES
POSE_MIN_DIM = 174


class BeatScoreUnavailable(NotImplementedError):
    pass


def _refuse(what):
    raise BeatScoreUnavailable(f"model.Beat_score_v2.{what}: not part of the eval loop and not implemented here "
                               "(plotting, load_data, and the other metric classes of that file)")


class _Tables:
    """Device copies of eg_beat_tables (filterbank [1025,128] transposed, Hann [2048], twiddles [1024,2], bands [128,2]), per device."""

    def __init__(self, device: torch.device):
        lib = L.load()
        fb, win, tw = np.zeros(1025 * 128, np.float32), np.zeros(2048, np.float32), np.zeros(2048, np.float32)
        band = np.zeros(256, np.int32)
        L.check(lib.eg_beat_tables(host_ptr(fb), host_ptr(win), host_ptr(tw), host_ptr(band)), "eg_beat_tables")
        self.fb, self.win, self.tw, self.band = (torch.from_numpy(a).to(device) for a in (fb, win, tw, band))
        self.lib = lib


_TABLES = BoundedCache()


def _tables(device: torch.device) -> _Tables:
    return _TABLES.get(str(device), lambda: _Tables(device))


def _run(audio: torch.Tensor, pose: Optional[torch.Tensor], fps: int, t_start: int, t_end: int, sigma: float, order: int,
         want_beats: bool):
    if not (isinstance(audio, torch.Tensor) and audio.is_cuda):
        raise RuntimeError("beat_alignment: audio must be a CUDA tensor (there is no CPU fallback)")
    if audio.dim() != 2:
        raise ValueError(f"beat_alignment: audio must be [B, n_samples], got {tuple(audio.shape)}")
    dev = audio.device
    audio = audio.to(torch.float32).contiguous()
    B, n = audio.shape
    T = 1 + n // HOP
    if n < 2048 or T > MAX_FRAMES:
        raise ValueError(f"beat_alignment: n_samples={n} outside 2048..{MAX_FRAMES * HOP - 1}")
    F = 0
    if pose is not None:
        if not (isinstance(pose, torch.Tensor) and pose.device == dev):
            raise RuntimeError("beat_alignment: pose must be a CUDA tensor on the audio's device")
        if pose.dim() != 3 or pose.shape[0] != B:
            raise ValueError(f"beat_alignment: pose must be [B, F, D] with B={B}, got {tuple(pose.shape)}")
        if pose.shape[2] < POSE_MIN_DIM:
            raise ValueError(f"beat_alignment: pose_dim={pose.shape[2]}: the beat joints are columns 18:42 and 150:174 (needs >= {POSE_MIN_DIM})")
        pose = pose.to(torch.float32).contiguous()
        F = pose.shape[1]
        if F < 2 or F - 1 > MAX_FRAMES:
            raise ValueError(f"beat_alignment: {F} pose frames (2..{MAX_FRAMES + 1})")
        if not (0 <= t_start < t_end) or order < 1 or fps <= 0 or not sigma > 0:
            raise ValueError(f"beat_alignment: t_start={t_start} t_end={t_end} order={order} fps={fps} sigma={sigma}")
    tab = _tables(dev)
    lib = tab.lib
    nbytes = lib.eg_beat_workspace_bytes(B, n)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev) if pose is not None else None
    nab = torch.empty(B, dtype=torch.int32, device=dev)
    oenv = rms = am = pm = None
    if want_beats:
        oenv = torch.empty(B, T, dtype=torch.float32, device=dev)
        rms = torch.empty(B, T, dtype=torch.float32, device=dev)
        am = torch.empty(B, 3, T, dtype=torch.uint8, device=dev)
        if pose is not None:
            pm = torch.empty(B, 8, F - 1, dtype=torch.uint8, device=dev)
    L.check(lib.eg_beat_align(_ptr(audio), B, n, _ptr(pose), F, 0 if pose is None else pose.shape[2], int(fps), int(t_start), int(t_end),
                              float(sigma), int(order), _ptr(tab.fb), _ptr(tab.win), _ptr(tab.tw), _ptr(tab.band), _ptr(ws), nbytes,
                              _ptr(score), _ptr(nab), _ptr(oenv), _ptr(rms), _ptr(am), _ptr(pm), _stream(dev)), "eg_beat_align")
    return score, {"n_audio_beats": nab, "oenv": oenv, "rms": rms, "audio_beats": am, "pose_beats": pm}


def beat_alignment(audio: torch.Tensor, pose: torch.Tensor, fps: int = 15, t_start: int = 0, t_end: Optional[int] = None,
                   sigma: float = 0.3, order: int = 2, want_beats: bool = False):
    """Per-clip beat-alignment scores of a batch: ``alignment(sigma, order)``'s load_audio(audio[b], t_start) + load_pose(pose[b], t_start,
    t_end, fps) + calculate_align(..., fps) for every clip, on the GPU.

    audio [B, n] fp32 CUDA, 16 kHz (sliced here at t_start * 16000 as load_audio does); pose [B, F, D] fp32 CUDA with D >= 174;
    ``t_end`` defaults to int(F / fps) (the eval script's int(n_poses / fps)).  Returns fp64 scores [B] on the device; a clip without
    audio onsets scores NaN (upstream raises ZeroDivisionError there).  ``want_beats`` also returns a dict with ``n_audio_beats`` [B],
    ``oenv`` / ``rms`` [B, T], ``audio_beats`` [B, 3, T] uint8 (onset_raw 0/1, onset_bt / onset_bt_rms as multiplicities) and ``pose_beats``
    [B, 8, F-1] uint8 in load_pose's return order (right-side indices relative to the slice start)."""
    if t_end is None:
        t_end = int(pose.shape[1] / fps)
    if t_start:
        audio = audio[:, t_start * SAMPLE_RATE:]
    score, beats = _run(audio, pose, fps, t_start, t_end, sigma, order, want_beats)
    return (score, beats) if want_beats else score


# ---- whole recordings ---------------------------------------------------------------------------------------------------------------
class _TracksPlan:
    """Host vectors, the uploaded meta table and the workspace size of one (lengths, frames, t_end, fps, draws, Tmax, device)."""

    def __init__(self, lib, lengths, frames, t_end, fps, draws, Tmax, device):
        U = len(lengths)
        self.U = U
        self.lengths = np.ascontiguousarray(lengths, np.int32)
        self.frames = None if frames is None else np.ascontiguousarray(frames, np.int32)
        self.t_end = None if t_end is None else np.ascontiguousarray(t_end, np.int32)
        self.h_lengths, self.h_frames, self.h_t_end = host_ptr(self.lengths), host_ptr(self.frames), host_ptr(self.t_end)
        meta = np.zeros(max(int(lib.eg_beat_tracks_meta_ints(U)), 1), np.int32)
        L.check(lib.eg_beat_tracks_meta(self.h_lengths, self.h_frames, self.h_t_end, int(fps), U, host_ptr(meta)), "eg_beat_tracks_meta")
        self.T = 1 + self.lengths // HOP
        self.offsets = np.concatenate([[0], np.cumsum(self.T)[:-1]]).astype(np.int64)
        self.sum_T = int(self.T.sum())
        self.bytes = sized("eg_beat_tracks_workspace_bytes", self.h_lengths, self.h_frames, U, int(draws), int(Tmax))
        self.meta = torch.from_numpy(meta).to(device)


_PLANS = BoundedCache(16)


def _tracks_plan(lib, lengths, frames, t_end, fps, draws, Tmax, device) -> _TracksPlan:
    key = (tuple(lengths), None if frames is None else tuple(frames), None if t_end is None else tuple(t_end), int(fps), int(draws),
           int(Tmax), str(device))
    return _PLANS.get(key, lambda: _TracksPlan(lib, lengths, frames, t_end, fps, draws, Tmax, device))


def _run_tracks(audio: torch.Tensor, track: Optional[torch.Tensor], lengths, frames, fps, t_start, t_end, sigma, order, want_beats,
                workspace: Optional[torch.Tensor] = None, out: Optional[dict] = None):
    """One eg_beat_align_tracks call.  ``audio`` is already sliced at t_start; ``track [U, R, Tmax, D]`` or None (audio half only).
    ``workspace`` / ``out``: preallocated buffers of an earlier call with the same shapes (graph capture: no allocation inside).  The launch
    also reads the returned plan's ``meta`` table: whoever captures this call into a graph must keep that plan, the cache of 16 may drop it."""
    dev = audio.device
    U, stride = audio.shape
    R = Tmax = D = 0
    if track is not None:
        _, R, Tmax, D = track.shape
    tab = _tables(dev)
    lib = tab.lib
    plan = _tracks_plan(lib, lengths, frames if track is not None else None, t_end if track is not None else None, fps, max(R, 1), Tmax, dev)
    ws = workspace if workspace is not None else torch.empty(plan.bytes, dtype=torch.uint8, device=dev)
    if out is None:
        out = {"score": torch.empty(U, R, dtype=torch.float64, device=dev) if track is not None else None,
               "n_audio_beats": torch.empty(U, dtype=torch.int32, device=dev), "oenv": None, "rms": None, "audio_beats": None,
               "pose_beats": None}
        if want_beats:
            out["oenv"] = torch.empty(plan.sum_T, dtype=torch.float32, device=dev)
            out["rms"] = torch.empty(plan.sum_T, dtype=torch.float32, device=dev)
            out["audio_beats"] = torch.empty(3, plan.sum_T, dtype=torch.uint8, device=dev)
            if track is not None:
                out["pose_beats"] = torch.empty(U, R, 8, Tmax - 1, dtype=torch.uint8, device=dev)
    L.check(lib.eg_beat_align_tracks(_ptr(audio), U, stride, plan.h_lengths, _ptr(plan.meta), _ptr(track), max(R, 1), Tmax, D, plan.h_frames,
                                     int(fps), int(t_start), plan.h_t_end, float(sigma), int(order), _ptr(tab.fb), _ptr(tab.win), _ptr(tab.tw),
                                     _ptr(tab.band), _ptr(ws), ws.numel(), _ptr(out["score"]), _ptr(out["n_audio_beats"]), _ptr(out["oenv"]),
                                     _ptr(out["rms"]), _ptr(out["audio_beats"]), _ptr(out["pose_beats"]), _stream(dev)), "eg_beat_align_tracks")
    return out, plan, ws


def beat_alignment_tracks(audio: torch.Tensor, track: torch.Tensor, lengths=None, frames=None, fps: int = 15, t_start: int = 0, t_end=None,
                          sigma: float = 0.3, order: int = 2, want_beats: bool = False):
    """Beat-alignment scores of whole recordings: ``alignment(sigma, order)`` on ``(audio[u, :lengths[u]], track[u, r, :frames[u]])`` for
    every recording u and draw r, any length, one call (eg_beat_align_tracks).

    audio [U, stride] fp32 CUDA, 16 kHz, ``lengths[u]`` real samples in row u (default: the whole row; nothing past them is read);
    track [U, Tmax, D] or [U, R, Tmax, D] fp32 CUDA with D >= 174, ``frames[u]`` real poses (default Tmax).  ``t_start`` is common (audio sliced
    at t_start * 16000 as load_audio does), ``t_end``: None (int(frames[u] / fps) per recording), an int, or U ints.  The audio half of a
    recording runs once and serves its R draws.  Returns fp64 scores [U] or [U, R] on the device, NaN for a recording without onsets.

    ``want_beats`` also returns the dict of ``beat_alignment`` with the per-recording arrays zero-padded to the longest recording and the
    counts beside them: ``n_audio_beats`` [U], ``oenv`` / ``rms`` [U, max T], ``audio_beats`` [U, 3, max T] uint8, ``n_frames`` [U] (the
    onset frames T_u of each recording), ``pose_beats`` [U, (R,) 8, Tmax-1] uint8, ``pose_frames`` [U].  Where a recording fits
    ``beat_alignment`` every one of these equals, bit for bit, what ``beat_alignment`` returns for the trimmed rows."""
    if not (isinstance(audio, torch.Tensor) and audio.is_cuda):
        raise RuntimeError("beat_alignment_tracks: audio must be a CUDA tensor (there is no CPU fallback)")
    if not (isinstance(track, torch.Tensor) and track.device == audio.device):
        raise RuntimeError("beat_alignment_tracks: track must be a CUDA tensor on the audio's device")
    if audio.dim() != 2:
        raise ValueError(f"beat_alignment_tracks: audio must be [U, samples], got {tuple(audio.shape)}")
    U = audio.shape[0]
    if track.dim() not in (3, 4) or track.shape[0] != U:
        raise ValueError(f"beat_alignment_tracks: track must be [U, Tmax, D] or [U, R, Tmax, D] with U={U}, got {tuple(track.shape)}")
    has_draws = track.dim() == 4
    if track.shape[-1] < POSE_MIN_DIM:
        raise ValueError(f"beat_alignment_tracks: pose_dim={track.shape[-1]}: the beat joints are columns 18:42 and 150:174 "
                         f"(needs >= {POSE_MIN_DIM})")
    trk = track.to(torch.float32).contiguous()
    trk = trk if has_draws else trk[:, None]
    Tmax = trk.shape[2]
    lengths = [audio.shape[1]] * U if lengths is None else count_list(lengths, U, "beat_alignment_tracks", "lengths")
    frames = [Tmax] * U if frames is None else count_list(frames, U, "beat_alignment_tracks")
    if t_end is not None:
        t_end = [int(t_end)] * U if isinstance(t_end, (int, np.integer)) else count_list(t_end, U, "beat_alignment_tracks", "t_end")
    audio = audio.to(torch.float32)
    if t_start:
        audio = audio[:, int(t_start) * SAMPLE_RATE:]
        lengths = [n - int(t_start) * SAMPLE_RATE for n in lengths]
    audio = audio.contiguous()
    out, plan, _ws = _run_tracks(audio, trk, lengths, frames, fps, t_start, t_end, sigma, order, want_beats)
    score = out["score"] if has_draws else out["score"][:, 0]
    if not want_beats:
        return score
    maxT = int(plan.T.max())
    idx = torch.from_numpy((plan.offsets[:, None] + np.minimum(np.arange(maxT)[None, :], plan.T[:, None] - 1)).astype(np.int64)).to(audio.device)
    live = torch.from_numpy(np.arange(maxT)[None, :] < plan.T[:, None]).to(audio.device)
    pad = lambda packed: torch.where(live, packed[idx], torch.zeros((), dtype=packed.dtype, device=packed.device))
    am = torch.stack([pad(out["audio_beats"][a]) for a in range(3)], dim=1)
    pb = out["pose_beats"] if has_draws else out["pose_beats"][:, 0]
    beats = {"n_audio_beats": out["n_audio_beats"], "oenv": pad(out["oenv"]), "rms": pad(out["rms"]), "audio_beats": am, "pose_beats": pb,
             "n_frames": torch.from_numpy(plan.T.astype(np.int32)).to(audio.device),
             "pose_frames": torch.tensor(frames, dtype=torch.int32, device=audio.device)}
    return score, beats


# ---- drop-in for `from model.Beat_score_v2 import alignment` ----------------------------------------------------------------------
def _frames_to_time(frames) -> np.ndarray:
    """librosa.frames_to_time with its defaults (hop 512, sr 22050), as calculate_align calls it."""
    return (np.asanyarray(frames) * HOP).astype(int) / float(LIBROSA_DEFAULT_SR)


def _argrelextrema_less(data: np.ndarray, order: int):
    from scipy.signal import argrelextrema
    return argrelextrema(data, np.less, order=order)


class alignment(object):
    """model/Beat_score_v2.py:51-197.  load_audio runs on the GPU (audio-only mode of eg_beat_align); load_pose / GAHR / calculate_align
    are host numpy as upstream.  ``S`` stays None (only the plotting method reads it)."""

    def __init__(self, sigma, order):
        self.sigma = sigma
        self.order = order
        self.times = self.oenv = self.S = self.rms = None
        self.pose_data = []

    def load_audio(self, wave, t_start, without_file=False, sr_audio=16000, device=None):
        """:58-77.  Returns (onset_raw, onset_bt, onset_bt_rms) int arrays; sets oenv [T], times (times_like, sr 22050) and rms [1, T]."""
        if sr_audio != SAMPLE_RATE:
            raise ValueError(f"alignment.load_audio: the onset front-end is defined at {SAMPLE_RATE} Hz (got sr_audio={sr_audio})")
        if isinstance(wave, torch.Tensor):
            wave = wave.detach().cpu().numpy()
        short_y = np.ascontiguousarray(np.asarray(wave, dtype=np.float32).reshape(-1)[t_start * sr_audio:])
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        y = torch.from_numpy(short_y).to(dev)[None]
        _, beats = _run(y, None, 15, 0, 1, self.sigma, self.order, True)
        oenv, rms, am = (beats[k][0].cpu().numpy() for k in ("oenv", "rms", "audio_beats"))
        self.oenv = oenv
        self.times = _frames_to_time(np.arange(oenv.shape[-1]))
        self.rms = rms[None, :]
        frames = np.arange(oenv.shape[-1])
        onset_raw = np.flatnonzero(am[0]).astype(np.int64)
        onset_bt = np.repeat(frames, am[1].astype(np.int64))          # ascending, duplicates kept
        onset_bt_rms = np.repeat(frames, am[2].astype(np.int64))
        return onset_raw, onset_bt, onset_bt_rms

    def load_pose(self, pose, t_start, t_end, pose_fps, without_file=False):
        """:80-135: velocity L2 norms of 8 joint groups, beats = argrelextrema(np.less, order); returns 8 index tuples (right arm,
        shoulder, fore arm, wrist, left arm, shoulder, fore arm, wrist).  Only the right-side curves are sliced, as upstream."""
        if isinstance(pose, torch.Tensor):
            pose = pose.detach().cpu().numpy()
        pose = np.asarray(pose)
        if pose.ndim != 2 or pose.shape[1] < POSE_MIN_DIM:
            raise ValueError(f"alignment.load_pose: pose [F, D] needs D >= {POSE_MIN_DIM} (columns 18:42 and 150:174), got {pose.shape}")
        data_each_file = np.array([np.concatenate([row[18:42], row[150:174]], 0) for row in pose])
        vel = data_each_file[1:, :] - data_each_file[:-1, :]

        def norm(c0):
            return np.linalg.norm(np.array([vel[:, c0 + i] for i in range(6)]), axis=0)

        sl = slice(t_start * pose_fps, t_end * pose_fps)
        vel_right_shoulder, vel_right_arm, vel_right_fore_arm, vel_right_wrist = norm(0), norm(6), norm(12), norm(18)
        beat_right_arm = _argrelextrema_less(vel_right_arm[sl], self.order)
        beat_right_shoulder = _argrelextrema_less(vel_right_shoulder[sl], self.order)
        beat_right_fore_arm = _argrelextrema_less(vel_right_fore_arm[sl], self.order)
        beat_right_wrist = _argrelextrema_less(vel_right_wrist[sl], self.order)
        vel_left_shoulder, vel_left_arm, vel_left_fore_arm, vel_left_wrist = norm(24), norm(30), norm(36), norm(42)
        beat_left_arm = _argrelextrema_less(vel_left_arm, self.order)
        beat_left_shoulder = _argrelextrema_less(vel_left_shoulder, self.order)
        beat_left_fore_arm = _argrelextrema_less(vel_left_fore_arm, self.order)
        beat_left_wrist = _argrelextrema_less(vel_left_wrist, self.order)
        return (beat_right_arm, beat_right_shoulder, beat_right_fore_arm, beat_right_wrist, beat_left_arm, beat_left_shoulder,
                beat_left_fore_arm, beat_left_wrist)

    def load_data(self, *a, **k):
        """:137-140 cannot run upstream (it unpacks load_pose's 8 beat sets into 6 names); not called by the eval loop."""
        _refuse("alignment.load_data")

    def eval_random_pose(self, wave, pose, t_start, t_end, pose_fps, num_random=60):
        """:142-149"""
        onset_raw, onset_bt, onset_bt_rms = self.load_audio(wave, t_start, t_end)
        dur = t_end - t_start
        for i in range(num_random):
            beats = self.load_pose(pose, i, i + dur, pose_fps)
            dis_all_b2a = self.calculate_align(onset_raw, onset_bt, onset_bt_rms, *beats)
            print(f"{i}s: ", dis_all_b2a)

    def audio_beat_vis(self, *a, **k):
        _refuse("alignment.audio_beat_vis")

    @staticmethod
    def motion_frames2time(vel, offset, pose_fps):
        time_vel = vel[0] / pose_fps + offset
        return time_vel

    @staticmethod
    def GAHR(a, b, sigma):
        """:159-171 (an empty `b` raises ZeroDivisionError, an empty `a` contributes exp(-inf) = 0)."""
        dis_all_b2a = 0
        for b_each in b:
            l2_min = np.inf
            for a_each in a:
                l2_dis = abs(a_each - b_each)
                if l2_dis < l2_min:
                    l2_min = l2_dis
            dis_all_b2a += math.exp(-(l2_min ** 2) / (2 * sigma ** 2))
        dis_all_b2a /= len(b)
        return dis_all_b2a

    def calculate_align(self, onset_raw, onset_bt, onset_bt_rms, beat_right_arm, beat_right_shoulder, beat_right_fore_arm, beat_right_wrist,
                        beat_left_arm, beat_left_shoulder, beat_left_fore_arm, beat_left_wrist, pose_fps=15):
        """:173-197: sum of the 3 x 8 GAHR terms / 24, fp64."""
        avg_dis_all_b2a = 0
        for audio_beat in [onset_raw, onset_bt, onset_bt_rms]:
            for pose_beat in [beat_right_arm, beat_right_shoulder, beat_right_fore_arm, beat_right_wrist, beat_left_arm, beat_left_shoulder,
                              beat_left_fore_arm, beat_left_wrist]:
                audio_bt = _frames_to_time(audio_beat)
                pose_bt = self.motion_frames2time(pose_beat, 0, pose_fps)
                dis_all_b2a = self.GAHR(pose_bt, audio_bt, self.sigma)
                avg_dis_all_b2a += dis_all_b2a
        avg_dis_all_b2a /= 24
        return avg_dis_all_b2a


def _refuse_joint_score(what):
    raise BeatScoreUnavailable(f"model.Beat_score_v2.{what}: not part of the eval loop and not built in this module; the joint-space scores "
                               f"of whole tracks are emotiongestures_amd.jointscore.{what} (run / avg as upstream, CUDA tensors through the "
                               "kernel)")


class L1div(object):
    def __init__(self, *a, **k):
        _refuse_joint_score("L1div")


class SRGR(object):
    def __init__(self, *a, **k):
        _refuse_joint_score("SRGR")
