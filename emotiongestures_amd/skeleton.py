"""Skeleton output: gesture tracks in the model's coordinates <-> joint positions in metres (csrc/skeleton.hip).

Every synthesis call returns ``pose_dim = 3K`` numbers per frame: K bone direction vectors, usually with the data set's mean subtracted.
A renderer, an avatar or a metric in metres needs joints.  The reference bridges the gap on the host, one numpy loop over the bones per call
(utils/data_utils_expressive.py:153-201, ``convert_dir_vec_to_pose`` / ``convert_pose_seq_to_dir_vec``); here whole tracks stay on the device:

``Skeleton(parents, children, lengths)``     a table of K bones in topological order over J = K + 1 joints, joint 0 the root at the origin
``ted_expressive()``                          the 43-joint TED-Expressive upper body with fingers and face
``joints_from_tracks(track, skeleton, ...)``  ``[..., T, 3K]`` -> ``[..., T_out, J, 3]``: add the mean, optionally re-normalise the bones, walk the
                                              tree; with ``fps=(src, dst)`` also resample linearly to the renderer's frame rate
``dir_vec_from_joints(joints, skeleton)``     the inverse: joints -> unit bone vectors (minus the mean): the ``seed_pose`` a generator takes
``rotations_from_tracks(track, skeleton, rest, ...)``  ``[..., T, 3K]`` -> ``[..., T_out, K, 4]``: one local (or global) unit quaternion
                                              ``(w, x, y, z)`` per bone relative to the rest pose ``rest [K, 3]``: what a rigged avatar consumes

Definition (include/emogest.h).  For a source frame t: ``x_k = track[t, 3k:3k+3] + mean_k``; with ``unit``: ``x_k /= max(|x_k|, 1e-12)``;
``p[0] = 0`` and ``p[child_k] = p[parent_k] + length_k * x_k`` in table order.  With ``L / M = dst / src`` reduced, a row of n valid frames has
``n_out = ceil(n * L / M)`` output frames; frame k' is ``p(lo) + (p(lo + 1) - p(lo)) * f``, ``lo = min(floor(k' M / L), n - 2)``,
``f = (k' M - lo L) / L`` in exact integers: ``datapath.resample_pose_seq``'s linear interpolation with its extrapolation past the last frame
(n = 1: every frame is ``p(0)``).  At the native rate nothing is blended.  Output frames from ``n_out`` on are zeros; source frames from n on
are never used and may hold NaN.

Rotations (include/emogest.h: eg_skeleton_rotations).  ``rest`` rows are normalised in float64 and rounded to fp32.  ``pb(k)`` is the bone whose
child is ``parents[k]`` (-1 at the root); ``x^_k = x_k / max(|x_k|, 1e-12)``; in table order ``P_k = G_pb(k)`` (the identity at the root),
``v_k = conj(P_k) o x^_k``, ``L_k = arc(rest_k, v_k)``, ``G_k = P_k (x) L_k`` -- ``arc(a, b)`` the shortest arc ``(1 + c, a x b)`` normalised,
``c = a . b``, or for ``c < -1 + 1e-6`` the half turn about ``a x e_m`` (``e_m`` the first axis on which ``|a|`` is smallest).  On an interpolated
frame the vectors are blended (after the mean), then the chain runs on the blended frame.

CUDA tensors go through the kernels (fp32; there is no eager-PyTorch fallback for them).  numpy arrays and CPU tensors take the definition in
float64 numpy -- what the reference's functions compute -- so data preparation and the drop-ins of ``utils.data_utils_expressive`` run without
a GPU.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import BoundedCache, host_ptr, int_list, ptr as _ptr, stream as _stream

__all__ = ["Skeleton", "RestPose", "ted_expressive", "joints_from_tracks", "dir_vec_from_joints", "rotations_from_tracks", "out_frames",
           "rate_ratio", "TILE_FRAMES", "MAX_BONES", "MAX_FACTOR"]

TILE_FRAMES = L.EG_SKELETON_TILE_FRAMES      # output frames of one workgroup
MAX_BONES = L.EG_SKELETON_MAX_BONES
MAX_FACTOR = L.EG_SKELETON_MAX_FACTOR


class Skeleton:
    """K bones ``(parents[k], children[k], lengths[k])`` in topological order (eg_skeleton_check refuses anything else by name).  The device
    table is uploaded once per device."""

    def __init__(self, parents: Sequence[int], children: Sequence[int], lengths: Sequence[float]):
        if not (len(parents) == len(children) == len(lengths)):
            raise L.EgError(f"Skeleton: parents / children / lengths have {len(parents)} / {len(children)} / {len(lengths)} entries")
        self.parents = np.ascontiguousarray(parents, np.int32)
        self.children = np.ascontiguousarray(children, np.int32)
        self.lengths = np.ascontiguousarray(lengths, np.float64)          # as given: the float64 path's lengths
        self.lengths32 = self.lengths.astype(np.float32)                  # the device's
        self.K = int(len(self.parents))
        self.J = self.K + 1
        L.check(L.load().eg_skeleton_check(*self.host_ptrs(), self.K), "eg_skeleton_check")
        self._tables = BoundedCache()
        self._rests = BoundedCache(limit=16)

    def host_ptrs(self):
        return host_ptr(self.parents), host_ptr(self.children), host_ptr(self.lengths32)

    @property
    def pose_dim(self) -> int:
        return 3 * self.K

    @property
    def dir_vec_pairs(self) -> List[Tuple[int, int, float]]:
        """``(parent, child, length)`` per bone: what the reference's callers iterate over to draw bones."""
        return [(int(a), int(b), float(l)) for a, b, l in zip(self.parents, self.children, self.lengths)]

    @property
    def depth(self) -> np.ndarray:
        """Bones between the root and every joint, ``[J]``."""
        d = np.zeros(self.J, np.int64)
        for a, b in zip(self.parents, self.children):
            d[b] = d[a] + 1
        return d

    @property
    def bone_parents(self) -> np.ndarray:
        """``pb [K]``: the bone whose child is ``parents[k]``, -1 where that is the root.  ``pb[k] < k``."""
        owner = {int(b): k for k, b in enumerate(self.children)}
        return np.array([owner.get(int(a), -1) for a in self.parents], np.int64)

    def rest_pose(self, rest) -> "RestPose":
        """The checked, normalised rest pose ``rest [K, 3]`` with its level table; built once per distinct pose (the last 16 are kept)."""
        if isinstance(rest, RestPose):
            if rest.sk is not self and rest.sk != self:
                raise L.EgError(f"rest pose of {rest.sk!r} used with {self!r}")
            return rest
        if isinstance(rest, torch.Tensor):
            rest = rest.detach().cpu().numpy()
        raw = np.ascontiguousarray(rest, np.float64)
        if raw.shape != (self.K, 3):
            raise L.EgError(f"rest pose shape {raw.shape}: a skeleton of K={self.K} bones takes one direction per bone, [{self.K}, 3]")
        return self._rests.get(raw.tobytes(), lambda: RestPose(self, raw))

    def table(self, device) -> torch.Tensor:
        """int32 ``[3K]`` on ``device``: parents | children | lengths (fp32 bits)."""
        return self._tables.get(str(device), lambda: torch.from_numpy(
            np.concatenate([self.parents, self.children, self.lengths32.view(np.int32)])).to(device))

    def __eq__(self, other):
        return (isinstance(other, Skeleton) and np.array_equal(self.parents, other.parents) and np.array_equal(self.children, other.children)
                and np.array_equal(self.lengths, other.lengths))

    __hash__ = None

    def __repr__(self):
        return f"Skeleton(bones={self.K}, joints={self.J})"


class RestPose:
    """The bind pose of an avatar for one skeleton: ``raw [K, 3]`` float64 as given (eg_skeleton_rest_check refuses a non-finite or
    near-zero row by name), ``unit32 [K, 3]``: every row normalised in float64 and rounded to fp32 -- the unit vectors both the device and the
    float64 path use -- and ``words``, eg_skeleton_levels' table (levels by depth, bone parents, the same fp32 rows), uploaded once per device."""

    def __init__(self, sk: Skeleton, raw: np.ndarray):
        self.sk, self.raw = sk, raw
        L.check(L.load().eg_skeleton_rest_check(host_ptr(raw), sk.K), "eg_skeleton_rest_check")
        self.unit32 = (raw / np.sqrt(raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1] + raw[:, 2] * raw[:, 2])[:, None]).astype(np.float32)
        self.words = np.zeros(65 + 5 * sk.K, np.int32)
        L.check(L.load().eg_skeleton_levels(*sk.host_ptrs(), sk.K, host_ptr(raw), host_ptr(self.words)), "eg_skeleton_levels")
        self._tables = BoundedCache()

    def table(self, device) -> torch.Tensor:
        """int32 ``[65 + 5K]`` on ``device``."""
        return self._tables.get(str(device), lambda: torch.from_numpy(self.words).to(device))

    def __repr__(self):
        return f"RestPose(bones={self.sk.K}, levels={int(self.words[0])})"


def ted_expressive() -> Skeleton:
    """The TED-Expressive body: 43 joints, 42 bones, lengths in metres.  Joint 0 is the spine base, 1 the neck."""
    parents: List[int] = []
    children: List[int] = []
    lengths: List[float] = []

    def limb(start: int, joints: Sequence[int], lens: Sequence[float]) -> None:
        for j, l in zip(joints, lens):
            parents.append(start)
            children.append(j)
            lengths.append(l)
            start = j

    finger_lengths = {"index": (0.137, 0.044, 0.031), "middle": (0.144, 0.042, 0.033), "pinky": (0.127, 0.027, 0.026),
                      "ring": (0.134, 0.039, 0.033), "thumb": (0.068, 0.042, 0.036)}

    def hand(wrist: int, first: int) -> None:                 # five fingers of three joints, numbered consecutively from `first`
        for f, name in enumerate(("index", "middle", "pinky", "ring", "thumb")):
            limb(wrist, range(first + 3 * f, first + 3 * f + 3), finger_lengths[name])

    limb(0, [1], [0.26])                                      # spine -> neck
    limb(1, [2], [0.22])                                      # neck -> left shoulder
    limb(1, [3], [0.22])                                      # neck -> right shoulder
    limb(2, [4, 6], [0.36, 0.33])                             # left arm: elbow, wrist
    hand(6, 8)                                                # left hand: joints 8..22
    limb(3, [5, 7], [0.36, 0.33])                             # right arm: elbow, wrist
    hand(7, 23)                                               # right hand: joints 23..37
    limb(1, [38], [0.18])                                     # neck -> nose
    limb(38, [39], [0.14])                                    # nose -> right eye
    limb(38, [40], [0.14])                                    # nose -> left eye
    limb(39, [41], [0.15])                                    # right eye -> right ear
    limb(40, [42], [0.15])                                    # left eye -> left ear
    return Skeleton(parents, children, lengths)


# ---- rates and frame counts ------------------------------------------------------------------------------------------------------------
def rate_ratio(fps, who: str = "fps") -> Tuple[int, int]:
    """``fps=(src, dst)`` -> the reduced ``(L, M) = (dst, src) / gcd``; ``None``: ``(1, 1)``.  Refuses by name what the kernel does not take."""
    if fps is None:
        return 1, 1
    try:
        src, dst = fps
    except (TypeError, ValueError):
        raise L.EgError(f"{who}={fps!r}: need (source fps, output fps)")
    for v in (src, dst):
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise L.EgError(f"{who}={fps!r}: frame rates are positive integers")
    g = math.gcd(int(src), int(dst))
    Lf, M = int(dst) // g, int(src) // g
    if max(Lf, M) > MAX_FACTOR:
        raise L.EgError(f"{who}={fps!r} is the frame-rate ratio L={Lf} / M={M}: supported up to max(L, M) <= {MAX_FACTOR}")
    return Lf, M


def out_frames(n: int, fps=None) -> int:
    """``ceil(n * L / M)``: the output frames of n source frames."""
    Lf, M = rate_ratio(fps)
    return -(-int(n) * Lf // M)


def _frames_list(frames, U: int, T: int, who: str) -> Optional[List[int]]:
    if frames is None:
        return None
    fr = int_list([frames] if isinstance(frames, int) else frames)          # a bare int means one recording
    if len(fr) != U:
        raise L.EgError(f"{who}: frames has {len(fr)} entries for {U} recordings")
    if any(v < 0 or v > T for v in fr):
        raise L.EgError(f"{who}: frames {fr}: every value must be in [0, {T}]")
    return fr


def _frames_dev(fr: Optional[List[int]], device) -> Optional[torch.Tensor]:
    return None if fr is None else torch.tensor(fr, dtype=torch.int32, device=device)


def _lead(shape, n_tail: int, who: str):
    """Leading axes ``()``, ``(U,)`` or ``(U, R)`` -> (U, R)."""
    lead = tuple(shape[:-n_tail])
    if len(lead) > 2:
        raise L.EgError(f"{who}: shape {tuple(shape)}: at most two leading axes ([U, R, ...])")
    U = lead[0] if lead else 1
    R = lead[1] if len(lead) == 2 else 1
    return lead, int(U), int(R)


def _is_cuda(x) -> bool:
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host64(x, who: str) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, np.float64)


def _dev32(x: torch.Tensor) -> torch.Tensor:
    x = x.detach().to(torch.float32).contiguous()
    return x.clone() if x.data_ptr() % 16 else x                # a slice of a larger tensor may start anywhere


def _mean_dev(mean, K: int, device, who: str) -> Optional[torch.Tensor]:
    if mean is None:
        return None
    m = torch.as_tensor(mean).detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if m.numel() != 3 * K:
        raise L.EgError(f"{who}: mean has {m.numel()} values, the skeleton's tracks have {3 * K}")
    return m


def _mean_host(mean, K: int, who: str) -> Optional[np.ndarray]:
    if mean is None:
        return None
    m = _host64(mean, who).reshape(-1)
    if m.size != 3 * K:
        raise L.EgError(f"{who}: mean has {m.size} values, the skeleton's tracks have {3 * K}")
    return m


# ---- the float64 path: the definition ------------------------------------------------------------------------------------------------------
def _chain64(sk: Skeleton, x: np.ndarray) -> np.ndarray:
    """x [..., K, 3] -> p [..., J, 3]."""
    p = np.zeros(x.shape[:-2] + (sk.J, 3))
    for k in range(sk.K):
        p[..., sk.children[k], :] = p[..., sk.parents[k], :] + sk.lengths[k] * x[..., k, :]
    return p


def _joints64(v: np.ndarray, sk: Skeleton, frames: List[int], mean, unit: bool, Lf: int, M: int) -> np.ndarray:
    """v [B, T, 3K] float64, frames [B] -> [B, ceil(T L / M), J, 3]."""
    B, T, _D = v.shape
    out = np.zeros((B, -(-T * Lf // M), sk.J, 3))
    for b in range(B):
        n = frames[b]
        if n < 1:
            continue
        x = v[b, :n].reshape(n, sk.K, 3)
        if mean is not None:
            x = x + mean.reshape(sk.K, 3)
        if unit:
            x = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
        p = _chain64(sk, x)
        n_out = -(-n * Lf // M)
        if Lf == M:
            out[b, :n] = p
        elif n == 1:
            out[b, :n_out] = p[0]
        else:
            k = np.arange(n_out, dtype=np.int64)
            lo = np.minimum(k * M // Lf, n - 2)
            f = ((k * M - lo * Lf) / Lf)[:, None, None]
            out[b, :n_out] = p[lo] + (p[lo + 1] - p[lo]) * f
    return out


def _dir_vec64(p: np.ndarray, sk: Skeleton, frames: List[int], mean) -> np.ndarray:
    """p [B, T, J, 3] float64 -> [B, T, 3K]."""
    B, T = p.shape[:2]
    out = np.zeros((B, T, 3 * sk.K))
    for b in range(B):
        n = frames[b]
        if n < 1:
            continue
        d = p[b, :n][:, sk.children] - p[b, :n][:, sk.parents]
        d = d / np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12)
        d = d.reshape(n, 3 * sk.K)
        out[b, :n] = d if mean is None else d - mean
    return out


# quaternions (w, x, y, z) on the last axis, float64
def _qmul(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    pw, px, py, pz = np.moveaxis(p, -1, 0)
    qw, qx, qy, qz = np.moveaxis(q, -1, 0)
    return np.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)


def _qrot(q: np.ndarray, v: np.ndarray) -> np.ndarray:
    """q o v."""
    u, w = q[..., 1:], q[..., :1]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def _qconj(q: np.ndarray) -> np.ndarray:
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _arc64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a [3] unit, b [n, 3] unit or zero -> [n, 4]."""
    c = b[:, 0] * a[0] + b[:, 1] * a[1] + b[:, 2] * a[2]
    q = np.concatenate([(1.0 + c)[:, None], np.cross(a[None, :], b)], -1)
    q = q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-300)
    half = c < -1.0 + 1e-6
    if half.any():
        e = np.zeros(3)
        e[int(np.argmin(np.abs(a)))] = 1.0                      # argmin: the first axis on ties
        nrm = np.cross(a, e)
        q[half] = np.concatenate([[0.0], nrm / np.sqrt((nrm * nrm).sum())])
    return q


def _rotations64(v: np.ndarray, sk: Skeleton, rest: np.ndarray, frames: List[int], mean, glob: bool, Lf: int, M: int) -> np.ndarray:
    """v [B, T, 3K] float64, rest [K, 3] (unit), frames [B] -> [B, ceil(T L / M), K, 4]."""
    B, T, _D = v.shape
    out = np.zeros((B, -(-T * Lf // M), sk.K, 4))
    pb = sk.bone_parents
    for b in range(B):
        n = frames[b]
        if n < 1:
            continue
        x = v[b, :n].reshape(n, sk.K, 3)
        if mean is not None:
            x = x + mean.reshape(sk.K, 3)
        n_out = -(-n * Lf // M)
        if Lf == M:
            pass
        elif n == 1:
            x = np.repeat(x[:1], n_out, 0)
        else:                                                   # the vectors are blended, then the chain runs on the blended frame
            k = np.arange(n_out, dtype=np.int64)
            lo = np.minimum(k * M // Lf, n - 2)
            f = ((k * M - lo * Lf) / Lf)[:, None, None]
            x = (x[lo + 1] - x[lo]) * f + x[lo]
        x = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
        G = np.zeros((n_out, sk.K, 4))
        loc = np.zeros((n_out, sk.K, 4))
        for k in range(sk.K):
            if pb[k] < 0:
                loc[:, k] = G[:, k] = _arc64(rest[k], x[:, k])
            else:
                P = G[:, pb[k]]
                loc[:, k] = _arc64(rest[k], _qrot(_qconj(P), x[:, k]))
                G[:, k] = _qmul(P, loc[:, k])
        out[b, :n_out] = G if glob else loc
    return out


# ---- the device path ---------------------------------------------------------------------------------------------------------------------
def launch_joints(track: torch.Tensor, sk: Skeleton, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
                  mean: Optional[torch.Tensor] = None, unit: bool = False, ratio: Tuple[int, int] = (1, 1),
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_skeleton_joints on ``track [B, T, 3K]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``[B, T_out, J, 3]``: one launch on the current
    stream, nothing else -- static inputs and ``out`` make it capturable.  ``d_frames``: device int32 ``[B / draws]``, row b has
    ``d_frames[b // draws] * frame_unit`` valid frames."""
    B, T, D = track.shape
    if D != sk.pose_dim:
        raise L.EgError(f"skeleton of {sk.K} bones takes tracks of {sk.pose_dim} columns, got {D}")
    Lf, M = ratio
    t_out = -(-T * Lf // M)
    if out is None:
        out = torch.empty(B, t_out, sk.J, 3, dtype=torch.float32, device=track.device)
    L.check(L.load().eg_skeleton_joints(_ptr(track), B, T, *sk.host_ptrs(), sk.K, _ptr(sk.table(track.device)), _ptr(d_frames), int(draws),
                                        int(frame_unit), _ptr(mean), int(bool(unit)), Lf, M, _ptr(out), out.shape[1], _stream(track.device)),
            "eg_skeleton_joints")
    return out


def launch_dir_vec(joints: torch.Tensor, sk: Skeleton, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
                   mean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_skeleton_dir_vec on ``joints [B, T, J, 3]`` -> ``[B, T, 3K]``: one launch on the current stream."""
    B, T = joints.shape[:2]
    if out is None:
        out = torch.empty(B, T, sk.pose_dim, dtype=torch.float32, device=joints.device)
    L.check(L.load().eg_skeleton_dir_vec(_ptr(joints), B, T, *sk.host_ptrs(), sk.K, _ptr(sk.table(joints.device)), _ptr(d_frames), int(draws),
                                         int(frame_unit), _ptr(mean), _ptr(out), _stream(joints.device)), "eg_skeleton_dir_vec")
    return out


def _space(space, who: str) -> int:
    if space not in ("local", "global"):
        raise L.EgError(f"{who}: space={space!r}: 'local' (every bone relative to its parent) or 'global'")
    return L.EG_SKELETON_SPACE_GLOBAL if space == "global" else L.EG_SKELETON_SPACE_LOCAL


def launch_rotations(track: torch.Tensor, sk: Skeleton, rest: RestPose, d_frames: Optional[torch.Tensor] = None, draws: int = 1,
                     frame_unit: int = 1, mean: Optional[torch.Tensor] = None, space: str = "local", ratio: Tuple[int, int] = (1, 1),
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_skeleton_rotations on ``track [B, T, 3K]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``[B, T_out, K, 4]``: one launch on the current
    stream, nothing else (the level table is uploaded on first use per device: warm up before a capture).  ``rest``: ``sk.rest_pose(...)``;
    the other arguments as in ``launch_joints``."""
    B, T, D = track.shape
    if D != sk.pose_dim:
        raise L.EgError(f"skeleton of {sk.K} bones takes tracks of {sk.pose_dim} columns, got {D}")
    Lf, M = ratio
    t_out = -(-T * Lf // M)
    if out is None:
        out = torch.empty(B, t_out, sk.K, 4, dtype=torch.float32, device=track.device)
    L.check(L.load().eg_skeleton_rotations(_ptr(track), B, T, *sk.host_ptrs(), sk.K, host_ptr(rest.raw), _ptr(rest.table(track.device)),
                                           _ptr(d_frames), int(draws), int(frame_unit), _ptr(mean), _space(space, "launch_rotations"), Lf, M,
                                           _ptr(out), out.shape[1], _stream(track.device)), "eg_skeleton_rotations")
    return out


# ---- the public functions --------------------------------------------------------------------------------------------------------------------
def joints_from_tracks(track, skeleton: Skeleton, frames=None, mean=None, unit: bool = False, fps=None):
    """``track [..., T, 3K]`` with up to two leading axes (``[T, D]``, ``[U, T, D]``, ``[U, R, T, D]``) -> ``joints [..., T_out, J, 3]``,
    ``T_out = ceil(T * L / M)``.

    ``frames``: valid frames per recording (``[U]`` host ints; shared by the R draws of a recording; one value for ``[T, D]``): frames from
    ``frames[u]`` on are never used, the output is zeros from ``ceil(frames[u] * L / M)`` on.  ``mean [3K]``: added to every frame first (the
    data set's mean direction vectors).  ``unit``: every bone vector re-normalised to length 1 (``x / max(|x|, 1e-12)``).  ``fps=(src, dst)``:
    linear resampling to ``dst`` frames per second (``max(L, M) <= 64`` for the reduced ratio).

    A CUDA tensor: one kernel launch, fp32 CUDA result.  numpy or a CPU tensor: the definition in float64 (numpy in: numpy out; tensor in:
    float64 tensor out).  With ``frames`` or ``fps`` the result is ``(joints, joint_frames)``, ``joint_frames`` the valid output frames per
    recording (a list of U ints)."""
    who = "joints_from_tracks"
    if not isinstance(skeleton, Skeleton):
        raise L.EgError(f"{who}: skeleton must be a Skeleton, got {type(skeleton).__name__}")
    sk = skeleton
    shape = tuple(track.shape)
    if len(shape) < 2 or shape[-2] < 1:
        raise L.EgError(f"{who}: track shape {shape}: need [..., T >= 1, {sk.pose_dim}]")
    if shape[-1] != sk.pose_dim:
        raise L.EgError(f"{who}: track shape {shape}: a skeleton of K={sk.K} bones takes 3K={sk.pose_dim} columns per frame, not {shape[-1]}")
    lead, U, R = _lead(shape, 2, who)
    T = shape[-2]
    Lf, M = rate_ratio(fps, f"{who}: fps")
    fr = _frames_list(frames, U, T, who)
    t_out = -(-T * Lf // M)
    if _is_cuda(track):
        x = _dev32(track).reshape(U * R, T, sk.pose_dim)
        j = launch_joints(x, sk, _frames_dev(fr, x.device), R, 1, _mean_dev(mean, sk.K, x.device, who), unit, (Lf, M))
        joints = j.reshape(lead + (t_out, sk.J, 3))
    else:
        v = _host64(track, who).reshape(U * R, T, sk.pose_dim)
        per_row = [n for n in (fr if fr is not None else [T] * U) for _ in range(R)]
        j = _joints64(v, sk, per_row, _mean_host(mean, sk.K, who), bool(unit), Lf, M).reshape(lead + (t_out, sk.J, 3))
        joints = torch.from_numpy(j) if isinstance(track, torch.Tensor) else j
    if frames is None and fps is None:
        return joints
    return joints, [-(-n * Lf // M) for n in (fr if fr is not None else [T] * U)]


def dir_vec_from_joints(joints, skeleton: Skeleton, frames=None, mean=None):
    """``joints [..., T, J, 3]`` (up to two leading axes) -> ``dir_vec [..., T, 3K]``: ``d = p[child] - p[parent]``, ``d / max(|d|, 1e-12)`` (a
    zero-length bone gives the zero vector), minus ``mean [3K]`` when given -- the ``seed_pose`` / ``prior_seq`` a generator takes from
    motion-capture joints.  ``frames`` as in ``joints_from_tracks``: zeros from ``frames[u]`` on.  CUDA in: the kernel, fp32; numpy / CPU in:
    float64."""
    who = "dir_vec_from_joints"
    if not isinstance(skeleton, Skeleton):
        raise L.EgError(f"{who}: skeleton must be a Skeleton, got {type(skeleton).__name__}")
    sk = skeleton
    shape = tuple(joints.shape)
    if len(shape) < 3 or shape[-2:] != (sk.J, 3) or shape[-3] < 1:
        raise L.EgError(f"{who}: joints shape {shape}: need [..., T >= 1, {sk.J}, 3] for a skeleton of {sk.K} bones")
    lead, U, R = _lead(shape, 3, who)
    T = shape[-3]
    fr = _frames_list(frames, U, T, who)
    if _is_cuda(joints):
        p = _dev32(joints).reshape(U * R, T, sk.J, 3)
        return launch_dir_vec(p, sk, _frames_dev(fr, p.device), R, 1, _mean_dev(mean, sk.K, p.device, who)).reshape(lead + (T, sk.pose_dim))
    p = _host64(joints, who).reshape(U * R, T, sk.J, 3)
    per_row = [n for n in (fr if fr is not None else [T] * U) for _ in range(R)]
    d = _dir_vec64(p, sk, per_row, _mean_host(mean, sk.K, who)).reshape(lead + (T, sk.pose_dim))
    return torch.from_numpy(d) if isinstance(joints, torch.Tensor) else d


def rotations_from_tracks(track, skeleton: Skeleton, rest, frames=None, mean=None, fps=None, space: str = "local"):
    """``track [..., T, 3K]`` with up to two leading axes -> ``rotations [..., T_out, K, 4]``: per bone and output frame the unit quaternion
    ``(w, x, y, z)`` that turns the rest pose's bone into the track's -- ``space="local"``: relative to the parent bone (a pure swing, ``w >= 0``:
    what a glTF / VRM node, an engine rig or a BVH channel takes); ``"global"``: relative to the root, ``G_k o rest_k = x^_k``.

    ``rest [K, 3]``: the direction of every bone in the avatar's bind pose (any length; a row that is not finite or shorter than 1e-6 is
    refused by name), or ``skeleton.rest_pose(rest)``.  ``frames``, ``mean`` and ``fps`` as in ``joints_from_tracks``; on a resampled frame
    the bone vectors are blended and the rotations follow from the blended frame.  Forward kinematics with the offsets
    ``lengths[k] * rest_k`` and the local rotations gives ``joints_from_tracks(..., unit=True)``.

    A CUDA tensor: one kernel launch, fp32 CUDA result.  numpy or a CPU tensor: the definition in float64.  With ``frames`` or ``fps`` the
    result is ``(rotations, rotation_frames)`` under the rule of ``joints_from_tracks``."""
    who = "rotations_from_tracks"
    if not isinstance(skeleton, Skeleton):
        raise L.EgError(f"{who}: skeleton must be a Skeleton, got {type(skeleton).__name__}")
    sk = skeleton
    shape = tuple(track.shape)
    if len(shape) < 2 or shape[-2] < 1:
        raise L.EgError(f"{who}: track shape {shape}: need [..., T >= 1, {sk.pose_dim}]")
    if shape[-1] != sk.pose_dim:
        raise L.EgError(f"{who}: track shape {shape}: a skeleton of K={sk.K} bones takes 3K={sk.pose_dim} columns per frame, not {shape[-1]}")
    sp = _space(space, who)
    pose = sk.rest_pose(rest)
    lead, U, R = _lead(shape, 2, who)
    T = shape[-2]
    Lf, M = rate_ratio(fps, f"{who}: fps")
    fr = _frames_list(frames, U, T, who)
    t_out = -(-T * Lf // M)
    if _is_cuda(track):
        x = _dev32(track).reshape(U * R, T, sk.pose_dim)
        q = launch_rotations(x, sk, pose, _frames_dev(fr, x.device), R, 1, _mean_dev(mean, sk.K, x.device, who), space, (Lf, M))
        rot = q.reshape(lead + (t_out, sk.K, 4))
    else:
        v = _host64(track, who).reshape(U * R, T, sk.pose_dim)
        per_row = [n for n in (fr if fr is not None else [T] * U) for _ in range(R)]
        q = _rotations64(v, sk, pose.unit32.astype(np.float64), per_row, _mean_host(mean, sk.K, who), sp == L.EG_SKELETON_SPACE_GLOBAL, Lf, M)
        q = q.reshape(lead + (t_out, sk.K, 4))
        rot = torch.from_numpy(q) if isinstance(track, torch.Tensor) else q
    if frames is None and fps is None:
        return rot
    return rot, [-(-n * Lf // M) for n in (fr if fr is not None else [T] * U)]
