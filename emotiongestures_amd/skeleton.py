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
from types import SimpleNamespace
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


def level_words(K: int) -> int:
    """EG_SKELETON_LEVEL_WORDS(K): the level count | 64 level offsets | order [K] | bone parents [K] | rest [K, 3]."""
    return 1 + 64 + 5 * K


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
        self.words = np.zeros(level_words(sk.K), np.int32)
        L.check(L.load().eg_skeleton_levels(*sk.host_ptrs(), sk.K, host_ptr(raw), host_ptr(self.words)), "eg_skeleton_levels")
        self._tables = BoundedCache()

    def table(self, device) -> torch.Tensor:
        """int32 ``[level_words(K)]`` on ``device``."""
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


def _mean_checked(m, K: int, who: str):                        # m: the flat mean, a tensor or an array
    if len(m) != 3 * K:
        raise L.EgError(f"{who}: mean has {len(m)} values, the skeleton's tracks have {3 * K}")
    return m


def _mean_dev(mean, K: int, device, who: str) -> Optional[torch.Tensor]:
    return None if mean is None else _mean_checked(torch.as_tensor(mean).detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous(), K, who)


def _mean_host(mean, K: int, who: str) -> Optional[np.ndarray]:
    return None if mean is None else _mean_checked(_host64(mean, who).reshape(-1), K, who)


# ---- the float64 path: the definition ------------------------------------------------------------------------------------------------------
def _chain64(sk: Skeleton, x: np.ndarray) -> np.ndarray:
    """x [..., K, 3] -> p [..., J, 3]."""
    p = np.zeros(x.shape[:-2] + (sk.J, 3))
    for k in range(sk.K):
        p[..., sk.children[k], :] = p[..., sk.parents[k], :] + sk.lengths[k] * x[..., k, :]
    return p


def _resample64(y: np.ndarray, n_out: int, Lf: int, M: int) -> np.ndarray:
    """y [n, ., 3] at the source rate -> [n_out, ., 3]: frame k' blends the source frames lo and lo + 1 with the weight f (n = 1: frame 0)."""
    n = len(y)
    if Lf == M or n == 1:
        return y if Lf == M else np.repeat(y, n_out, 0)
    k = np.arange(n_out, dtype=np.int64)
    lo = np.minimum(k * M // Lf, n - 2)
    f = ((k * M - lo * Lf) / Lf)[:, None, None]
    return y[lo] + (y[lo + 1] - y[lo]) * f


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
        n_out = -(-n * Lf // M)
        out[b, :n_out] = _resample64(_chain64(sk, x), n_out, Lf, M)
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
        x = _resample64(x, n_out, Lf, M)                        # the vectors are blended, then the chain runs on the blended frame
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
def _forward_out(track: torch.Tensor, sk: Skeleton, ratio: Tuple[int, int], out: Optional[torch.Tensor], tail: Tuple[int, int]):
    """What launch_joints and launch_rotations do before the call: ``(B, T, L, M, out)``, ``out [B, T_out, *tail]`` made here unless given."""
    B, T, D = track.shape
    if D != sk.pose_dim:
        raise L.EgError(f"skeleton of {sk.K} bones takes tracks of {sk.pose_dim} columns, got {D}")
    Lf, M = ratio
    if out is None:
        out = torch.empty((B, -(-T * Lf // M)) + tail, dtype=torch.float32, device=track.device)
    return B, T, Lf, M, out


def launch_joints(track: torch.Tensor, sk: Skeleton, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
                  mean: Optional[torch.Tensor] = None, unit: bool = False, ratio: Tuple[int, int] = (1, 1),
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_skeleton_joints on ``track [B, T, 3K]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``[B, T_out, J, 3]``: one launch on the current
    stream, nothing else -- static inputs and ``out`` make it capturable.  ``d_frames``: device int32 ``[B / draws]``, row b has
    ``d_frames[b // draws] * frame_unit`` valid frames."""
    B, T, Lf, M, out = _forward_out(track, sk, ratio, out, (sk.J, 3))
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
    B, T, Lf, M, out = _forward_out(track, sk, ratio, out, (sk.K, 4))
    L.check(L.load().eg_skeleton_rotations(_ptr(track), B, T, *sk.host_ptrs(), sk.K, host_ptr(rest.raw), _ptr(rest.table(track.device)),
                                           _ptr(d_frames), int(draws), int(frame_unit), _ptr(mean), _space(space, "launch_rotations"), Lf, M,
                                           _ptr(out), out.shape[1], _stream(track.device)), "eg_skeleton_rotations")
    return out


# ---- the public functions --------------------------------------------------------------------------------------------------------------------
def _per_row(fr: Optional[List[int]], U: int, R: int, T: int) -> List[int]:
    return [n for n in (fr if fr is not None else [T] * U) for _ in range(R)]


def _shape_checked(track, sk, who: str) -> Skeleton:
    """The first half of the front end of both forward functions: the skeleton's type and the track's shape; returns the skeleton."""
    if not isinstance(sk, Skeleton):
        raise L.EgError(f"{who}: skeleton must be a Skeleton, got {type(sk).__name__}")
    shape = tuple(track.shape)
    if len(shape) < 2 or shape[-2] < 1:
        raise L.EgError(f"{who}: track shape {shape}: need [..., T >= 1, {sk.pose_dim}]")
    if shape[-1] != sk.pose_dim:
        raise L.EgError(f"{who}: track shape {shape}: a skeleton of K={sk.K} bones takes 3K={sk.pose_dim} columns per frame, not {shape[-1]}")
    return sk


def _front(track, sk: Skeleton, frames, fps, who: str) -> SimpleNamespace:
    """The second half, behind a caller's own checks: the leading axes ``lead`` of the track (``()``, ``(U,)`` or ``(U, R)``), ``U``, ``R``,
    ``T``, the reduced ``ratio = (L, M)``, ``fr`` (``frames`` as a checked list, or None), ``t_out``, the valid source frames
    ``per_row [U * R]`` and the valid output frames ``n_out [U]``."""
    lead, U, R = _lead(track.shape, 2, who)
    T = track.shape[-2]
    Lf, M = rate_ratio(fps, f"{who}: fps")
    fr = _frames_list(frames, U, T, who)
    return SimpleNamespace(lead=lead, U=U, R=R, T=T, ratio=(Lf, M), fr=fr, t_out=-(-T * Lf // M), per_row=_per_row(fr, U, R, T),
                           n_out=[-(-n * Lf // M) for n in (fr if fr is not None else [T] * U)])


def _finish(res, track, fe, tail: Tuple[int, int], frames, fps):
    """``res [U * R, T_out, *tail]`` under the leading axes of ``track``; tensor in: tensor out; with ``frames`` or ``fps``: ``(res, n_out)``."""
    res = res.reshape(fe.lead + (fe.t_out,) + tail)
    if isinstance(track, torch.Tensor) and not isinstance(res, torch.Tensor):
        res = torch.from_numpy(res)
    return res if frames is None and fps is None else (res, fe.n_out)


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
    sk = _shape_checked(track, skeleton, who)
    fe = _front(track, sk, frames, fps, who)
    if _is_cuda(track):
        x = _dev32(track).reshape(fe.U * fe.R, fe.T, sk.pose_dim)
        j = launch_joints(x, sk, _frames_dev(fe.fr, x.device), fe.R, 1, _mean_dev(mean, sk.K, x.device, who), unit, fe.ratio)
    else:
        v = _host64(track, who).reshape(fe.U * fe.R, fe.T, sk.pose_dim)
        j = _joints64(v, sk, fe.per_row, _mean_host(mean, sk.K, who), bool(unit), *fe.ratio)
    return _finish(j, track, fe, (sk.J, 3), frames, fps)


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
    d = _dir_vec64(p, sk, _per_row(fr, U, R, T), _mean_host(mean, sk.K, who)).reshape(lead + (T, sk.pose_dim))
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
    sk = _shape_checked(track, skeleton, who)
    sp, pose = _space(space, who), sk.rest_pose(rest)
    fe = _front(track, sk, frames, fps, who)
    if _is_cuda(track):
        x = _dev32(track).reshape(fe.U * fe.R, fe.T, sk.pose_dim)
        q = launch_rotations(x, sk, pose, _frames_dev(fe.fr, x.device), fe.R, 1, _mean_dev(mean, sk.K, x.device, who), space, fe.ratio)
    else:
        v = _host64(track, who).reshape(fe.U * fe.R, fe.T, sk.pose_dim)
        q = _rotations64(v, sk, pose.unit32.astype(np.float64), fe.per_row, _mean_host(mean, sk.K, who), sp == L.EG_SKELETON_SPACE_GLOBAL, *fe.ratio)
    return _finish(q, track, fe, (sk.K, 4), frames, fps)


def _output_args_early(who: str, joints, joints_fps, rotations, fps_allowed: bool = True) -> None:
    """The part of ``output_args`` that needs no model: what a caller refuses before it looks at anything else."""
    if not fps_allowed and joints_fps is not None:
        raise L.EgError(f"{who}: joints_fps= is not supported (a frame-rate change needs the frame after the last one emitted, which a "
                        "stream does not have yet); resample the joints of the finished track with skeleton.joints_from_tracks(..., fps=)")
    if rotations is not None and joints is None:
        raise L.EgError(f"{who}: rotations= without joints=skeleton (the rest pose belongs to a skeleton's bones)")


def output_args(who: str, pose_dim: int, joints, joints_mean, joints_unit, joints_fps, rotations, rotations_space, fps_allowed: bool = True,
                hint: str = "") -> Optional[RestPose]:
    """The skeleton-output arguments of a caller (``synthesize``, ``GestureStream``: ``who``, the prefix of every message), checked before
    anything runs; returns the rest pose of ``rotations=`` on ``joints``' skeleton, or None.  ``pose_dim``: the model's; ``fps_allowed``: the
    caller can change the frame rate; ``hint`` ends the message about a skeleton that does not fit ``pose_dim``."""
    _output_args_early(who, joints, joints_fps, rotations, fps_allowed)
    if rotations is None and rotations_space != "local":
        raise L.EgError(f"{who}: rotations_space without rotations=rest")
    if joints is None:
        if joints_mean is not None or joints_unit or joints_fps is not None:
            raise L.EgError(f"{who}: joints_mean / joints_unit{' / joints_fps' if fps_allowed else ''} without joints=skeleton")
        return None
    if not isinstance(joints, Skeleton):
        raise L.EgError(f"{who}: joints= takes a skeleton.Skeleton, got {type(joints).__name__}")
    if joints.pose_dim != pose_dim:
        raise L.EgError(f"{who}: joints=: the skeleton has K={joints.K} bones, 3K={joints.pose_dim} != pose_dim={pose_dim}{hint}")
    rate_ratio(joints_fps, f"{who}: joints_fps")                                   # refuses an unsupported ratio
    if rotations is None:
        return None
    _space(rotations_space, f"{who}: rotations_space")                             # and a bad space or rest pose
    return joints.rest_pose(rotations)
