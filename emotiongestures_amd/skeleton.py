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

Articulated bodies (include/emogest.h: eg_articulate_forward / eg_articulate_rot6d).  The BEAT generators' tracks hold one 6-D rotation per
joint, ``pose_dim = 6J``; their body is ``JointTree(parents, offsets, basis="rows", names=None)``: ``1 <= J <= 64`` joints in topological order
(``parents[0] == -1``, ``0 <= parents[j] < j``), ``offsets [J, 3]`` in metres the joint's position in its parent's frame at the bind pose
(finite; zero allowed); ``basis`` states how the data set wrote the six numbers and belongs to the tree.
``JointTree.from_bvh(text, joints=None, unit=0.01)`` reads the ``HIERARCHY`` block of a BVH file.  For a source frame
``d_j = track[t, 6j:6j+6] (+ mean_j)``, ``a1 = d_j[0:3]``, ``a2 = d_j[3:6]``; ``b1 = a1 / max(|a1|, 1e-12)``, ``u2 = a2 - (b1 . a2) b1``,
``b2 = u2 / max(|u2|, 1e-12)``, ``b3 = b1 x b2``; ``R_j`` has the rows ``b1, b2, b3`` (``basis="rows"``: pytorch3d's ``rotation_6d_to_matrix``)
or has them as columns (``"columns"``: Zhou et al. 2019).  A degenerate group (zero, or ``a1`` parallel to ``a2``) gives a finite matrix that is
not a rotation; every output stays finite.  Chain, in table order: ``G_0 = R_0``, ``p_0 = offsets[0]``, ``G_j = G_parent R_j``,
``p_j = p_parent + G_parent offsets[j]``.  ``joints_from_rot6d`` returns ``p [..., T_out, J, 3]``; ``rotations_from_rot6d`` the unit quaternion
``(w, x, y, z)`` of ``R_j`` (``space="local"``) or ``G_j`` (``"global"``) ``[..., T_out, J, 4]``: from the matrix by the branch of the largest
of (trace, m00, m11, m22), normalised, ``w >= 0``.  ``fps=(src, dst)``: the same ``L / M``, ``lo`` and ``f`` as above; the 6-D vectors of the
source frames ``lo`` and ``lo + 1`` are blended, after the mean, and the whole chain runs on the blended frame, so the joints and rotations of
one call describe the same pose (n = 1: every frame is frame 0).  Source frames from ``frames[u]`` on are never read; output frames from
``n_out`` on are zeros.  ``rot6d_from_rotations(quat [..., T, J, 4], tree)`` is the inverse: the quaternion normalised
(``/ max(|q|, 1e-12)``), the first two rows (or columns) of its matrix as ``a1 | a2``, minus the mean; zeros from ``frames[u]`` on: the
``seed_pose`` a BEAT generator takes from motion capture.

Euler channels (include/emogest.h: eg_articulate_euler / eg_articulate_rot6d_euler / eg_angle_unwrap).  ``euler_from_rot6d(track, tree, order)``
gives the same ``R_j`` as the angles of a BVH file's rotation channels, ``[..., T_out, J, 3]``; ``rot6d_from_euler`` is the inverse and
``unwrap_angles`` the Euler filter (whole turns only); their docstrings hold the definitions.  ``emotiongestures_amd.bvh`` reads and writes
the files.

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
from ._host import BoundedCache, host_ptr, ptr as _ptr, stream as _stream
from ._rows import dev32, frames_dev, frames_list, front, host64, is_cuda, lead_axes, per_row

__all__ = ["Skeleton", "RestPose", "ted_expressive", "joints_from_tracks", "dir_vec_from_joints", "rotations_from_tracks", "out_frames",
           "rate_ratio", "TILE_FRAMES", "MAX_BONES", "MAX_FACTOR", "JointTree", "joints_from_rot6d", "rotations_from_rot6d",
           "rot6d_from_rotations", "ARTICULATE_TILE_FRAMES", "MAX_JOINTS", "euler_from_rot6d", "rot6d_from_euler", "unwrap_angles", "launch_euler",
           "launch_rot6d_euler", "launch_unwrap", "unwrap_workspace", "order_codes", "order_axes", "euler_args", "TrackOutputs", "ORDERS", "UNWRAP_TILE_FRAMES"]

TILE_FRAMES = L.EG_SKELETON_TILE_FRAMES      # output frames of one workgroup
MAX_BONES = L.EG_SKELETON_MAX_BONES
MAX_FACTOR = L.EG_SKELETON_MAX_FACTOR


def level_words(K: int) -> int:
    """EG_SKELETON_LEVEL_WORDS(K): the level count | 64 level offsets | order [K] | bone parents [K] | rest [K, 3]."""
    return 1 + 64 + 5 * K


class Skeleton:
    """K bones ``(parents[k], children[k], lengths[k])`` in topological order (eg_skeleton_check refuses anything else by name).  The device
    table is uploaded once per device."""
    noun, sym, parts, factor = "skeleton", "K", "bones", 3        # how the checks speak of this body: pose_dim = factor * count

    def __init__(self, parents: Sequence[int], children: Sequence[int], lengths: Sequence[float]):
        if not (len(parents) == len(children) == len(lengths)):
            raise L.EgError(f"Skeleton: parents / children / lengths have {len(parents)} / {len(children)} / {len(lengths)} entries")
        self.parents = np.ascontiguousarray(parents, np.int32)
        self.children = np.ascontiguousarray(children, np.int32)
        self.lengths = np.ascontiguousarray(lengths, np.float64)          # as given: the float64 path's lengths
        self.lengths32 = self.lengths.astype(np.float32)                  # the device's
        self.K = self.count = int(len(self.parents))
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


def _mean_checked(m, D: int, who: str):                        # m: the flat mean, a tensor or an array; D: the body's pose_dim
    if len(m) != D:
        raise L.EgError(f"{who}: mean has {len(m)} values, the skeleton's tracks have {D}")
    return m


def _mean_dev(mean, D: int, device, who: str) -> Optional[torch.Tensor]:
    return None if mean is None else _mean_checked(torch.as_tensor(mean).detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous(), D, who)


def _mean_host(mean, D: int, who: str) -> Optional[np.ndarray]:
    return None if mean is None else _mean_checked(host64(mean, who).reshape(-1), D, who)


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


def _valid_rows64(v: np.ndarray, frames: List[int], tail: Tuple[int, ...], fn, Lf: int = 1, M: int = 1) -> np.ndarray:
    """The valid rows of every recording, zeros elsewhere: ``out [B, ceil(T L / M), *tail]`` with ``out[b, :n_out] = fn(v[b, :n], n, n_out)`` for
    the ``n = frames[b] >= 1`` valid source frames of row b of ``v [B, T, ...]`` and their ``n_out = ceil(n L / M)`` output frames."""
    out = np.zeros((len(v), -(-v.shape[1] * Lf // M)) + tail)
    for b, n in enumerate(frames):
        if n >= 1:
            n_out = -(-n * Lf // M)
            out[b, :n_out] = fn(v[b, :n], n, n_out)
    return out


def _joints64(v: np.ndarray, sk: Skeleton, frames: List[int], mean, unit: bool, Lf: int, M: int) -> np.ndarray:
    """v [B, T, 3K] float64, frames [B] -> [B, ceil(T L / M), J, 3]."""
    def row(x, n, n_out):
        x = x.reshape(n, sk.K, 3)
        if mean is not None:
            x = x + mean.reshape(sk.K, 3)
        if unit:
            x = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
        return _resample64(_chain64(sk, x), n_out, Lf, M)
    return _valid_rows64(v, frames, (sk.J, 3), row, Lf, M)


def _dir_vec64(p: np.ndarray, sk: Skeleton, frames: List[int], mean) -> np.ndarray:
    """p [B, T, J, 3] float64 -> [B, T, 3K]."""
    def row(pn, n, _n_out):
        d = pn[:, sk.children] - pn[:, sk.parents]
        d = d / np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12)
        d = d.reshape(n, 3 * sk.K)
        return d if mean is None else d - mean
    return _valid_rows64(p, frames, (3 * sk.K,), row)


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
    pb = sk.bone_parents

    def row(x, n, n_out):
        x = x.reshape(n, sk.K, 3)
        if mean is not None:
            x = x + mean.reshape(sk.K, 3)
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
        return G if glob else loc
    return _valid_rows64(v, frames, (sk.K, 4), row, Lf, M)


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
def _body_checked(body, kind, who: str):
    if not isinstance(body, kind):
        raise L.EgError(f"{who}: {kind.noun} must be a {kind.__name__}, got {type(body).__name__}")
    return body


def _track_checked(track, body, kind, who: str):
    """The first half of the front end of every forward function: the body's type (``kind``: Skeleton or JointTree) and the track's shape, in
    the body's own words; returns the body."""
    b = _body_checked(body, kind, who)
    shape = tuple(track.shape)
    if len(shape) < 2 or shape[-2] < 1:
        raise L.EgError(f"{who}: track shape {shape}: need [..., T >= 1, {b.pose_dim}]")
    if shape[-1] != b.pose_dim:
        raise L.EgError(f"{who}: track shape {shape}: a {b.noun} of {b.sym}={b.count} {b.parts} takes {b.factor}{b.sym}={b.pose_dim} columns "
                        f"per frame, not {shape[-1]}")
    return b


def _front(track, sk: Skeleton, frames, fps, who: str) -> SimpleNamespace:
    """The second half, behind a caller's own checks: the leading axes ``lead`` of the track (``()``, ``(U,)`` or ``(U, R)``), ``U``, ``R``,
    ``T``, the reduced ``ratio = (L, M)``, ``fr`` (``frames`` as a checked list, or None), ``t_out``, the valid source frames
    ``per_row [U * R]`` and the valid output frames ``n_out [U]``."""
    lead, U, R = lead_axes(track.shape, 2, who)
    T = track.shape[-2]
    Lf, M = rate_ratio(fps, f"{who}: fps")
    fr = frames_list(frames, U, T, who)
    return SimpleNamespace(lead=lead, U=U, R=R, T=T, ratio=(Lf, M), fr=fr, t_out=-(-T * Lf // M), per_row=per_row(fr, U, R, T),
                           n_out=[-(-n * Lf // M) for n in (fr if fr is not None else [T] * U)])


def _finish(res, track, fe, tail: Tuple[int, int], frames, fps):
    """``res [U * R, T_out, *tail]`` under the leading axes of ``track``; tensor in: tensor out; with ``frames`` or ``fps``: ``(res, n_out)``."""
    res = res.reshape(fe.lead + (fe.t_out,) + tail)
    if isinstance(track, torch.Tensor) and not isinstance(res, torch.Tensor):
        res = torch.from_numpy(res)
    return res if frames is None and fps is None else (res, fe.n_out)


def _forward(track, body, frames, mean, fps, who: str, tail: Tuple[int, int], on_device, on_host):
    """Behind the checks of a forward function: ``_front``, then ``on_device(x [U * R, T, D] fp32, fe, d_frames, d_mean)`` for a CUDA tensor
    or ``on_host(v [U * R, T, D] float64, fe, mean64)`` for anything else, then ``_finish``."""
    fe = _front(track, body, frames, fps, who)
    D = body.pose_dim
    if is_cuda(track):
        x = dev32(track).reshape(fe.U * fe.R, fe.T, D)
        res = on_device(x, fe, frames_dev(fe.fr, x.device), _mean_dev(mean, D, x.device, who))
    else:
        res = on_host(host64(track, who).reshape(fe.U * fe.R, fe.T, D), fe, _mean_host(mean, D, who))
    return _finish(res, track, fe, tail, frames, fps)


def _inverse(x, body, kind, name: str, width: int, who: str):
    """The check of an inverse function: the body's type and the shape of ``x [..., T, J, width]``; returns the body."""
    b = _body_checked(body, kind, who)
    shape = tuple(x.shape)
    if len(shape) < 3 or shape[-2:] != (b.J, width) or shape[-3] < 1:
        raise L.EgError(f"{who}: {name} shape {shape}: need [..., T >= 1, {b.J}, {width}] for a {b.noun} of {b.count} {b.parts}")
    return b


def _per_frame(x, n_tail: int, frames, who: str, tail: Tuple[int, ...], on_device, on_host):
    """The front end and the finish of the inverse and in-place functions, whose output has the input's frames: ``x [..., T, *]`` with
    ``n_tail`` axes from T on and up to two leading ones -> ``[..., T, *tail]`` from ``on_device(x [U * R, T, *] fp32, d_frames, R)`` for a
    CUDA tensor or ``on_host(x [U * R, T, *] float64, per_row)`` for anything else (tensor in: tensor out)."""
    fe = front(x, n_tail, frames, who, lambda xd, _fr, d_frames, R: on_device(xd, d_frames, R), on_host)
    return fe.res.reshape(fe.lead + (fe.T,) + tail)


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
    sk = _track_checked(track, skeleton, Skeleton, who)
    return _forward(track, sk, frames, mean, fps, who, (sk.J, 3),
                    lambda x, fe, d_frames, d_mean: launch_joints(x, sk, d_frames, fe.R, 1, d_mean, unit, fe.ratio),
                    lambda v, fe, mean64: _joints64(v, sk, fe.per_row, mean64, bool(unit), *fe.ratio))


def dir_vec_from_joints(joints, skeleton: Skeleton, frames=None, mean=None):
    """``joints [..., T, J, 3]`` (up to two leading axes) -> ``dir_vec [..., T, 3K]``: ``d = p[child] - p[parent]``, ``d / max(|d|, 1e-12)`` (a
    zero-length bone gives the zero vector), minus ``mean [3K]`` when given -- the ``seed_pose`` / ``prior_seq`` a generator takes from
    motion-capture joints.  ``frames`` as in ``joints_from_tracks``: zeros from ``frames[u]`` on.  CUDA in: the kernel, fp32; numpy / CPU in:
    float64."""
    who = "dir_vec_from_joints"
    sk = _inverse(joints, skeleton, Skeleton, "joints", 3, who)
    return _per_frame(joints, 3, frames, who, (sk.pose_dim,),
                      lambda p, d_frames, R: launch_dir_vec(p, sk, d_frames, R, 1, _mean_dev(mean, sk.pose_dim, p.device, who)),
                      lambda p, per_row: _dir_vec64(p, sk, per_row, _mean_host(mean, sk.pose_dim, who)))


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
    sk = _track_checked(track, skeleton, Skeleton, who)
    sp, pose = _space(space, who), sk.rest_pose(rest)
    return _forward(track, sk, frames, mean, fps, who, (sk.K, 4),
                    lambda x, fe, d_frames, d_mean: launch_rotations(x, sk, pose, d_frames, fe.R, 1, d_mean, space, fe.ratio),
                    lambda v, fe, mean64: _rotations64(v, sk, pose.unit32.astype(np.float64), fe.per_row, mean64,
                                                       sp == L.EG_SKELETON_SPACE_GLOBAL, *fe.ratio))


# ---- articulated bodies: 6-D joint rotations (the BEAT generators) -----------------------------------------------------------------------------
ARTICULATE_TILE_FRAMES = L.EG_ARTICULATE_TILE_FRAMES
MAX_JOINTS = L.EG_ARTICULATE_MAX_JOINTS
_BASES = {"rows": L.EG_ARTICULATE_BASIS_ROWS, "columns": L.EG_ARTICULATE_BASIS_COLUMNS}


def articulate_level_words(J: int) -> int:
    """EG_ARTICULATE_LEVEL_WORDS(J): the level count | 65 level offsets | order [J] | parents [J] | offsets [J, 3]."""
    return 1 + 65 + 5 * J


class JointTree:
    """A body for tracks of 6-D joint rotations: J joints in topological order (``parents[0] == -1``, ``0 <= parents[j] < j``),
    ``offsets [J, 3]`` in metres -- the joint's position in its parent's frame at the bind pose -- and ``basis``: how the data set wrote the six
    numbers of a joint, ``"rows"`` (the first two rows of the matrix: pytorch3d's ``rotation_6d_to_matrix``) or ``"columns"`` (Zhou et al.
    2019).  ``pose_dim = 6J``.  eg_articulate_check refuses a bad table by name.  The level table (the joints by depth, the parents and the
    fp32 offsets: what the kernel reads) is built once and uploaded once per device."""
    noun, sym, parts, factor = "tree", "J", "joints", 6

    def __init__(self, parents: Sequence[int], offsets, basis: str = "rows", names: Optional[Sequence[str]] = None):
        if basis not in _BASES:
            raise L.EgError(f"JointTree: basis={basis!r}: 'rows' (pytorch3d's rotation_6d_to_matrix) or 'columns' (Zhou et al. 2019)")
        self.parents = np.ascontiguousarray(parents, np.int32).reshape(-1)
        if isinstance(offsets, torch.Tensor):
            offsets = offsets.detach().cpu().numpy()
        self.offsets = np.ascontiguousarray(offsets, np.float64)          # as given: the float64 path's offsets
        self.J = self.count = int(len(self.parents))
        if self.offsets.shape != (self.J, 3):
            raise L.EgError(f"JointTree: offsets shape {self.offsets.shape}: {self.J} parents take one offset per joint, [{self.J}, 3]")
        self.offsets32 = self.offsets.astype(np.float32)                  # the device's
        self.basis = basis
        self.names = None if names is None else [str(n) for n in names]
        if self.names is not None and (len(self.names) != self.J or len(set(self.names)) != self.J):
            raise L.EgError(f"JointTree: names: need {self.J} distinct names, got {len(self.names)} ({len(set(self.names))} distinct)")
        L.check(L.load().eg_articulate_check(*self.host_ptrs(), self.J), "eg_articulate_check")
        self.words = np.zeros(articulate_level_words(self.J), np.int32)
        L.check(L.load().eg_articulate_levels(*self.host_ptrs(), self.J, host_ptr(self.words)), "eg_articulate_levels")
        self._tables = BoundedCache()

    def host_ptrs(self):
        return host_ptr(self.parents), host_ptr(self.offsets32)

    @property
    def pose_dim(self) -> int:
        return 6 * self.J

    @property
    def basis_code(self) -> int:
        return _BASES[self.basis]

    @property
    def depth(self) -> np.ndarray:
        """Joints between the root and every joint, ``[J]`` (0 at the root)."""
        d = np.zeros(self.J, np.int64)
        for j in range(1, self.J):
            d[j] = d[self.parents[j]] + 1
        return d

    @property
    def levels(self) -> int:
        return int(self.words[0])

    def table(self, device) -> torch.Tensor:
        """int32 ``[articulate_level_words(J)]`` on ``device``: eg_articulate_levels' table."""
        return self._tables.get(str(device), lambda: torch.from_numpy(self.words).to(device))

    @classmethod
    def from_bvh(cls, text: str, joints: Optional[Sequence[str]] = None, unit: float = 0.01, basis: str = "rows") -> "JointTree":
        """The body of a BVH file's ``HIERARCHY`` block (``ROOT`` / ``JOINT`` / ``End Site`` / ``OFFSET``; ``CHANNELS`` and everything from
        ``MOTION`` on are ignored).  ``joints``: the names to keep, returned in file order (None: every joint, no end sites).  A kept joint's
        parent is its nearest kept ancestor and its offset the sum of the offsets along the skipped joints between them -- exact while the
        skipped joints stay at the identity rotation, which is what a data set that does not animate them means.  The first kept joint is
        the root and keeps its own offset only.  Offsets are scaled by ``unit`` (0.01: a file in centimetres).  Refuses by name: an unknown
        joint name, a duplicate, and a kept joint that does not descend from the first kept joint."""
        nodes: List[Tuple[str, int, List[float]]] = []                    # (name, parent node or -1, offset); end sites have the name None
        stack: List[int] = []
        pending: Optional[int] = None
        tokens = text.split()
        i = 0
        while i < len(tokens):
            tok = tokens[i]
            if tok == "MOTION":
                break
            if tok in ("ROOT", "JOINT") or (tok == "End" and i + 1 < len(tokens) and tokens[i + 1] == "Site"):
                if i + 1 >= len(tokens):
                    raise L.EgError(f"JointTree.from_bvh: {tok} without a name at the end of the text")
                nodes.append((None if tok == "End" else tokens[i + 1], stack[-1] if stack else -1, [0.0, 0.0, 0.0]))
                pending = len(nodes) - 1
                i += 2
                continue
            if tok == "{":
                if pending is None:
                    raise L.EgError("JointTree.from_bvh: '{' without ROOT / JOINT / End Site before it")
                stack.append(pending)
                pending = None
            elif tok == "}":
                if not stack:
                    raise L.EgError("JointTree.from_bvh: '}' without an open joint")
                stack.pop()
            elif tok == "OFFSET":
                if not stack or i + 3 >= len(tokens):
                    raise L.EgError("JointTree.from_bvh: OFFSET outside a joint, or without three numbers")
                try:
                    nodes[stack[-1]][2][:] = [float(v) for v in tokens[i + 1:i + 4]]
                except ValueError:
                    raise L.EgError(f"JointTree.from_bvh: OFFSET {' '.join(tokens[i + 1:i + 4])}: not three numbers")
                i += 3
            i += 1
        named = [k for k, nd in enumerate(nodes) if nd[0] is not None]
        if not named:
            raise L.EgError("JointTree.from_bvh: no ROOT / JOINT in the text (need the HIERARCHY block of a BVH file)")
        all_names = [nodes[k][0] for k in named]
        if joints is None:
            keep = list(all_names)
        else:
            keep = [str(n) for n in joints]
            for n in keep:
                if n not in all_names:
                    raise L.EgError(f"JointTree.from_bvh: joints: unknown joint name {n!r} (the file has {len(all_names)} joints)")
                if keep.count(n) > 1:
                    raise L.EgError(f"JointTree.from_bvh: joints: duplicate joint name {n!r}")
        if len(set(all_names)) != len(all_names):
            dup = next(n for n in all_names if all_names.count(n) > 1)
            raise L.EgError(f"JointTree.from_bvh: duplicate joint name {dup!r} in the file")
        kept = [k for k in named if nodes[k][0] in set(keep)]             # file order
        index = {k: j for j, k in enumerate(kept)}
        parents, offsets = [], []
        for j, k in enumerate(kept):
            off = np.array(nodes[k][2], np.float64)
            a = nodes[k][1]
            while j > 0 and a >= 0 and a not in index:                     # the skipped joints between a kept joint and its kept ancestor
                off = off + np.array(nodes[a][2], np.float64)
                a = nodes[a][1]
            if j > 0 and a < 0:
                raise L.EgError(f"JointTree.from_bvh: joints: {nodes[k][0]!r} does not descend from {nodes[kept[0]][0]!r}, the first kept "
                                "joint (the root of the body)")
            parents.append(-1 if j == 0 else index[a])
            offsets.append(off * float(unit))
        return cls(parents, np.array(offsets), basis=basis, names=[nodes[k][0] for k in kept])

    def __eq__(self, other):
        return (isinstance(other, JointTree) and self.basis == other.basis and np.array_equal(self.parents, other.parents)
                and np.array_equal(self.offsets, other.offsets))

    __hash__ = None

    def __repr__(self):
        return f"JointTree(joints={self.J}, levels={self.levels}, basis={self.basis!r})"


def _quat64(m: np.ndarray) -> np.ndarray:
    """m [..., 3, 3] -> the unit quaternion [..., 4], ``w >= 0``: the branch of the first largest of (trace, m00, m11, m22)."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[..., r, c] for r in range(3) for c in range(3))
    tr = m00 + m11 + m22
    one = np.ones_like(tr)
    cand = np.stack([np.stack([one + tr, m21 - m12, m02 - m20, m10 - m01], -1),
                     np.stack([m21 - m12, one + m00 - m11 - m22, m01 + m10, m02 + m20], -1),
                     np.stack([m02 - m20, m01 + m10, one - m00 + m11 - m22, m12 + m21], -1),
                     np.stack([m10 - m01, m02 + m20, m12 + m21, one - m00 - m11 + m22], -1)], -2)
    pick = np.argmax(np.stack([tr, m00, m11, m22], -1), -1)              # argmax: the first on ties
    q = np.take_along_axis(cand, pick[..., None, None], -2)[..., 0, :]
    q = q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)
    return np.where(q[..., :1] < 0, -q, q)


def _rot6d_matrices64(d: np.ndarray, columns: bool) -> np.ndarray:
    """d [..., 6] -> R [..., 3, 3] by Gram-Schmidt."""
    a1, a2 = d[..., :3], d[..., 3:]
    b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(-1, keepdims=True)), 1e-12)
    u2 = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = u2 / np.maximum(np.sqrt((u2 * u2).sum(-1, keepdims=True)), 1e-12)
    R = np.stack([b1, b2, np.cross(b1, b2)], -2)
    return np.swapaxes(R, -1, -2) if columns else R


def _rot6d_rows64(x: np.ndarray, J: int, mean, n_out: int, Lf: int, M: int) -> np.ndarray:
    """x [n, 6J] -> the 6-D vectors [n_out, J, 6] of the output frames: plus the mean, then blended; the chain runs on the blended frame."""
    x = x.reshape(len(x), J, 6)
    if mean is not None:
        x = x + mean.reshape(J, 6)
    return _resample64(x, n_out, Lf, M)


def _articulate64(v: np.ndarray, tree: JointTree, frames: List[int], mean, glob: bool, Lf: int, M: int):
    """v [B, T, 6J] float64, frames [B] -> (joints [B, T_out, J, 3], rotations [B, T_out, J, 4])."""
    J = tree.J

    def row(x, n, n_out):                                       # position | quaternion, seven numbers per joint
        x = _rot6d_rows64(x, J, mean, n_out, Lf, M)
        R = _rot6d_matrices64(x, tree.basis == "columns")
        G, p = np.zeros_like(R), np.zeros((n_out, J, 3))
        for j in range(J):
            a = int(tree.parents[j])
            if a < 0:
                G[:, j], p[:, j] = R[:, j], tree.offsets[j]
            else:
                G[:, j] = G[:, a] @ R[:, j]
                p[:, j] = p[:, a] + G[:, a] @ tree.offsets[j]
        return np.concatenate([p, _quat64(G if glob else R)], -1)
    out = _valid_rows64(v, frames, (J, 7), row, Lf, M)
    return out[..., :3], out[..., 3:]


def _first_two64(m: np.ndarray, tree: JointTree, mean) -> np.ndarray:
    """m [n, J, 3, 3] -> [n, 6J]: the first two rows (``basis="rows"``) or columns of every matrix as ``a1 | a2``, minus the mean."""
    if tree.basis == "columns":
        m = np.swapaxes(m, -1, -2)
    d = m[..., :2, :].reshape(len(m), 6 * tree.J)
    return d if mean is None else d - mean


def _rot6d64(q: np.ndarray, tree: JointTree, frames: List[int], mean) -> np.ndarray:
    """q [B, T, J, 4] float64 -> [B, T, 6J]."""
    def row(qn, n, _n_out):
        u = qn / np.maximum(np.sqrt((qn * qn).sum(-1, keepdims=True)), 1e-12)
        w, x, y, z = (u[..., i] for i in range(4))
        m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                      2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                      2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(n, tree.J, 3, 3)
        return _first_two64(m, tree, mean)
    return _valid_rows64(q, frames, (6 * tree.J,), row)


def launch_articulate(track: torch.Tensor, tree: JointTree, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
                      mean: Optional[torch.Tensor] = None, space: str = "local", ratio: Tuple[int, int] = (1, 1),
                      out_joints: Optional[torch.Tensor] = None, out_rotations: Optional[torch.Tensor] = None, joints: bool = True,
                      rotations: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """eg_articulate_forward on ``track [B, T, 6J]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``(joints [B, T_out, J, 3] or None,
    rotations [B, T_out, J, 4] or None)``: one launch on the current stream, nothing else (the level table is uploaded on first use per
    device: warm up before a capture).  ``joints`` / ``rotations``: which outputs to make (an output that is given is made; not neither).
    The other arguments as in ``launch_joints``."""
    B, T, D = track.shape
    if D != tree.pose_dim:
        raise L.EgError(f"launch_articulate: a tree of {tree.J} joints takes tracks of {tree.pose_dim} columns, got {D}")
    Lf, M = ratio
    t_out = -(-T * Lf // M)
    if out_joints is None and joints:
        out_joints = torch.empty((B, t_out, tree.J, 3), dtype=torch.float32, device=track.device)
    if out_rotations is None and rotations:
        out_rotations = torch.empty((B, t_out, tree.J, 4), dtype=torch.float32, device=track.device)
    if out_joints is None and out_rotations is None:
        raise L.EgError("launch_articulate: neither joints nor rotations asked for")
    if out_joints is not None and out_rotations is not None and out_joints.shape[1] != out_rotations.shape[1]:
        raise L.EgError(f"launch_articulate: out_joints has {out_joints.shape[1]} frames per row, out_rotations {out_rotations.shape[1]}")
    stride = (out_joints if out_joints is not None else out_rotations).shape[1]
    L.check(L.load().eg_articulate_forward(_ptr(track), B, T, *tree.host_ptrs(), tree.J, _ptr(tree.table(track.device)), _ptr(d_frames),
                                           int(draws), int(frame_unit), _ptr(mean), tree.basis_code, _space(space, "launch_articulate"), Lf, M,
                                           _ptr(out_joints), _ptr(out_rotations), stride, _stream(track.device)), "eg_articulate_forward")
    return out_joints, out_rotations


def launch_rot6d(quat: torch.Tensor, tree: JointTree, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
                 mean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_articulate_rot6d on ``quat [B, T, J, 4]`` -> ``[B, T, 6J]``: one launch on the current stream."""
    B, T = quat.shape[:2]
    if out is None:
        out = torch.empty(B, T, tree.pose_dim, dtype=torch.float32, device=quat.device)
    L.check(L.load().eg_articulate_rot6d(_ptr(quat), B, T, tree.J, _ptr(d_frames), int(draws), int(frame_unit), _ptr(mean), tree.basis_code,
                                         _ptr(out), _stream(quat.device)), "eg_articulate_rot6d")
    return out


def _articulate(track, tree, frames, mean, fps, space: str, want_joints: bool, who: str):
    """Both forward functions: the joints or the rotations of ``track`` under its leading axes."""
    tree = _track_checked(track, tree, JointTree, who)
    sp, pick = _space(space, who), 0 if want_joints else 1
    return _forward(track, tree, frames, mean, fps, who, (tree.J, 3 if want_joints else 4),
                    lambda x, fe, d_frames, d_mean: launch_articulate(x, tree, d_frames, fe.R, 1, d_mean, space, fe.ratio, joints=want_joints,
                                                                      rotations=not want_joints)[pick],
                    lambda v, fe, mean64: _articulate64(v, tree, fe.per_row, mean64, sp == L.EG_SKELETON_SPACE_GLOBAL, *fe.ratio)[pick])


def joints_from_rot6d(track, tree: JointTree, frames=None, mean=None, fps=None):
    """``track [..., T, 6J]`` with up to two leading axes -> ``joints [..., T_out, J, 3]`` in metres: every joint's 6-D rotation made a matrix
    by Gram-Schmidt (``tree.basis``), then forward kinematics over the tree's offsets: ``G_j = G_parent R_j``,
    ``p_j = p_parent + G_parent offsets[j]``, ``p_0 = offsets[0]``.  ``frames``, ``mean [6J]`` and ``fps`` as in ``joints_from_tracks``; on a
    resampled frame the 6-D vectors are blended (after the mean) and the chain runs on the blended frame.  A CUDA tensor: one kernel
    launch, fp32; numpy or a CPU tensor: the definition in float64.  With ``frames`` or ``fps`` the result is ``(joints, joint_frames)``."""
    return _articulate(track, tree, frames, mean, fps, "local", True, "joints_from_rot6d")


def rotations_from_rot6d(track, tree: JointTree, frames=None, mean=None, fps=None, space: str = "local"):
    """``track [..., T, 6J]`` -> ``rotations [..., T_out, J, 4]``: the unit quaternion ``(w, x, y, z)``, ``w >= 0``, of every joint's rotation
    ``R_j`` relative to its parent (``space="local"``: what a rig or a BVH channel takes) or of ``G_j`` relative to the root (``"global"``).
    A degenerate group (zero, or ``a1`` parallel to ``a2``) gives a finite value that is not a rotation.  The other arguments and the
    return as in ``joints_from_rot6d``; the rotations and joints of the same arguments describe the same pose."""
    return _articulate(track, tree, frames, mean, fps, space, False, "rotations_from_rot6d")


def rot6d_from_rotations(quat, tree: JointTree, frames=None, mean=None):
    """``quat [..., T, J, 4]`` (up to two leading axes) -> ``rot6d [..., T, 6J]``: every quaternion normalised (``q / max(|q|, 1e-12)``), the
    first two rows (``basis="rows"``) or columns of its matrix as ``a1 | a2``, minus ``mean [6J]`` when given: the ``seed_pose`` a BEAT
    generator takes from motion capture, the counterpart of ``dir_vec_from_joints``.  Zeros from ``frames[u]`` on.  CUDA in: the kernel,
    fp32; numpy / CPU in: float64."""
    who = "rot6d_from_rotations"
    tree = _inverse(quat, tree, JointTree, "quat", 4, who)
    return _per_frame(quat, 3, frames, who, (tree.pose_dim,),
                      lambda q, d_frames, R: launch_rot6d(q, tree, d_frames, R, 1, _mean_dev(mean, tree.pose_dim, q.device, who)),
                      lambda q, per_row: _rot6d64(q, tree, per_row, _mean_host(mean, tree.pose_dim, who)))


# ---- Euler channels of 6-D rotation tracks, their inverse, and the Euler filter ------------------------------------------------------------------
ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")               # the order codes of include/emogest.h: i = code // 2, the others up / down
UNWRAP_TILE_FRAMES = L.EG_UNWRAP_TILE_FRAMES


def order_codes(order, J: int, who: str = "order") -> np.ndarray:
    """One order string for all joints, or J strings -> int32 ``[J]`` codes.  Refuses by name an order that is no permutation of XYZ (one that
    repeats an axis, like ``ZXZ``, is a proper Euler order, not a Tait-Bryan one: BVH rotation channels never have it)."""
    names = [order] * J if isinstance(order, str) else list(order)
    if len(names) != J:
        raise L.EgError(f"{who}: {len(names)} orders for {J} joints (one string for all joints, or one per joint)")
    codes = []
    for j, o in enumerate(names):
        o = str(o).upper()
        if len(o) == 3 and set(o) <= set("XYZ") and len(set(o)) < 3:
            raise L.EgError(f"{who}: joint {j}: order {o!r} repeats an axis; the six Tait-Bryan orders are {', '.join(ORDERS)}")
        if o not in ORDERS:
            raise L.EgError(f"{who}: joint {j}: order {o!r}: need one of {', '.join(ORDERS)}")
        codes.append(ORDERS.index(o))
    return np.array(codes, np.int32)


def order_axes(code: int) -> Tuple[int, int, int, float]:
    """An order code -> its axes ``(i, j, k)`` and ``eps``: +1 for XYZ, YZX, ZXY (``j`` follows ``i`` cyclically), -1 for the others."""
    i, j, k = ("XYZ".index(ch) for ch in ORDERS[int(code)])
    return i, j, k, (1.0 if j == (i + 1) % 3 else -1.0)


def _euler_of_matrices64(R: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """R [..., J, 3, 3] -> (a, b, c) [..., J, 3] in radians: the definition of include/emogest.h in float64."""
    out = np.zeros(R.shape[:-2] + (3,))
    for jt, code in enumerate(codes):
        i, j, k, eps = order_axes(code)
        m = R[..., jt, :, :]
        s = eps * m[..., i, k]
        lock = 1.0 - np.abs(s) < 2.0 ** -20
        out[..., jt, 1] = np.arctan2(s, np.sqrt(m[..., i, i] ** 2 + m[..., i, j] ** 2))
        out[..., jt, 0] = np.where(lock, np.arctan2(eps * m[..., k, j], m[..., j, j]), np.arctan2(-eps * m[..., j, k], m[..., k, k]))
        out[..., jt, 2] = np.where(lock, 0.0, np.arctan2(-eps * m[..., i, j], m[..., i, i]))
    return out


def _axis_rotation64(axis: int, th: np.ndarray) -> np.ndarray:
    c, s = np.cos(th), np.sin(th)
    m = np.zeros(th.shape + (3, 3))
    u, v = (axis + 1) % 3, (axis + 2) % 3
    m[..., axis, axis] = 1.0
    m[..., u, u], m[..., u, v], m[..., v, u], m[..., v, v] = c, -s, s, c
    return m


def _matrices_of_euler64(e: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """(a, b, c) [..., J, 3] in radians -> R = R_i(a) R_j(b) R_k(c) [..., J, 3, 3]."""
    R = np.zeros(e.shape[:-1] + (3, 3))
    for jt, code in enumerate(codes):
        i, j, k, _eps = order_axes(code)
        R[..., jt, :, :] = _axis_rotation64(i, e[..., jt, 0]) @ _axis_rotation64(j, e[..., jt, 1]) @ _axis_rotation64(k, e[..., jt, 2])
    return R


def _unwrap64(p: np.ndarray, frames: List[int], period: float) -> np.ndarray:
    """p [B, T, C] float64 -> the definition in float64: ``out_t = p_t - c_t P``; frames from ``frames[b]`` on stay as they are."""
    out = np.array(p, np.float64)
    for b, n in enumerate(frames):
        if n > 1:
            k = np.rint(np.diff(out[b, :n], axis=0) / period)
            out[b, 1:n] -= np.cumsum(k, axis=0) * period
    return out


def _euler64(v: np.ndarray, tree: JointTree, codes: np.ndarray, frames: List[int], mean, Lf: int, M: int, degrees: bool) -> np.ndarray:
    """v [B, T, 6J] float64 -> [B, T_out, J, 3]."""
    def row(x, _n, n_out):
        e = _euler_of_matrices64(_rot6d_matrices64(_rot6d_rows64(x, tree.J, mean, n_out, Lf, M), tree.basis == "columns"), codes)
        return np.degrees(e) if degrees else e
    return _valid_rows64(v, frames, (tree.J, 3), row, Lf, M)


class _Orders:
    """The order codes of a call on the host and, once per device, on the device."""
    _cache = BoundedCache(64)

    @classmethod
    def get(cls, order, J: int, who: str):
        codes = order_codes(order, J, who)
        return cls._cache.get(codes.tobytes(), lambda: SimpleNamespace(codes=codes, dev=BoundedCache()))

    @staticmethod
    def table(entry, device) -> torch.Tensor:
        return entry.dev.get(str(device), lambda: torch.from_numpy(entry.codes).to(device))


def launch_euler(track: torch.Tensor, tree: JointTree, order, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
                 mean: Optional[torch.Tensor] = None, ratio: Tuple[int, int] = (1, 1), degrees: bool = True,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_articulate_euler on ``track [B, T, 6J]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``[B, T_out, J, 3]``: one launch on the current
    stream, nothing else (the order codes are uploaded on first use per device: warm up before a capture).  The other arguments as in
    ``launch_articulate``."""
    B, T, D = track.shape
    if D != tree.pose_dim:
        raise L.EgError(f"launch_euler: a tree of {tree.J} joints takes tracks of {tree.pose_dim} columns, got {D}")
    Lf, M = ratio
    if out is None:
        out = torch.empty((B, -(-T * Lf // M), tree.J, 3), dtype=torch.float32, device=track.device)
    o = _Orders.get(order, tree.J, "launch_euler: order")
    L.check(L.load().eg_articulate_euler(_ptr(track), B, T, tree.J, host_ptr(o.codes), _ptr(_Orders.table(o, track.device)), _ptr(d_frames),
                                         int(draws), int(frame_unit), _ptr(mean), tree.basis_code, int(bool(degrees)), Lf, M, _ptr(out),
                                         out.shape[1], _stream(track.device)), "eg_articulate_euler")
    return out


def launch_rot6d_euler(euler: torch.Tensor, tree: JointTree, order, d_frames: Optional[torch.Tensor] = None, draws: int = 1,
                       frame_unit: int = 1, mean: Optional[torch.Tensor] = None, degrees: bool = True,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_articulate_rot6d_euler on ``euler [B, T, J, 3]`` -> ``[B, T, 6J]``: one launch on the current stream."""
    B, T = euler.shape[:2]
    if out is None:
        out = torch.empty(B, T, tree.pose_dim, dtype=torch.float32, device=euler.device)
    o = _Orders.get(order, tree.J, "launch_rot6d_euler: order")
    L.check(L.load().eg_articulate_rot6d_euler(_ptr(euler), B, T, tree.J, host_ptr(o.codes), _ptr(_Orders.table(o, euler.device)),
                                               _ptr(d_frames), int(draws), int(frame_unit), _ptr(mean), tree.basis_code, int(bool(degrees)),
                                               _ptr(out), _stream(euler.device)), "eg_articulate_rot6d_euler")
    return out


def unwrap_workspace(rows: int, T: int, C: int, device) -> Optional[torch.Tensor]:
    """The workspace ``launch_unwrap`` takes for ``[rows, T, C]``; None where the track fits one tile and none is needed."""
    if T <= UNWRAP_TILE_FRAMES:
        return None
    need = int(L.load().eg_angle_unwrap_workspace_bytes(int(rows), int(T), int(C)))
    if need <= 0:
        L.check(1, "eg_angle_unwrap_workspace_bytes")
    return torch.empty(need // 4, dtype=torch.int32, device=device)


def launch_unwrap(angles: torch.Tensor, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1, period: float = 360.0,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_angle_unwrap on ``angles [B, T, C]`` (contiguous fp32 CUDA), in place: up to three launches on the current stream, nothing else
    when ``workspace`` (``unwrap_workspace``) is given; without it one is allocated here."""
    B, T, Cc = angles.shape
    if workspace is None:
        workspace = unwrap_workspace(B, T, Cc, angles.device)
    L.check(L.load().eg_angle_unwrap(_ptr(angles), B, T, Cc, _ptr(d_frames), int(draws), int(frame_unit), float(period), _ptr(workspace),
                                     0 if workspace is None else workspace.numel() * 4, _stream(angles.device)), "eg_angle_unwrap")
    return angles


def _period_checked(period, who: str) -> float:
    p = float(period)
    if not (math.isfinite(p) and p > 0.0 and math.isfinite(float(np.float32(p))) and float(np.float32(p)) > 0.0):
        raise L.EgError(f"{who}: period={period!r} (need finite and > 0)")
    return p


def euler_from_rot6d(track, tree: JointTree, order, frames=None, mean=None, fps=None, degrees: bool = True, unwrap: bool = False):
    """``track [..., T, 6J]`` with up to two leading axes -> ``euler [..., T_out, J, 3]``: the angles ``(a, b, c)`` of every joint's rotation
    ``R_j = R_i(a) R_j(b) R_k(c)`` relative to its parent, in the order of the joint's BVH rotation channels, in degrees (``degrees=False``:
    radians).  ``order``: one of XYZ, XZY, YXZ, YZX, ZXY, ZYX for all joints, or J of them; ``CHANNELS 3 Zrotation Xrotation Yrotation`` is
    ``"ZXY"``.  With ``eps = +1`` for XYZ, YZX, ZXY and ``-1`` for the others: ``s = eps R[i][k]``, ``b = atan2(s, sqrt(R[i][i]^2 +
    R[i][j]^2))`` in ``[-90, 90]``; ``a = atan2(-eps R[j][k], R[k][k])``, ``c = atan2(-eps R[i][j], R[i][i])`` while ``1 - |s| >= 2^-20``;
    at the lock ``a = atan2(eps R[k][j], R[j][j])``, ``c = 0``.  ``R_j`` is ``joints_from_rot6d``'s (mean, blend of the 6-D vectors with
    ``fps``, Gram-Schmidt, ``tree.basis``), so the angles, the quaternions and the joints of the same arguments describe one pose.
    ``unwrap=True`` then runs ``unwrap_angles`` over the result: whole turns are taken out along time.  Only whole turns: the middle angle
    stays in ``[-90, 90]`` by definition, so the other Euler triple of a rotation is never chosen and ``a`` / ``c`` still jump by 180 degrees
    where a joint passes through the lock.  A CUDA tensor: one launch (plus the unwrap launches), fp32; numpy or a CPU tensor: float64.
    With ``frames`` or ``fps`` the result is ``(euler, joint_frames)``; zeros from ``joint_frames[u]`` on."""
    who = "euler_from_rot6d"
    tree = _track_checked(track, tree, JointTree, who)
    o = _Orders.get(order, tree.J, f"{who}: order")
    period = 360.0 if degrees else 2.0 * math.pi

    def on_device(x, fe, d_frames, d_mean):
        res = launch_euler(x, tree, order, d_frames, fe.R, 1, d_mean, fe.ratio, degrees)
        return _unwrapped(res, fe, period) if unwrap else res

    def on_host(v, fe, mean64):
        res = _euler64(v, tree, o.codes, fe.per_row, mean64, *fe.ratio, degrees)
        if unwrap:
            n_rows = [n for n in fe.n_out for _ in range(fe.R)]
            res = _unwrap64(res.reshape(fe.U * fe.R, fe.t_out, 3 * tree.J), n_rows, period)
        return res
    return _forward(track, tree, frames, mean, fps, who, (tree.J, 3), on_device, on_host)


def _unwrapped(euler: torch.Tensor, fe: SimpleNamespace, period: float) -> torch.Tensor:
    """The Euler filter over ``euler [U * R, T_out, J, 3]`` on the device, in place, on the valid output frames of the front end ``fe``."""
    launch_unwrap(euler.view(fe.U * fe.R, fe.t_out, -1), frames_dev(fe.n_out if fe.fr is not None else None, euler.device), fe.R, 1, period)
    return euler


def rot6d_from_euler(euler, tree: JointTree, order, frames=None, mean=None, degrees: bool = True):
    """``euler [..., T, J, 3]`` (up to two leading axes; degrees unless ``degrees=False``) -> ``rot6d [..., T, 6J]``: ``R = R_i(a) R_j(b)
    R_k(c)`` for the joint's ``order``, its first two rows (``basis="rows"``) or columns as ``a1 | a2``, minus ``mean [6J]`` when given:
    the ``seed_pose`` or the target track of a BEAT generator from a BVH file's channels.  Zeros from ``frames[u]`` on.  CUDA in: the
    kernel, fp32; numpy / CPU in: float64."""
    who = "rot6d_from_euler"
    tree = _inverse(euler, tree, JointTree, "euler", 3, who)
    o = _Orders.get(order, tree.J, f"{who}: order")

    def on_host(e, per_row):
        mh = _mean_host(mean, tree.pose_dim, who)
        return _valid_rows64(e, per_row, (tree.pose_dim,),
                             lambda en, _n, _n_out: _first_two64(_matrices_of_euler64(np.radians(en) if degrees else en, o.codes), tree, mh))
    return _per_frame(euler, 3, frames, who, (tree.pose_dim,),
                      lambda e, d_frames, R: launch_rot6d_euler(e, tree, order, d_frames, R, 1, _mean_dev(mean, tree.pose_dim, e.device, who), degrees),
                      on_host)


def unwrap_angles(angles, frames=None, period: float = 360.0):
    """The Euler filter on ``angles [..., T, C]`` (up to two leading axes; flatten ``[T, J, 3]`` to ``[T, 3J]`` first): every (row, column)
    series loses its whole-period jumps: ``k_t = nearbyint((p_t - p_(t-1)) / period)``, ``out_t = p_t - period (k_1 + .. + k_t)``:
    ``np.unwrap`` on tie-free input.  ``frames``: valid frames per recording; the rest stays as it is.  Returns a new tensor or array.
    CUDA in: fp32 on the device (the differences in fp32, the quotient in float64, ``fmaf(-c_t, period, p_t)``; up to three launches);
    numpy / CPU in: float64.  Only whole periods are removed: see ``euler_from_rot6d``."""
    who = "unwrap_angles"
    period = _period_checked(period, who)
    shape = tuple(angles.shape)
    if len(shape) < 2 or shape[-2] < 1 or shape[-1] < 1:
        raise L.EgError(f"{who}: angles shape {shape}: need [..., T >= 1, C >= 1]")
    return _per_frame(angles, 2, frames, who, shape[-1:], lambda a, d_frames, R: launch_unwrap(a.clone(), d_frames, R, 1, period),
                      lambda a, per_row: _unwrap64(a, per_row, period))


def euler_args(who: str, joints, euler, euler_unwrap: bool = False, unwrap_allowed: bool = True):
    """The ``euler=`` / ``euler_unwrap=`` arguments of a caller, checked before anything runs: the J order strings, or None.  ``euler``: an
    order for all joints, J orders, or a ``bvh.BvhFile`` (the orders of the tree's joints, by name)."""
    if euler is None:
        if euler_unwrap:
            raise L.EgError(f"{who}: euler_unwrap=True without euler=order")
        return None
    if not unwrap_allowed and euler_unwrap:
        raise L.EgError(f"{who}: euler_unwrap=True is not supported (a stream emits principal values: a whole turn is only known against the "
                        "frames before it); unwrap the finished track with skeleton.unwrap_angles")
    if joints is None:
        raise L.EgError(f"{who}: euler= without joints=tree (the angles belong to a JointTree's joints)")
    if isinstance(joints, Skeleton):
        raise L.EgError(f"{who}: euler= with joints=Skeleton: direction-vector bodies have no joint rotations (Euler channels need a "
                        "skeleton.JointTree and a generator of 6-D rotations)")
    if not isinstance(joints, JointTree):
        raise L.EgError(f"{who}: euler= needs joints=JointTree, got {type(joints).__name__}")
    if callable(getattr(euler, "orders", None)):                                   # a bvh.BvhFile
        if joints.names is None:
            raise L.EgError(f"{who}: euler=BvhFile needs a tree with joint names (BvhFile.tree(...))")
        euler = euler.orders(joints.names)
    return [ORDERS[c] for c in order_codes(euler, joints.J, f"{who}: euler")]




# ---- the output stage of the callers -------------------------------------------------------------------------------------------------------
class TrackOutputs:
    """The output stage of a caller (``synthesize``, ``GestureStream``: ``who``, the prefix of every message): the one place that knows which
    launches turn pose rows into the joints, rotations and Euler channels the caller asked for.  Construction checks the caller's arguments
    before anything runs, in two steps: here what needs no model (``streaming``: the caller is a stream, which refuses ``joints_fps`` and
    ``euler_unwrap``), in ``fit`` the rest against the model's ``pose_dim`` -- at once where ``pose_dim`` is given; ``hint`` ends the message
    about a skeleton that does not fit it.  Plain fields: ``body`` (the Skeleton or JointTree), ``tree`` (it is a JointTree), ``unit``,
    ``ratio`` (the reduced ``(L, M)`` of ``joints_fps``), ``rest`` (a RestPose; None without rotations, and with a tree, whose offsets are
    the bind pose), ``want_rotations``, ``space``, ``euler`` (the J order strings, or None), ``unwrap``, and ``made``: the outputs' names in
    launch order.  ``to(device)`` makes the device copies of the mean, the tables and the order codes and holds them: their addresses are
    what a captured graph replays."""

    def __init__(self, who: str, joints, joints_mean=None, joints_unit: bool = False, joints_fps=None, rotations=None,
                 rotations_space: str = "local", euler=None, euler_unwrap: bool = False, pose_dim: Optional[int] = None,
                 streaming: bool = False, hint: str = ""):
        self.who, self.streaming, self.hint = who, bool(streaming), hint
        self.body, self.tree = joints, isinstance(joints, JointTree)
        self.unit, self.fps, self.space, self.unwrap = bool(joints_unit), joints_fps, rotations_space, bool(euler_unwrap)
        self._mean, self._rotations, self._device = joints_mean, rotations, None
        if streaming and joints_fps is not None:
            raise L.EgError(f"{who}: joints_fps= is not supported (a frame-rate change needs the frame after the last one emitted, which a "
                            "stream does not have yet); resample the joints of the finished track with skeleton.joints_from_tracks(..., fps=); in a live "
                            "session: render=")
        if rotations is not None and joints is None:
            raise L.EgError(f"{who}: rotations= without joints=skeleton (the rest pose belongs to a skeleton's bones)")
        if pose_dim is not None:
            self.fit(pose_dim)
        self.euler = euler_args(who, joints, euler, euler_unwrap, unwrap_allowed=not streaming)
        self.orders = None if self.euler is None else _Orders.get(self.euler, joints.J, f"{who}: euler")

    def fit(self, pose_dim: int) -> Optional["TrackOutputs"]:
        """The second step: the arguments against each other and against the model's ``pose_dim``; returns the stage, or None when no output
        was asked for."""
        who, body, rotations = self.who, self.body, self._rotations
        if rotations is None and self.space != "local":
            raise L.EgError(f"{who}: rotations_space without rotations=rest")
        if body is None:
            if self._mean is not None or self.unit or self.fps is not None:
                raise L.EgError(f"{who}: joints_mean / joints_unit{'' if self.streaming else ' / joints_fps'} without joints=skeleton")
            return None
        if self.tree:                                                                  # the second body type: 6-D joint rotations
            if body.pose_dim != pose_dim:
                raise L.EgError(f"{who}: joints=: the joint tree has J={body.J} joints, 6J={body.pose_dim} != pose_dim={pose_dim}")
            if self.unit:
                raise L.EgError(f"{who}: joints_unit=True with joints=JointTree (Gram-Schmidt already normalises the 6-D rotations; joints_unit "
                                "re-normalises a Skeleton's bone vectors)")
            if rotations is not None and rotations is not True:
                raise L.EgError(f"{who}: rotations= with joints=JointTree takes True, got {type(rotations).__name__} (the tree's offsets are the "
                                "bind pose: there is no rest)")
        elif not isinstance(body, Skeleton):
            raise L.EgError(f"{who}: joints= takes a skeleton.Skeleton, got {type(body).__name__}")
        elif body.pose_dim != pose_dim:
            raise L.EgError(f"{who}: joints=: the skeleton has K={body.K} bones, 3K={body.pose_dim} != pose_dim={pose_dim}{self.hint}")
        self.ratio = rate_ratio(self.fps, f"{who}: joints_fps")                        # refuses an unsupported ratio
        self.want_rotations, self.rest = rotations is not None, None
        if self.want_rotations:
            _space(self.space, f"{who}: rotations_space")                              # and a bad space or rest pose
            self.rest = None if self.tree else body.rest_pose(rotations)
        return self

    @property
    def made(self) -> Tuple[str, ...]:
        return ("joints",) + ("rotations",) * self.want_rotations + ("euler",) * (self.euler is not None)

    def to(self, device) -> "TrackOutputs":
        """The device copies, made once per device: ``mean`` here, the tables and the order codes where they are cached, held here."""
        if self._device != str(device):
            self.mean = _mean_dev(self._mean, self.body.pose_dim, device, f"{self.who}: joints_mean")
            self._held = (self.body.table(device), self.rest and self.rest.table(device), self.orders and _Orders.table(self.orders, device))
            self._device = str(device)
        return self

    def launch(self, rows: torch.Tensor, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
               want: Sequence[str] = ("joints", "rotations", "euler")) -> dict:
        """Those of the outputs ``want`` names that the caller asked for, of ``rows [B, T, pose_dim]`` (contiguous fp32 on the device of
        ``to``, 16-byte aligned; ``d_frames``, ``draws``, ``frame_unit`` as in ``launch_joints``) -> ``{name: [B, T_out, ., .]}``.  Nothing
        but the launches, so it can be captured: a tree's joints and rotations from one ``launch_articulate`` and its Euler channels from
        one ``launch_euler``; a skeleton's from ``launch_joints`` and ``launch_rotations``."""
        j, q, e = (n in want and n in self.made for n in ("joints", "rotations", "euler"))
        args, out = (d_frames, draws, frame_unit, self.mean), {}
        if self.tree and (j or q):
            out["joints"], out["rotations"] = launch_articulate(rows, self.body, *args, self.space if q else "local", self.ratio, joints=j, rotations=q)
        if not self.tree and j:
            out["joints"] = launch_joints(rows, self.body, *args, self.unit, self.ratio)
        if not self.tree and q:
            out["rotations"] = launch_rotations(rows, self.body, self.rest, *args, self.space, self.ratio)
        if e:
            out["euler"] = launch_euler(rows, self.body, self.euler, *args, self.ratio)
        return {n: v for n, v in out.items() if v is not None}

    def tracks(self, poses: torch.Tensor, frames) -> dict:
        """Whole tracks ``poses [U, (R,) T, pose_dim]`` with ``frames [U]`` valid poses per recording -> every output under the leading axes
        of ``poses``, ``[U, (R,) T_out, ., .]``, and ``"joint_frames"``, the valid output frames per recording; the Euler channels
        unwrapped where the caller asked for it."""
        fe = _front(poses, self.body, frames, self.fps, f"{self.who}: joints")
        x = dev32(poses).reshape(fe.U * fe.R, fe.T, self.body.pose_dim)
        out = self.to(x.device).launch(x, frames_dev(fe.fr, x.device), fe.R)
        if self.unwrap:
            _unwrapped(out["euler"], fe, 360.0)
        return dict({n: v.reshape(fe.lead + tuple(v.shape[1:])) for n, v in out.items()}, joint_frames=fe.n_out)
