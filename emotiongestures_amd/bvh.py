"""BVH in and out (host only): the text format the BEAT data set ships its motion capture in and every animation tool opens.

``parse(text) -> BvhFile``           every node of ``HIERARCHY`` (name, parent, ``OFFSET``, channel list, end sites), ``frames``,
                                     ``frame_time`` and ``motion [F, C]`` float64 (None for a header-only text)
``BvhFile.tree(joints, unit, basis)``  the body, equal to ``JointTree.from_bvh`` on the same text
``BvhFile.orders(joints)``           the rotation order of every kept joint, e.g. ``"ZXY"`` for ``Zrotation Xrotation Yrotation``
``BvhFile.euler(joints)``            ``[F, J, 3]`` degrees in channel order: what ``skeleton.rot6d_from_euler`` takes
``BvhFile.root_position()``          ``[F, 3]`` in file units
``BvhFile.rot6d(tree, mean, device)``  the motion as a 6-D rotation track: a ``seed_pose`` or an evaluation target
``BvhFile.format(euler, ...)`` / ``write(path, euler, ...)``  one take as BVH text: the file's own ``HIERARCHY`` verbatim, then ``MOTION``

Convention: ``CHANNELS 3 Zrotation Xrotation Yrotation`` means ``R = Rz(a) Rx(b) Ry(c)`` with ``v_parent = R v_local``, angles in degrees: the
``R_j`` of ``skeleton.joints_from_rot6d``.  Position channels: the root's are its position in file units; any other joint's are written as
that joint's ``OFFSET`` and ignored on read (a body's bone lengths do not change with time here; ``JointTree`` takes them from ``OFFSET``).
A joint that is not kept (``joints=``) is written with zero rotation channels, which is what ``JointTree.from_bvh`` assumes of skipped joints.
The text is formatted on the host: one take per call, numbers as ``%.6f``.
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import skeleton as S

__all__ = ["parse", "read", "BvhFile", "BvhNode"]

_CHANNEL_WORDS = ("Xposition", "Yposition", "Zposition", "Xrotation", "Yrotation", "Zrotation")
_STRUCTURE = ("ROOT", "JOINT", "End", "{", "}", "OFFSET", "CHANNELS", "HIERARCHY", "MOTION")


class BvhNode:
    """One node of the hierarchy.  ``name`` is None for an end site; ``parent`` indexes ``BvhFile.nodes`` (-1 at the root); ``channels`` are
    the node's channel words in file order and ``first`` the column of the first of them in a ``MOTION`` row."""

    def __init__(self, name: Optional[str], parent: int):
        self.name, self.parent = name, parent
        self.offset = [0.0, 0.0, 0.0]
        self.channels: List[str] = []
        self.first = 0

    @property
    def rotation_columns(self) -> List[int]:
        return [self.first + i for i, c in enumerate(self.channels) if c.endswith("rotation")]

    @property
    def order(self) -> str:
        return "".join(c[0] for c in self.channels if c.endswith("rotation"))


def _canonical(word: str) -> Optional[str]:
    for w in _CHANNEL_WORDS:
        if w.lower() == word.lower():
            return w
    return None


def parse(text: str) -> "BvhFile":
    """The whole of a BVH text.  Refuses by name: a ``CHANNELS`` count that does not match its list, an unknown channel word, a joint whose
    rotation channels repeat an axis (or are not three), a ``MOTION`` row of the wrong width, a frame count that does not match the rows."""
    who = "bvh.parse"
    cut = re.search(r"(?m)^[ \t]*MOTION\b", text)
    hierarchy = text if cut is None else text[:cut.start()]
    nodes: List[BvhNode] = []
    stack: List[int] = []
    pending: Optional[int] = None
    tokens = hierarchy.split()
    width = 0
    i = 0
    while i < len(tokens):
        tok = tokens[i]
        if tok in ("ROOT", "JOINT") or (tok == "End" and i + 1 < len(tokens) and tokens[i + 1] == "Site"):
            if i + 1 >= len(tokens):
                raise L.EgError(f"{who}: {tok} without a name at the end of the text")
            nodes.append(BvhNode(None if tok == "End" else tokens[i + 1], stack[-1] if stack else -1))
            pending = len(nodes) - 1
            i += 2
            continue
        if tok == "{":
            if pending is None:
                raise L.EgError(f"{who}: '{{' without ROOT / JOINT / End Site before it")
            stack.append(pending)
            pending = None
        elif tok == "}":
            if not stack:
                raise L.EgError(f"{who}: '}}' without an open joint")
            stack.pop()
        elif tok == "OFFSET":
            if not stack or i + 3 >= len(tokens):
                raise L.EgError(f"{who}: OFFSET outside a joint, or without three numbers")
            try:
                nodes[stack[-1]].offset = [float(v) for v in tokens[i + 1:i + 4]]
            except ValueError:
                raise L.EgError(f"{who}: OFFSET {' '.join(tokens[i + 1:i + 4])}: not three numbers")
            i += 3
        elif tok == "CHANNELS":
            if not stack:
                raise L.EgError(f"{who}: CHANNELS outside a joint")
            nd = nodes[stack[-1]]
            label = nd.name if nd.name is not None else "an End Site"
            try:
                count = int(tokens[i + 1])
            except (IndexError, ValueError):
                raise L.EgError(f"{who}: joint {label!r}: CHANNELS without a count")
            words = []
            k = i + 2
            while k < len(tokens) and tokens[k] not in _STRUCTURE:
                words.append(tokens[k])
                k += 1
            for w in words:
                if _canonical(w) is None:
                    raise L.EgError(f"{who}: joint {label!r}: unknown channel word {w!r} (need one of {', '.join(_CHANNEL_WORDS)})")
            if len(words) != count:
                raise L.EgError(f"{who}: joint {label!r}: CHANNELS {count} is followed by {len(words)} channel words")
            nd.channels = [_canonical(w) for w in words]
            rot = nd.order
            if len(set(rot)) != len(rot):
                raise L.EgError(f"{who}: joint {label!r}: rotation channels {rot!r} repeat an axis (the six Tait-Bryan orders are "
                                f"{', '.join(S.ORDERS)})")
            if len(rot) not in (0, 3):
                raise L.EgError(f"{who}: joint {label!r}: {len(rot)} rotation channels {rot!r} (need all three axes, or none)")
            nd.first = width
            width += count
            i = k - 1
        i += 1
    if not any(nd.name is not None for nd in nodes):
        raise L.EgError(f"{who}: no ROOT / JOINT in the text (need the HIERARCHY block of a BVH file)")
    frames = frame_time = motion = None
    if cut is not None:
        lines = [ln.strip() for ln in text[cut.end():].splitlines() if ln.strip()]
        rows: List[str] = []
        for ln in lines:
            m = re.match(r"(?i)frames\s*:\s*(\S+)$", ln)
            t = re.match(r"(?i)frame\s+time\s*:\s*(\S+)$", ln)
            try:
                if m and frames is None and not rows:
                    frames = int(m.group(1))
                elif t and frame_time is None and not rows:
                    frame_time = float(t.group(1))
                else:
                    rows.append(ln)
            except ValueError:
                raise L.EgError(f"{who}: MOTION: {ln!r}: not a number")
        if frames is None or frame_time is None:
            raise L.EgError(f"{who}: MOTION without 'Frames:' and 'Frame Time:'")
        data = np.zeros((len(rows), width))
        for r, ln in enumerate(rows):
            vals = ln.split()
            if len(vals) != width:
                raise L.EgError(f"{who}: MOTION row {r} has {len(vals)} numbers, the hierarchy has {width} channels")
            try:
                data[r] = [float(v) for v in vals]
            except ValueError:
                raise L.EgError(f"{who}: MOTION row {r}: not {width} numbers")
        if len(rows) != frames:
            raise L.EgError(f"{who}: MOTION: Frames: {frames} but {len(rows)} rows")
        motion = data
    return BvhFile(hierarchy, nodes, width, frames, frame_time, motion)


def read(path: str) -> "BvhFile":
    with open(path) as fh:
        return parse(fh.read())


class BvhFile:
    """A parsed BVH text: ``hierarchy`` (the text before ``MOTION``, verbatim), ``nodes``, ``channels`` (the width of a ``MOTION`` row),
    ``frames``, ``frame_time`` and ``motion [F, C]`` float64 -- the last three None for a header-only text."""

    def __init__(self, hierarchy: str, nodes: List[BvhNode], channels: int, frames, frame_time, motion):
        self.hierarchy, self.nodes, self.channels = hierarchy, nodes, channels
        self.frames, self.frame_time, self.motion = frames, frame_time, motion

    @property
    def names(self) -> List[str]:
        return [nd.name for nd in self.nodes if nd.name is not None]

    def _kept(self, joints: Optional[Sequence[str]], who: str) -> List[BvhNode]:
        """The kept joints in file order; the names are checked as ``JointTree.from_bvh`` checks them."""
        named = [nd for nd in self.nodes if nd.name is not None]
        if joints is None:
            return named
        keep = [str(n) for n in joints]
        have = set(self.names)
        for n in keep:
            if n not in have:
                raise L.EgError(f"{who}: joints: unknown joint name {n!r} (the file has {len(named)} joints)")
            if keep.count(n) > 1:
                raise L.EgError(f"{who}: joints: duplicate joint name {n!r}")
        return [nd for nd in named if nd.name in set(keep)]

    def _rotating(self, joints, who: str) -> List[BvhNode]:
        kept = self._kept(joints, who)
        for nd in kept:
            if len(nd.order) != 3:
                raise L.EgError(f"{who}: joint {nd.name!r} has no rotation channels")
        return kept

    def _motion(self, who: str) -> np.ndarray:
        if self.motion is None:
            raise L.EgError(f"{who}: the text has no MOTION block")
        return self.motion

    def tree(self, joints: Optional[Sequence[str]] = None, unit: float = 0.01, basis: str = "rows") -> S.JointTree:
        """``JointTree.from_bvh`` of this file's hierarchy."""
        return S.JointTree.from_bvh(self.hierarchy, joints=joints, unit=unit, basis=basis)

    def orders(self, joints: Optional[Sequence[str]] = None) -> List[str]:
        """The rotation order of the kept joints, in file order: the ``order`` argument of ``skeleton.euler_from_rot6d``."""
        return [nd.order for nd in self._rotating(joints, "BvhFile.orders")]

    def euler(self, joints: Optional[Sequence[str]] = None) -> np.ndarray:
        """``[F, J, 3]`` float64: the rotation channels of the kept joints, degrees, in channel order."""
        who = "BvhFile.euler"
        motion = self._motion(who)
        cols = [c for nd in self._rotating(joints, who) for c in nd.rotation_columns]
        return np.ascontiguousarray(motion[:, cols]).reshape(len(motion), -1, 3)

    def _root_columns(self) -> List[Optional[int]]:
        root = self.nodes[0]
        return [root.first + root.channels.index(w) if w in root.channels else None for w in _CHANNEL_WORDS[:3]]

    def root_position(self) -> np.ndarray:
        """``[F, 3]`` float64 in file units: the root's position channels (its ``OFFSET`` on an axis it has no channel for)."""
        motion = self._motion("BvhFile.root_position")
        out = np.tile(np.asarray(self.nodes[0].offset, np.float64), (len(motion), 1))
        for axis, c in enumerate(self._root_columns()):
            if c is not None:
                out[:, axis] = motion[:, c]
        return out

    def rot6d(self, tree: S.JointTree, mean=None, device=None):
        """The file's motion as ``[F, 6J]`` for ``tree`` (made by ``tree()`` of this file, so that it has the joints' names): through
        ``skeleton.rot6d_from_euler``.  ``device=None``: float64 numpy; a CUDA device: fp32 there, by the kernel."""
        who = "BvhFile.rot6d"
        if not isinstance(tree, S.JointTree) or tree.names is None:
            raise L.EgError(f"{who}: tree must be a JointTree with names (BvhFile.tree(...))")
        e = self.euler(tree.names)
        orders = self.orders(tree.names)
        if device is not None:
            e = torch.from_numpy(e).to(device=device, dtype=torch.float32)
        return S.rot6d_from_euler(e, tree, orders, mean=mean)

    def format(self, euler, joints: Optional[Sequence[str]] = None, frame_time: Optional[float] = None, root_position=None) -> str:
        """One take as BVH text.  ``euler [T, J, 3]``: degrees in channel order for the kept joints (``joints``: as in ``tree``; a CUDA tensor
        is copied to the host once).  The file's ``HIERARCHY`` text verbatim, then ``MOTION``: joints that are not kept get zero rotation
        channels; the root's position channels hold ``root_position [T, 3]`` (file units) or the root's ``OFFSET``; position channels of any
        other joint hold that joint's ``OFFSET`` (and ``parse`` ignores them: ``euler`` / ``root_position`` never read them).
        ``frame_time``: seconds per frame, default the file's own.  Numbers are written as ``%.6f``."""
        who = "BvhFile.format"
        kept = self._rotating(joints, who)
        if isinstance(euler, torch.Tensor):
            euler = euler.detach().cpu().numpy()
        e = np.asarray(euler, np.float64)
        if e.ndim != 3 or e.shape[1:] != (len(kept), 3):
            raise L.EgError(f"{who}: euler shape {tuple(e.shape)}: need [T, {len(kept)}, 3] (one take, {len(kept)} kept joints)")
        if frame_time is None:
            frame_time = self.frame_time
        if frame_time is None or not (float(frame_time) > 0.0 and np.isfinite(float(frame_time))):
            raise L.EgError(f"{who}: frame_time={frame_time!r} (the text has no MOTION block to take it from: need seconds per frame > 0)")
        T = len(e)
        motion = np.zeros((T, self.channels))
        for nd in self.nodes:
            for i, w in enumerate(nd.channels):
                if w.endswith("position"):
                    motion[:, nd.first + i] = nd.offset["XYZ".index(w[0])]
        for jt, nd in enumerate(kept):
            motion[:, nd.rotation_columns] = e[:, jt]
        if root_position is not None:
            if isinstance(root_position, torch.Tensor):
                root_position = root_position.detach().cpu().numpy()
            rp = np.asarray(root_position, np.float64)
            if rp.shape != (T, 3):
                raise L.EgError(f"{who}: root_position shape {tuple(rp.shape)}: need [{T}, 3]")
            for axis, c in enumerate(self._root_columns()):
                if c is not None:
                    motion[:, c] = rp[:, axis]
        fmt = " ".join(["%.6f"] * self.channels)
        head = self.hierarchy if self.hierarchy.endswith("\n") else self.hierarchy + "\n"
        return head + "MOTION\nFrames: %d\nFrame Time: %.6f\n" % (T, float(frame_time)) + "\n".join(fmt % tuple(row) for row in motion) + "\n"

    def write(self, path: str, euler, joints: Optional[Sequence[str]] = None, frame_time: Optional[float] = None, root_position=None) -> None:
        """``format(...)`` into the file ``path``."""
        text = self.format(euler, joints, frame_time, root_position)
        with open(path, "w") as fh:
            fh.write(text)

    def __repr__(self):
        return f"BvhFile(joints={len(self.names)}, channels={self.channels}, frames={self.frames})"
