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
``format`` builds the text on the host: one take per call, numbers as ``%.6f``.

``BvhFile.format_tracks(euler, frames, ...) -> BvhText`` / ``write_tracks(paths, euler, ...)``  every take of ``[U, (R,) T, J, 3]`` at once.  For
a CUDA tensor the ``MOTION`` lines are formatted on the device (include/emogest.h, "BVH text of whole takes": eg_bvh_text_measure, one small
copy of the sizes to the host -- the one synchronisation, which the allocation of the text needs --, eg_bvh_text_write) and come to the host
in one copy; numpy or a CPU tensor goes through ``format`` per take.  ``BvhText.text(u, r)`` is by definition ``format(euler[u, r, :n], ...)``.
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence

import numpy as np
import torch

import ctypes as C
import os

from . import _lib as L
from . import _rows as R_
from . import skeleton as S
from ._host import device_bytes, host_ptr, ptr, sized, stream

__all__ = ["parse", "read", "BvhFile", "BvhNode", "BvhText", "TextKernels", "TEXT_TILE_FRAMES", "TEXT_MAX_CHANNELS"]

TEXT_TILE_FRAMES, TEXT_MAX_CHANNELS = L.EG_BVH_TEXT_TILE_FRAMES, L.EG_BVH_TEXT_MAX_CHANNELS

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

    def _channel_sources(self, kept: List[BvhNode], root: bool) -> list:
        """What every column of a ``MOTION`` row of a written take holds, for ``format`` and ``format_tracks`` alike: ``("euler", k)`` element
        k of the take's angles ``[3J]`` of that frame (a kept joint's rotation channel), ``("root", axis)`` an axis of ``root_position``
        (the root's position channels, when ``root``), or ``("const", value)``: float64 zero for a rotation channel of a joint that is not
        kept, the node's ``OFFSET`` for a position channel."""
        sources = [("const", 0.0)] * self.channels
        for nd in self.nodes:
            for i, w in enumerate(nd.channels):
                if w.endswith("position"):
                    sources[nd.first + i] = ("const", nd.offset["XYZ".index(w[0])])
        for jt, nd in enumerate(kept):
            for k, c in enumerate(nd.rotation_columns):
                sources[c] = ("euler", 3 * jt + k)
        if root:
            for axis, c in enumerate(self._root_columns()):
                if c is not None:
                    sources[c] = ("root", axis)
        return sources

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
        rp = None
        if root_position is not None:
            if isinstance(root_position, torch.Tensor):
                root_position = root_position.detach().cpu().numpy()
            rp = np.asarray(root_position, np.float64)
            if rp.shape != (T, 3):
                raise L.EgError(f"{who}: root_position shape {tuple(rp.shape)}: need [{T}, 3]")
        flat = e.reshape(T, 3 * len(kept))
        motion = np.zeros((T, self.channels))
        for c, (kind, k) in enumerate(self._channel_sources(kept, rp is not None)):
            motion[:, c] = k if kind == "const" else (flat[:, k] if kind == "euler" else rp[:, k])
        fmt = " ".join(["%.6f"] * self.channels)
        head = self.hierarchy if self.hierarchy.endswith("\n") else self.hierarchy + "\n"
        return head + "MOTION\nFrames: %d\nFrame Time: %.6f\n" % (T, float(frame_time)) + "\n".join(fmt % tuple(row) for row in motion) + "\n"

    def write(self, path: str, euler, joints: Optional[Sequence[str]] = None, frame_time: Optional[float] = None, root_position=None) -> None:
        """``format(...)`` into the file ``path``."""
        text = self.format(euler, joints, frame_time, root_position)
        with open(path, "w") as fh:
            fh.write(text)

    def _text_head(self, frame_time, who: str):
        if frame_time is None:
            frame_time = self.frame_time
        if frame_time is None or not (float(frame_time) > 0.0 and np.isfinite(float(frame_time))):
            raise L.EgError(f"{who}: frame_time={frame_time!r} (the text has no MOTION block to take it from: need seconds per frame > 0)")
        head = self.hierarchy if self.hierarchy.endswith("\n") else self.hierarchy + "\n"
        return head, float(frame_time)

    def text_table(self, joints: Optional[Sequence[str]] = None, root: bool = False, who: str = "BvhFile.text_table") -> np.ndarray:
        """The channel table of eg_bvh_text_measure / eg_bvh_text_write for this file (include/emogest.h): uint8 ``[28 C]``, ``src int32 [C] |
        const_len int32 [C] | const_text [C][20]``.  The constants -- zero rotation channels of joints that are not kept, ``OFFSET`` values
        -- are formatted here, by ``"%.6f"`` of the float64 value as ``format`` does; ``root``: the root's position channels read
        ``root_position``."""
        Cn = self.channels
        if not 1 <= Cn <= TEXT_MAX_CHANNELS:
            raise L.EgError(f"{who}: the file has {Cn} channels (the device formats 1 .. {TEXT_MAX_CHANNELS})")
        src, clen, ctext = np.full(Cn, -4, np.int32), np.zeros(Cn, np.int32), np.zeros((Cn, 20), np.uint8)
        for c, (kind, k) in enumerate(self._channel_sources(self._rotating(joints, who), root)):
            if kind == "const":
                word = ("%.6f" % k).encode()
                if not 8 <= len(word) <= L.EG_BVH_TEXT_MAX_WIDTH:
                    raise L.EgError(f"{who}: channel {c}: OFFSET {k!r} is written as {len(word)} bytes (need 8 .. {L.EG_BVH_TEXT_MAX_WIDTH})")
                clen[c] = len(word)
                ctext[c, :len(word)] = np.frombuffer(word, np.uint8)
            else:
                src[c] = k if kind == "euler" else -1 - k
        return np.concatenate([src.view(np.uint8), clen.view(np.uint8), ctext.reshape(-1)])

    def format_tracks(self, euler, frames=None, joints: Optional[Sequence[str]] = None, frame_time: Optional[float] = None,
                      root_position=None) -> "BvhText":
        """Every take as BVH text.  ``euler [T, J, 3]``, ``[U, T, J, 3]`` or ``[U, R, T, J, 3]``: as in ``format``, with ``frames [U]`` valid
        frames per recording (at least 1; frames behind them are never read and may hold NaN).  ``root_position [T, 3]`` or ``[U, T, 3]``
        (one per recording, shared by its takes) is converted to fp32: the text is that of the fp32 values.  Returns a ``BvhText``.

        A CUDA tensor is formatted on the device: fp32 angles, ``"%.6f"`` of every value computed in integers (byte for byte what
        ``format`` gives for the same fp32 values), four launches and, between the third and the fourth, one small copy of the text's size to
        the host: the allocation needs it.  A value in a take's valid frames that is NaN, infinite or ``>= 2^31`` in magnitude is refused by
        name, with the first such take and its count, before any text is made (``format`` would print ``nan``, which no BVH reader takes).
        numpy or a CPU tensor: ``format`` per take, the same ``BvhText`` holding host bytes."""
        who = "BvhFile.format_tracks"
        kept = self._rotating(joints, who)
        shape = tuple(euler.shape)
        if not 3 <= len(shape) <= 5 or shape[-2:] != (len(kept), 3):
            raise L.EgError(f"{who}: euler shape {shape}: need [T, {len(kept)}, 3], [U, T, {len(kept)}, 3] or [U, R, T, {len(kept)}, 3] "
                            f"({len(kept)} kept joints)")
        head, ft = self._text_head(frame_time, who)
        lead, U, Rd = R_.lead_axes(shape, 3, who)
        T = shape[-3]
        rp = None
        if root_position is not None:
            rp = root_position.detach() if isinstance(root_position, torch.Tensor) else torch.from_numpy(np.asarray(root_position))
            rp = rp.to(torch.float32)
            if rp.dim() == 2:
                rp = rp[None]
            if tuple(rp.shape) != (U, T, 3):
                raise L.EgError(f"{who}: root_position shape {tuple(rp.shape)}: need [{T}, 3] or [{U}, {T}, 3] (one per recording)")

        def on_device(x, fr, d_frames, draws):
            k = TextKernels(self.text_table(joints, rp is not None, who), x, fr, d_frames, draws,
                            None if rp is None else rp.to(x.device).contiguous(), who)
            k.measure()
            total, offsets = k.sizes(lead)
            body = torch.empty(total, dtype=torch.uint8, device=x.device)
            k.write(body)
            return body, offsets

        def on_host(x, per_row):
            rows = []
            for b, n in enumerate(per_row):
                txt = self.format(x[b, :n], joints, ft, None if rp is None else rp[b // Rd, :n].cpu().numpy())
                rows.append(txt.encode("ascii")[len(head) + len("MOTION\nFrames: %d\nFrame Time: %.6f\n" % (n, ft)):])
            offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
            return np.frombuffer(b"".join(rows), np.uint8).copy(), offsets

        fe = R_.front(euler, 3, frames, who, on_device, on_host, min_frames=1, why="1")
        body, offsets = fe.res
        if isinstance(body, np.ndarray):
            body = torch.from_numpy(body)
        return BvhText(head, ft, lead, fe.fr if fe.fr is not None else [T] * U, fe.per_row, offsets, body)

    def write_tracks(self, paths, euler, frames=None, joints: Optional[Sequence[str]] = None, frame_time: Optional[float] = None,
                     root_position=None) -> List[str]:
        """``format_tracks(...).write(paths)``: one ``.bvh`` file per take; returns the paths."""
        return self.format_tracks(euler, frames, joints, frame_time, root_position).write(paths)

    def __repr__(self):
        return f"BvhFile(joints={len(self.names)}, channels={self.channels}, frames={self.frames})"


class TextKernels:
    """The two device calls for fixed buffers (include/emogest.h: eg_bvh_text_measure, eg_bvh_text_write): ``table`` from
    ``BvhFile.text_table``, ``euler [rows, T, J, 3]`` or ``[rows, T, 3J]`` contiguous fp32 CUDA, ``fr`` / ``d_frames`` the host and device
    counts per recording (both or neither), ``draws``, ``root [rows / draws, T, 3]`` fp32 on the same device or None.  Holds the table's
    upload, the workspace, ``line_off`` int64 ``[rows * T + 1]`` and ``summary``; ``measure()`` and ``write(text)`` do nothing but launch, so
    each can be captured in a graph and replayed on new values in the same ``euler`` / ``root`` / ``d_frames`` buffers."""

    def __init__(self, table: np.ndarray, euler: torch.Tensor, fr=None, d_frames: Optional[torch.Tensor] = None, draws: int = 1,
                 root: Optional[torch.Tensor] = None, who: str = "TextKernels"):
        if not (R_.is_cuda(euler) and euler.dtype == torch.float32 and euler.is_contiguous()):
            raise L.EgError(f"{who}: euler must be a contiguous fp32 CUDA tensor")
        self.who, self.rows, self.T = who, int(euler.shape[0]), int(euler.shape[1])
        self.C = len(table) // 28
        dev = euler.device
        self._host = (np.ascontiguousarray(table, np.uint8), R_.counts32(fr))
        self._held = (euler, root, d_frames, torch.from_numpy(self._host[0]).to(dev))
        self.args = L.EgBvhTextArgs(ptr(euler), ptr(root), host_ptr(self._host[0]), ptr(self._held[3]), host_ptr(self._host[1]), ptr(d_frames),
                                    self.rows, self.T, int(euler[0, 0].numel()), self.C, int(draws), 1)
        self.workspace = device_bytes("eg_bvh_text_workspace_bytes", dev, self.rows, self.T, self.C)
        self.line_off = torch.empty(self.rows * self.T + 1, dtype=torch.int64, device=dev)
        self.summary = torch.empty(1 + (self.rows + 1) // 2, dtype=torch.int64, device=dev)

    def measure(self) -> None:
        L.check(L.load().eg_bvh_text_measure(C.byref(self.args), ptr(self.workspace), self.workspace.numel(), ptr(self.line_off),
                                             ptr(self.summary), stream(self.line_off.device)), "eg_bvh_text_measure")

    def sizes(self, lead=None):
        """After ``measure``: ``(total bytes, offsets)``, ``offsets`` host int64 ``[rows + 1]``, the byte at which every row starts.  The
        copy to the host synchronises.  Refuses by name the first row with values that are not writable (``lead``: the leading axes, to
        name the take as the caller indexes it)."""
        both = torch.cat([self.summary, self.line_off[::self.T]]).cpu().numpy()
        bad = both[1:len(self.summary)].view(np.int32)[:self.rows]
        if bad.any():
            b = int(np.flatnonzero(bad)[0])
            draws = self.args.draws
            take = f"take [{b // draws}, {b % draws}] (row {b})" if lead is not None and len(lead) == 2 else f"row {b}"
            raise L.EgError(f"{self.who}: {take} has {int(bad[b])} values in its valid frames that are NaN, infinite or >= 2^31 in magnitude: "
                            "not writable as %.6f")
        return int(both[0]), both[len(self.summary):].copy()

    def write(self, text: torch.Tensor) -> None:
        """``text``: uint8 on the device, at least the measured total; bytes behind the total are left as they are."""
        L.check(L.load().eg_bvh_text_write(C.byref(self.args), ptr(self.line_off), ptr(text), text.numel(), stream(text.device)),
                "eg_bvh_text_write")


class BvhText:
    """The BVH text of every take of one ``format_tracks`` call.  ``lead``: the leading axes of the angles, ``()``, ``(U,)`` or ``(U, R)``;
    ``frames [U]``: valid frames per recording; ``offsets``: host int64 ``[rows + 1]``, row b's ``MOTION`` lines are
    ``body[offsets[b]:offsets[b + 1]]``; ``body``: uint8, on the device the angles were on.  Take (u, r) is row ``u * R + r``."""

    def __init__(self, head: str, frame_time: float, lead, frames, per_row, offsets, body: torch.Tensor):
        self._head, self.frame_time, self.lead, self.frames, self._per_row = head, frame_time, tuple(lead), list(frames), list(per_row)
        self.offsets, self.body, self._host = np.asarray(offsets, np.int64), body, None

    def _row(self, u: int, r: int) -> int:
        U = self.lead[0] if self.lead else 1
        Rd = self.lead[1] if len(self.lead) == 2 else 1
        if not (0 <= u < U and 0 <= r < Rd):
            raise L.EgError(f"BvhText: take ({u}, {r}) outside the leading axes {self.lead}")
        return u * Rd + r

    def head(self, u: int = 0, r: int = 0) -> str:
        """The file's ``HIERARCHY`` verbatim, ``MOTION``, ``Frames:`` and ``Frame Time:`` of take (u, r)."""
        return self._head + "MOTION\nFrames: %d\nFrame Time: %.6f\n" % (self._per_row[self._row(u, r)], self.frame_time)

    def host(self) -> np.ndarray:
        """The whole body on the host, uint8: one copy, made once."""
        if self._host is None:
            self._host = self.body.cpu().numpy()
        return self._host

    def tobytes(self, u: int = 0, r: int = 0) -> bytes:
        b = self._row(u, r)
        return self.head(u, r).encode() + self.host()[self.offsets[b]:self.offsets[b + 1]].tobytes()

    def text(self, u: int = 0, r: int = 0) -> str:
        """Take (u, r) as ``BvhFile.format`` gives it."""
        return self.tobytes(u, r).decode()

    def write(self, paths) -> List[str]:
        """One file per take from the one host copy.  ``paths``: a directory (made if missing; the files are ``take.bvh``, ``take_<u>.bvh``
        or ``take_<u>_<r>.bvh`` by the leading axes), or one path per row in row order.  Returns the paths."""
        U = self.lead[0] if self.lead else 1
        Rd = self.lead[1] if len(self.lead) == 2 else 1
        if isinstance(paths, (str, os.PathLike)):
            os.makedirs(paths, exist_ok=True)
            names = ["take" + ("" if not self.lead else f"_{u:03d}" + (f"_{r:02d}" if len(self.lead) == 2 else "")) + ".bvh"
                     for u in range(U) for r in range(Rd)]
            paths = [os.path.join(paths, n) for n in names]
        paths = [os.fspath(p) for p in paths]
        if len(paths) != U * Rd:
            raise L.EgError(f"BvhText.write: {len(paths)} paths for {U * Rd} takes")
        host = self.host()
        for b, path in enumerate(paths):
            with open(path, "wb") as fh:
                fh.write(self.head(b // Rd, b % Rd).encode())
                fh.write(host[self.offsets[b]:self.offsets[b + 1]].data)
        return paths

    def __repr__(self):
        return f"BvhText(lead={self.lead}, frames={self.frames}, bytes={int(self.offsets[-1])}, device={self.body.device})"
