"""Preview frames: stick figures of whole takes, one 8-bit picture per frame, drawn on the device (csrc/preview.hip).

The reference shows a generated take with matplotlib, one 3-D figure per frame (``utils/train_utils_expressive.py``: ``create_video_and_save``
draws the ``dir_vec_pairs`` bones of every pose).  Here the bones of every frame of every take are rasterised in one launch:

``Camera(matrix, centre)`` / ``Camera.orbit(...)``   an orthographic camera: pixel ``(u, v) = matrix @ (x, y, z) + centre``, image y downwards
``PreviewSpec(body, height, width, ...)``            what to draw: the bones, the picture, the camera, colours, layout and colour space
``render_joints(joints, spec, frames=None)``         ``[T, J, 3]``, ``[U, T, J, 3]`` or ``[U, R, T, J, 3]`` metres -> ``uint8`` pictures
                                                     ``[..., T, H, W, 3]`` (``layout="hwc"``) or ``[..., T, 3, H, W]`` (``"chw"``)
``write_y4m(path_or_file, frames, fps)``             one take ``[T, 3, H, W]`` in Y, Cb, Cr as an uncompressed YUV4MPEG2 stream
``side_by_side(a, b)``                               two renderings next to each other (the reference's "human | generated" figure)

One frame (include/emogest.h states the same).  Every ``+ - *`` is one IEEE fp32 operation in the order written, no fused multiply-add; the
square root and the reciprocal are correctly rounded; a comparison with a NaN is false::

    u_j = ((M00*x_j + M01*y_j) + M02*z_j) + c0        v_j likewise with row 1 of the camera
    picture = background;  per bone k = (ja, jb), in bone order:
        ax, ay = u_ja, v_ja;  ex = u_jb - ax;  ey = v_jb - ay;  l2 = ex*ex + ey*ey;  inv = 1 / l2 if l2 > 0 else 0
        per pixel (px, py), X = px + 0.5, Y = py + 0.5:
            wx = X - ax;  wy = Y - ay;  s = (wx*ex + wy*ey) * inv;  t = 0 if s < 0 else s;  t = 1 if t > 1 else t       (a NaN stays)
            dx = wx - t*ex;  dy = wy - t*ey;  a = (radius + 0.5) - sqrt(dx*dx + dy*dy)
            q = 255 if a >= 1 else int(a*255 + 0.5) if a > 0 else 0                                               (a NaN: q = 0)
            every channel:  c = (c*(255 - q) + colour[k]*q + 127) // 255

so later bones paint over earlier ones (as the reference's successive ``plot`` calls do), a bone of zero length is a disc, a bone with an end
that is not finite draws nothing, and only ``q`` depends on floating point.  Frames from a recording's ``frames[u]`` on are all-zero bytes and
their joints are never read (they may hold NaN).

CUDA tensors go through the kernel (one launch; there is no eager-PyTorch fallback).  numpy arrays and CPU tensors take the definition in numpy
float32 -- the same bytes -- and come back as numpy / CPU tensors, as in every other stage.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import _rows as RW
from ._host import BoundedCache, host_ptr, ptr as _ptr, stream as _stream

__all__ = ["Camera", "PreviewSpec", "render_joints", "launch_preview", "write_y4m", "side_by_side", "rgb_to_ycbcr", "MAX_BONES", "PALETTE"]

MAX_BONES = L.EG_PREVIEW_MAX_BONES
_LAYOUTS = {"hwc": L.EG_PREVIEW_HWC, "chw": L.EG_PREVIEW_CHW}
_SPACES = ("rgb", "ycbcr")
# the ten colours matplotlib's ``plot`` gives successive lines (its default property cycle)
PALETTE = np.array([(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
                    (127, 127, 127), (188, 189, 34), (23, 190, 207)], np.uint8)


def rgb_to_ycbcr(rgb) -> np.ndarray:
    """8-bit R, G, B ``[..., 3]`` -> BT.601 limited-range Y, Cb, Cr ``uint8``, in integers (``>>`` floors)::

        Y  = (( 66*R + 129*G +  25*B + 128) >> 8) + 16
        Cb = ((-38*R -  74*G + 112*B + 128) >> 8) + 128
        Cr = ((112*R -  94*G -  18*B + 128) >> 8) + 128

    Black is (16, 128, 128) and white (235, 128, 128)."""
    c = np.asarray(rgb).astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    cb = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    cr = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    return np.stack([y, cb, cr], -1).astype(np.uint8)


class Camera:
    """An orthographic camera: ``matrix [2, 3]`` and ``centre [2]`` fp32; pixel ``(u, v) = matrix @ (x, y, z) + centre``.  It is data to the
    kernel: nothing but these eight numbers enters a picture."""

    def __init__(self, matrix, centre):
        self.matrix = np.ascontiguousarray(matrix, np.float32)
        self.centre = np.ascontiguousarray(centre, np.float32)
        if self.matrix.shape != (2, 3) or self.centre.shape != (2,):
            raise L.EgError(f"Camera: matrix shape {self.matrix.shape}, centre shape {self.centre.shape}: need [2, 3] and [2]")
        if not (np.isfinite(self.matrix).all() and np.isfinite(self.centre).all()):
            raise L.EgError("Camera: matrix and centre must be finite")
        self.words = np.ascontiguousarray(np.concatenate([self.matrix.reshape(-1), self.centre]), np.float32)

    @classmethod
    def orbit(cls, azim: float = -60, elev: float = 20, span: float = 1.0, *, height: int, width: int, target=(0, 0, 0), up: str = "-y") -> "Camera":
        """The camera of a figure that looks at ``target`` from azimuth ``azim`` and elevation ``elev`` (degrees) about the ``up`` axis
        (``"x"``, ``"-y"``, ...; TED-Expressive data has y pointing down), ``width / span`` pixels per metre, ``target`` in the middle of the
        picture.  Built in float64, rounded once to fp32.  The defaults are the reference's ``view_init(elev=20, azim=-60)``."""
        axis = "xyz".find(up[-1:]) if isinstance(up, str) and up[-1:] and len(up) <= 2 and up[:-1] in ("", "+", "-") else -1
        if axis < 0:
            raise L.EgError(f"Camera.orbit: up={up!r}: one of 'x', 'y', 'z', '-x', '-y', '-z'")
        if not (float(span) > 0 and math.isfinite(float(span))):
            raise L.EgError(f"Camera.orbit: span={span!r} metres across the picture (finite and > 0)")
        eye = np.eye(3)
        n, h1, h2 = eye[axis], eye[(axis + 1) % 3], eye[(axis + 2) % 3]              # h1 x h2 = n
        if up[0] == "-":
            n, h1, h2 = -n, h2, h1
        a, e = math.radians(float(azim)), math.radians(float(elev))
        f = math.cos(e) * (math.cos(a) * h1 + math.sin(a) * h2) + math.sin(e) * n      # from the target towards the camera
        right = np.cross(n, f)
        if np.linalg.norm(right) < 1e-9:
            raise L.EgError(f"Camera.orbit: elev={elev!r}: looking along the up axis leaves the picture's horizontal undefined")
        right /= np.linalg.norm(right)
        upv = np.cross(f, right)
        s = float(width) / float(span)
        m = np.stack([s * right, -s * upv])                                            # image y downwards
        tgt = np.asarray(target, np.float64).reshape(3)
        return cls(m, np.array([width / 2.0, height / 2.0]) - m @ tgt)

    def __repr__(self):
        return f"Camera(matrix={self.matrix.tolist()}, centre={self.centre.tolist()})"


def _bones_of(body, bones) -> List[Tuple[int, int]]:
    if bones is not None:
        try:
            return [(int(a), int(b)) for a, b in bones]
        except (TypeError, ValueError):
            raise L.EgError(f"PreviewSpec: bones={bones!r}: a list of (joint, joint) pairs")
    if hasattr(body, "dir_vec_pairs"):                                                   # a Skeleton: the pairs the reference draws
        return [(int(p[0]), int(p[1])) for p in body.dir_vec_pairs]
    if hasattr(body, "offsets") and hasattr(body, "parents"):                          # a JointTree: a parent < 0 marks the root
        return [(int(p), j) for j, p in enumerate(body.parents) if j >= 1 and int(p) >= 0]
    raise L.EgError(f"PreviewSpec: body= takes a skeleton.Skeleton or a skeleton.JointTree, got {type(body).__name__}")


class PreviewSpec:
    """What ``render_joints`` draws.  ``body``: a ``skeleton.Skeleton`` (its ``dir_vec_pairs`` are the bones, in that order) or a
    ``skeleton.JointTree`` (``(parents[j], j)`` for ``j >= 1``); ``bones=`` overrides with a list of pairs.  ``height``, ``width``: 8..2048;
    ``radius``: half the line width in pixels, 0.25..16; ``camera``: a ``Camera`` (default ``Camera.orbit(height=, width=)``); ``palette
    [bones, 3]`` ``uint8`` (default: matplotlib's ten-colour cycle, repeated); ``background``; ``layout``: ``"hwc"`` or ``"chw"``;
    ``colorspace``: ``"rgb"``, or ``"ycbcr"``: palette and background go through ``rgb_to_ycbcr`` on the host and the channels are Y, Cb, Cr
    (the device is colour-space agnostic); ``max_bytes``: the largest output a call may make.  Anything out of range is refused by name."""

    def __init__(self, body, height: int, width: int, camera: Optional[Camera] = None, radius: float = 1.5, palette=None,
                 background=(255, 255, 255), layout: str = "hwc", colorspace: str = "rgb", max_bytes: int = 8 << 30, bones=None):
        who = "PreviewSpec"
        self.body = body
        self.bones = _bones_of(body, bones)
        self.J = int(body.J) if hasattr(body, "J") else None
        for name, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not L.EG_PREVIEW_MIN_SIZE <= int(v) <= L.EG_PREVIEW_MAX_SIZE:
                raise L.EgError(f"{who}: {name}={v!r}: an integer in {L.EG_PREVIEW_MIN_SIZE}..{L.EG_PREVIEW_MAX_SIZE}")
        self.height, self.width = int(height), int(width)
        try:
            self.radius = float(radius)
        except (TypeError, ValueError):
            self.radius = float("nan")
        if not L.EG_PREVIEW_MIN_RADIUS <= self.radius <= L.EG_PREVIEW_MAX_RADIUS:
            raise L.EgError(f"{who}: radius={radius!r} pixels: {L.EG_PREVIEW_MIN_RADIUS}..{L.EG_PREVIEW_MAX_RADIUS}")
        if len(self.bones) < 1 or len(self.bones) > MAX_BONES:
            raise L.EgError(f"{who}: {len(self.bones)} bones (1..EG_PREVIEW_MAX_BONES = {MAX_BONES})")
        self.table = np.ascontiguousarray(self.bones, np.int32).reshape(-1, 2)
        if self.J is not None or self.table.min() < 0:
            self.check(self.J if self.J is not None else 1 << 30)
        if layout not in _LAYOUTS:
            raise L.EgError(f"{who}: layout={layout!r}: 'hwc' or 'chw'")
        if colorspace not in _SPACES:
            raise L.EgError(f"{who}: colorspace={colorspace!r}: 'rgb' or 'ycbcr'")
        self.layout, self.colorspace = layout, colorspace
        self.camera = Camera.orbit(height=self.height, width=self.width) if camera is None else camera
        if not isinstance(self.camera, Camera):
            raise L.EgError(f"{who}: camera= takes a preview.Camera, got {type(camera).__name__}")
        K = len(self.bones)
        pal = PALETTE[np.arange(K) % len(PALETTE)] if palette is None else np.asarray(palette)
        if pal.shape != (K, 3) or pal.dtype != np.uint8:
            raise L.EgError(f"{who}: palette shape {pal.shape} dtype {pal.dtype}: need uint8 [{K}, 3], one colour per bone")
        bg = np.asarray(background)
        if bg.shape != (3,) or (bg < 0).any() or (bg > 255).any():
            raise L.EgError(f"{who}: background={background!r}: three values in 0..255")
        self.palette, self.background = pal.copy(), bg.astype(np.uint8)
        # the three bytes per bone the device composites, whatever they mean
        self.colours, self.ground = (rgb_to_ycbcr(self.palette), rgb_to_ycbcr(self.background)) if colorspace == "ycbcr" else (self.palette, self.background)
        self.max_bytes = int(max_bytes)
        self._tables = BoundedCache()

    def check(self, J: int) -> None:
        """eg_preview_check: the bones against a body of J joints."""
        L.check(L.load().eg_preview_check(host_ptr(self.table), len(self.bones), int(J)), "eg_preview_check")

    def words(self) -> np.ndarray:
        """The device table (include/emogest.h: EG_PREVIEW_TABLE_WORDS)."""
        pack = lambda c: int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
        used = sorted({j for pair in self.bones for j in pair})
        where = {j: i for i, j in enumerate(used)}
        w = np.zeros(L.EG_PREVIEW_TABLE_WORDS, np.int32)
        w[0], w[1], w[2] = len(self.bones), len(used), pack(self.ground)
        w[4:4 + len(used)] = used
        for k, (a, b) in enumerate(self.bones):
            w[4 + 2 * MAX_BONES + k], w[4 + 3 * MAX_BONES + k], w[4 + 4 * MAX_BONES + k] = where[a], where[b], pack(self.colours[k])
        return w

    def device_table(self, device) -> torch.Tensor:
        """int32 ``[EG_PREVIEW_TABLE_WORDS]`` on ``device``, uploaded once per device (warm up before a capture)."""
        return self._tables.get(str(device), lambda: torch.from_numpy(self.words()).to(device))

    def frame_shape(self) -> Tuple[int, int, int]:
        return (self.height, self.width, 3) if self.layout == "hwc" else (3, self.height, self.width)

    def out_bytes(self, rows: int, T: int) -> int:
        return int(rows) * int(T) * self.height * self.width * 3

    def fit(self, rows: int, T: int, who: str) -> None:
        """Refuses an output of ``rows`` takes of ``T`` frames that is larger than ``max_bytes``."""
        nbytes = self.out_bytes(rows, T)
        if nbytes > self.max_bytes:
            raise L.EgError(f"{who}: the preview of {rows} takes x {T} frames x {self.height} x {self.width} x 3 is {nbytes} bytes "
                            f"({nbytes / 2 ** 30:.2f} GiB) > max_bytes={self.max_bytes}: render fewer takes per call or a smaller picture")

    @classmethod
    def of(cls, spec, who: str = "preview") -> "PreviewSpec":
        """A PreviewSpec as it is; a dict: ``PreviewSpec(**dict)``."""
        if isinstance(spec, PreviewSpec):
            return spec
        if isinstance(spec, dict):
            return cls(**spec)
        raise L.EgError(f"{who}= takes a preview.PreviewSpec or a dict of its arguments, got {type(spec).__name__}")

    def __repr__(self):
        return (f"PreviewSpec(bones={len(self.bones)}, {self.height}x{self.width}, radius={self.radius:g}, layout={self.layout!r}, "
                f"colorspace={self.colorspace!r})")


def _render32(v: np.ndarray, per_row: Sequence[int], spec: PreviewSpec) -> np.ndarray:
    """The definition: v [B, T, J, 3] fp32 -> [B, T] pictures in spec.layout, all the frames of a row at once."""
    f32 = np.float32
    B, T = v.shape[:2]
    H, W = spec.height, spec.width
    out = np.zeros((B, T, H, W, 3), np.uint8)
    m, c = spec.camera.matrix, spec.camera.centre
    X = (np.arange(W, dtype=f32) + f32(0.5))[None, None, :]
    Y = (np.arange(H, dtype=f32) + f32(0.5))[None, :, None]
    reach = f32(spec.radius) + f32(0.5)
    ground, colours = spec.ground.astype(np.int32), spec.colours.astype(np.int32)
    with np.errstate(all="ignore"):
        for b, n in enumerate(per_row):
            if n == 0:
                continue
            p = v[b, :n]
            u = ((m[0, 0] * p[..., 0] + m[0, 1] * p[..., 1]) + m[0, 2] * p[..., 2]) + c[0]           # [n, J]
            w = ((m[1, 0] * p[..., 0] + m[1, 1] * p[..., 1]) + m[1, 2] * p[..., 2]) + c[1]
            img = np.empty((n, H, W, 3), np.int32)
            img[:] = ground
            for k, (ja, jb) in enumerate(spec.bones):
                ax, ay = u[:, ja, None, None], w[:, ja, None, None]
                ex, ey = u[:, jb, None, None] - ax, w[:, jb, None, None] - ay
                l2 = ex * ex + ey * ey
                inv = np.where(l2 > 0, f32(1) / l2, f32(0)).astype(f32)
                wx, wy = X - ax, Y - ay
                s = (wx * ex + wy * ey) * inv
                t = np.where(s < 0, f32(0), s)
                t = np.where(t > 1, f32(1), t)
                dx, dy = wx - t * ex, wy - t * ey
                a = reach - np.sqrt(dx * dx + dy * dy)
                part = a > 0
                q = np.where(a >= 1, 255, np.where(part, (np.where(part, a, f32(0)) * f32(255) + f32(0.5)).astype(np.int32), 0))[..., None]
                img = (img * (255 - q) + colours[k] * q + 127) // 255
            out[b, :n] = img.astype(np.uint8)
    return out if spec.layout == "hwc" else np.ascontiguousarray(out.transpose(0, 1, 4, 2, 3))


def launch_preview(joints: torch.Tensor, spec: PreviewSpec, d_frames: Optional[torch.Tensor] = None, draws: int = 1, frame_unit: int = 1,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eg_preview_raster on ``joints [B, T, J, 3]`` (contiguous fp32 CUDA, 16-byte aligned) -> ``uint8 [B, T, *spec.frame_shape()]``: one
    launch on the current stream, nothing else (the table is uploaded on first use per device: warm up before a capture).  ``d_frames``:
    device int32 ``[B / draws]`` or None."""
    B, T, J, _ = joints.shape
    if out is None:
        out = torch.empty((B, T) + spec.frame_shape(), dtype=torch.uint8, device=joints.device)
    L.check(L.load().eg_preview_raster(_ptr(joints), B, T, J, host_ptr(spec.table), len(spec.bones), _ptr(spec.device_table(joints.device)),
                                       host_ptr(spec.camera.words), spec.radius, spec.height, spec.width, _LAYOUTS[spec.layout], int(draws),
                                       int(frame_unit), _ptr(d_frames), _ptr(out), _stream(joints.device)), "eg_preview_raster")
    return out


def render_joints(joints, spec, frames=None):
    """``joints [..., T, J, 3]`` in metres with up to two leading axes (``[T, J, 3]``, ``[U, T, J, 3]``, ``[U, R, T, J, 3]``) -> the pictures
    ``uint8 [..., T, H, W, 3]`` (``spec.layout == "hwc"``) or ``[..., T, 3, H, W]`` (``"chw"``) of the module's definition.

    ``spec``: a ``PreviewSpec`` (or a dict of its arguments).  ``frames``: valid frames per recording (``[U]`` host ints, shared by the R
    rows of a recording): a frame from ``frames[u]`` on is all-zero bytes and its joints are never read.  Refused by name before anything
    runs: a shape that is not ``[..., T >= 1, J, 3]``, a bone that names a joint ``>= J``, bad ``frames``, an output above ``spec.max_bytes``.

    A CUDA tensor: one kernel launch, a CUDA result.  numpy or a CPU tensor: the definition in numpy float32 (numpy in: numpy out)."""
    who = "render_joints"
    spec = PreviewSpec.of(spec, f"{who}: spec")
    shape = tuple(joints.shape)
    if len(shape) < 3 or shape[-1] != 3 or shape[-2] < 1 or shape[-3] < 1:
        raise L.EgError(f"{who}: joints shape {shape}: need [..., T >= 1, J >= 1, 3]")
    spec.check(shape[-2])
    _lead, U, R = RW.lead_axes(shape, 3, who)
    spec.fit(U * R, shape[-3], who)
    fe = RW.front(joints, 3, frames, who, lambda x, fr, d_frames, R: launch_preview(x, spec, d_frames, R),
                  lambda v, per_row: _render32(v, per_row, spec), host=RW.host32)
    return fe.res.reshape(fe.lead + (fe.T,) + spec.frame_shape())


def _is_chw(shape) -> bool:
    return len(shape) >= 4 and shape[-1] != 3 and shape[-3] == 3


def side_by_side(a, b):
    """Two renderings of the same shape and layout next to each other, ``a`` on the left: concatenated along the width (the last axis of a
    ``"chw"`` rendering, the one before the channels of an ``"hwc"`` one)."""
    if tuple(a.shape[:-3]) != tuple(b.shape[:-3]) or len(a.shape) < 4:
        raise L.EgError(f"side_by_side: shapes {tuple(a.shape)} and {tuple(b.shape)}: two renderings of the same takes")
    if _is_chw(a.shape) != _is_chw(b.shape):
        raise L.EgError(f"side_by_side: shapes {tuple(a.shape)} and {tuple(b.shape)}: one is layout='chw' and the other 'hwc'")
    axis = -1 if _is_chw(a.shape) else -2
    if tuple(a.shape[-3:][:axis]) != tuple(b.shape[-3:][:axis]) or (axis == -2 and a.shape[-1] != b.shape[-1]):
        raise L.EgError(f"side_by_side: shapes {tuple(a.shape)} and {tuple(b.shape)}: the heights differ")
    if isinstance(a, torch.Tensor):
        return torch.cat([a, b.to(a.device) if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).to(a.device)], dim=axis)
    return np.concatenate([np.asarray(a), b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)], axis=axis)


def _rate(fps) -> Fraction:
    try:
        f = Fraction(*fps) if isinstance(fps, (tuple, list)) else Fraction(fps).limit_denominator(1001)
    except (TypeError, ValueError, ZeroDivisionError):
        f = Fraction(0)
    if f <= 0:
        raise L.EgError(f"write_y4m: fps={fps!r}: a positive number or (numerator, denominator)")
    return f


def write_y4m(path_or_file, frames, fps, n: Optional[int] = None, spec: Optional[PreviewSpec] = None) -> int:
    """One take as an uncompressed YUV4MPEG2 stream, which players and encoders read.  THE BYTES DO NOT SAY WHAT THEIR CHANNELS MEAN: pass
    ``spec=``, the PreviewSpec the frames were made with, and a wrong layout or colour space is refused by name; without it only the shape
    is checked, and an RGB ``"chw"`` rendering would be written as if it were Y, Cb, Cr.  ``frames`` ``uint8 [T, 3, H, W]`` holding Y, Cb, Cr
    -- a rendering made with ``layout="chw"`` and ``colorspace="ycbcr"`` -- at ``fps`` (a number or ``(numerator, denominator)``); ``n``: how
    many frames to write (default all T; the take's ``joint_frames``).  A device tensor is brought over in one copy.  Writes the stream
    header (``C444``, ``F<num>:<den>``) and per frame ``FRAME\\n`` and the three planes, from slices of the one host array.  ``path_or_file``: a
    path, or a binary file object such as an encoder's stdin (left open).  Returns the bytes written.

    Refused by name: ``frames`` that is not ``uint8 [T, 3, H, W]`` (an ``"hwc"`` rendering, several takes at once) and, with ``spec=`` the
    PreviewSpec the frames were made with, a layout other than ``"chw"``, a colour space other than ``"ycbcr"`` or another picture size: the
    bytes themselves do not say what their channels mean."""
    who = "write_y4m"
    if spec is not None:
        if spec.layout != "chw":
            raise L.EgError(f"{who}: layout={spec.layout!r}: a YUV4MPEG2 frame is three planes, render with layout='chw'")
        if spec.colorspace != "ycbcr":
            raise L.EgError(f"{who}: colorspace={spec.colorspace!r}: a YUV4MPEG2 stream holds Y, Cb, Cr, render with colorspace='ycbcr'")
    shape = tuple(frames.shape)
    if len(shape) != 4 or shape[1] != 3 or shape[3] == 3:
        raise L.EgError(f"{who}: frames shape {shape}: one take [T, 3, H, W], made with layout='chw' (an 'hwc' rendering is [T, H, W, 3]; "
                        "of several takes pass one)")
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8:
            raise L.EgError(f"{who}: frames dtype {frames.dtype}: uint8")
        arr = frames.detach().contiguous().cpu().numpy()                               # the one copy
    else:
        if np.asarray(frames).dtype != np.uint8:
            raise L.EgError(f"{who}: frames dtype {np.asarray(frames).dtype}: uint8")
        arr = np.ascontiguousarray(frames)
    T, _, H, W = shape
    if spec is not None and (H, W) != (spec.height, spec.width):
        raise L.EgError(f"{who}: frames of {H} x {W} pixels, the spec's are {spec.height} x {spec.width}")
    n = T if n is None else int(n)
    if not 0 <= n <= T:
        raise L.EgError(f"{who}: n={n} frames of a take of {T}")
    rate = _rate(fps)
    f = open(path_or_file, "wb") if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__") else path_or_file
    try:
        head = f"YUV4MPEG2 W{W} H{H} F{rate.numerator}:{rate.denominator} Ip A1:1 C444\n".encode("ascii")
        f.write(head)
        total = len(head)
        for t in range(n):
            f.write(b"FRAME\n")
            f.write(memoryview(arr[t]).cast("B"))                                      # Y, Cb, Cr planes: contiguous in [3, H, W]
            total += 6 + 3 * H * W
    finally:
        if f is not path_or_file:
            f.close()
    return total
