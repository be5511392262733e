"""Test-side restatement of the BVH text of whole takes (include/emogest.h, "BVH text of whole takes"; emotiongestures_amd.bvh.format_tracks) in
integer arithmetic: no ``%`` formatting, no float product.  A helper module, not a test.

``decimal6(v)``: the text of a float (fp32 values and float64 constants alike): the value as an exact ratio num / 2^k
(``float.as_integer_ratio``), N = num * 10^6 / 2^k rounded half to even in integers, the digits by ``divmod``.
``lines`` / ``body``: the MOTION lines of rows ``[rows, T, 3J]`` under a channel list, their lengths and the rows' offsets."""
import math

import numpy as np

TILE_FRAMES, MAX_CHANNELS, MAX_WIDTH = 8, 512, 18              # include/emogest.h: EG_BVH_TEXT_*

# a root with 6 channels, a joint with 3, one with 6, end sites, an OFFSET of -0.0, offsets that are no fp32 values
SMALL = """HIERARCHY
ROOT Hips
{
  OFFSET 0.25 91.5 -0.0
  CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation
  JOINT Spine
  {
    OFFSET 0.0 10.123456789 0.0
    CHANNELS 3 Zrotation Xrotation Yrotation
    JOINT Arm
    {
      OFFSET 12345.678 -3.0000004 1e-9
      CHANNELS 6 Xposition Yposition Zposition Yrotation Xrotation Zrotation
      End Site
      {
        OFFSET 0.0 5.0 0.0
      }
    }
  }
  JOINT Leg
  {
    OFFSET -8.0 0.0 0.0
    CHANNELS 3 Xrotation Yrotation Zrotation
    End Site
    {
      OFFSET 0.0 -40.0 0.0
    }
  }
}
"""


def special_values():
    """fp32: signed zeros, values that round to zero, the neighbours of 5e-7 on both sides, carries that change the width, the largest
    writable value."""
    half = np.float32(5e-7)
    near = [np.nextafter(half, np.float32(0)), half, np.nextafter(half, np.float32(1))]
    vals = [0.0, -0.0, 1e-9, -1e-9, 9.9999995, 999.9999995, -9.9999995, 99999.9999995, 0.0078125, -0.0078125, 2147483520.0, -2147483520.0,
            0.9999995, 1.0, 359.99997, -180.0, np.nextafter(np.float32(4), np.float32(0)), np.nextafter(np.float32(1), np.float32(0))]
    return np.array(vals + near + [-v for v in near], np.float32)


def writable(v) -> bool:
    v = float(v)
    return math.isfinite(v) and abs(v) < 2.0 ** 31


def _digits(n: int) -> str:
    out = []
    while True:
        n, d = divmod(n, 10)
        out.append("0123456789"[d])
        if n == 0:
            return "".join(reversed(out))


def decimal6(v) -> str:
    v = float(v)
    assert math.isfinite(v)
    num, den = abs(v).as_integer_ratio()                     # den is a power of two
    q, r = divmod(num * 10 ** 6, den)
    if 2 * r > den or (2 * r == den and q % 2 == 1):
        q += 1
    ip, fp = divmod(q, 10 ** 6)
    frac = _digits(fp)
    return ("-" if math.copysign(1.0, v) < 0 else "") + _digits(ip) + "." + "0" * (6 - len(frac)) + frac


def is_tie(v) -> bool:
    num, den = abs(float(v)).as_integer_ratio()
    return 2 * ((num * 10 ** 6) % den) == den


def line(sources, angles, root=None) -> str:
    """One MOTION line.  ``sources``: per channel ``("euler", k)``, ``("root", axis)`` or ``("const", float64)`` (BvhFile._channel_sources);
    ``angles [3J]`` and ``root [3]`` fp32."""
    return " ".join(decimal6(k if kind == "const" else (angles[k] if kind == "euler" else root[k])) for kind, k in sources) + "\n"


def body(sources, euler, per_row, root=None, draws=1):
    """``euler [rows, T, 3J]`` fp32, ``per_row`` valid frames, ``root [rows / draws, T, 3]`` fp32 or None -> (bytes of all rows back to
    back, offsets int64 [rows + 1], line_off int64 [rows * T + 1]: the start of every line, frames behind a row's last one empty)."""
    rows, T = euler.shape[:2]
    parts, line_off, at = [], np.zeros(rows * T + 1, np.int64), 0
    offsets = np.zeros(rows + 1, np.int64)
    for b in range(rows):
        offsets[b] = at
        for t in range(T):
            line_off[b * T + t] = at
            if t < per_row[b]:
                txt = line(sources, euler[b, t], None if root is None else root[b // draws, t]).encode("ascii")
                parts.append(txt)
                at += len(txt)
    offsets[rows] = line_off[rows * T] = at
    return b"".join(parts), offsets, line_off
