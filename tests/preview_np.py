"""The picture of a preview frame restated in numpy float32, one frame and one bone at a time, from the formula of include/emogest.h
("Preview frames") and not from emotiongestures_amd.preview's host path.  Every + - * is one float32 operation in the order written (numpy
never fuses a multiply-add), np.sqrt and the division are correctly rounded, and a comparison with a NaN is false.  Also here: the BT.601
integer conversion and the coverage statistics the GPU cases are chosen by (the cases themselves: tests/preview_cases.py)."""
import numpy as np

F = np.float32
CYCLE = [(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127),
         (188, 189, 34), (23, 190, 207)]


def ycbcr(rgb):
    r, g, b = (int(v) for v in rgb)
    return (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128,
            ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128)


def coverage(ua, va, ub, vb, H, W, radius):
    """q [H, W] int64 of one bone from (ua, va) to (ub, vb), float32 scalars."""
    X = (np.arange(W, dtype=F) + F(0.5))[None, :]
    Y = (np.arange(H, dtype=F) + F(0.5))[:, None]
    with np.errstate(all="ignore"):
        ax, ay = F(ua), F(va)
        ex = F(ub) - ax
        ey = F(vb) - ay
        l2 = F(F(ex * ex) + F(ey * ey))
        inv = F(1) / l2 if l2 > 0 else F(0)
        wx = X - ax
        wy = Y - ay
        s = (wx * ex + wy * ey) * inv
        t = np.where(s < 0, F(0), s)                  # a NaN stays: both comparisons are false
        t = np.where(t > 1, F(1), t)
        dx = wx - t * ex
        dy = wy - t * ey
        a = (F(radius) + F(0.5)) - np.sqrt(dx * dx + dy * dy)
        assert a.dtype == F
        q = np.zeros((H, W), np.int64)
        full, part = a >= 1, (a > 0) & ~(a >= 1)
        q[full] = 255
        q[part] = (a[part] * F(255) + F(0.5)).astype(np.int64)
    return q


def frame(p, bones, camera, H, W, radius, colours, background, skip=()):
    """One frame: p [J, 3] float32, camera = (matrix [2, 3], centre [2]) float32 -> (picture [H, W, 3] uint8, q of every bone).  `skip`:
    bones left out (for the statistics of a case without one bone)."""
    m, c = np.asarray(camera[0], F), np.asarray(camera[1], F)
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        u = ((m[0, 0] * p[:, 0] + m[0, 1] * p[:, 1]) + m[0, 2] * p[:, 2]) + c[0]
        v = ((m[1, 0] * p[:, 0] + m[1, 1] * p[:, 1]) + m[1, 2] * p[:, 2]) + c[1]
    assert u.dtype == F and v.dtype == F
    img = np.empty((H, W, 3), np.int64)
    img[:] = np.asarray(background, np.int64)
    qs = []
    for k, (ja, jb) in enumerate(bones):
        if k in skip:
            continue
        q = coverage(u[ja], v[ja], u[jb], v[jb], H, W, radius)
        qs.append(q)
        for ch in range(3):
            img[:, :, ch] = (img[:, :, ch] * (255 - q) + int(colours[k][ch]) * q + 127) // 255
    return img.astype(np.uint8), qs


def render(joints, frames, bones, camera, H, W, radius, colours, background, layout="hwc"):
    """joints [B, T, J, 3], frames [B] valid frames per row -> uint8 [B, T, H, W, 3] or [B, T, 3, H, W]; zeros behind a row's frames."""
    B, T = joints.shape[:2]
    out = np.zeros((B, T, H, W, 3), np.uint8)
    for b in range(B):
        for t in range(int(frames[b])):
            out[b, t] = frame(joints[b, t], bones, camera, H, W, radius, colours, background)[0]
    return out if layout == "hwc" else np.ascontiguousarray(out.transpose(0, 1, 4, 2, 3))


def not_blank(joints, frames, bones, camera, H, W, radius, skip=()):
    """The condition that keeps a case from passing on blank pictures, asserted on this restatement: every valid frame shows at least 2 % of
    its pixels touched by a bone (q > 0; `skip`: without those bones) and at least one pixel with 0 < q < 255.  Returns the smallest share."""
    least = 1.0
    white, black = [(0, 0, 0)] * len(bones), (255, 255, 255)
    for b in range(joints.shape[0]):
        for t in range(int(frames[b])):
            _img, qs = frame(joints[b, t], bones, camera, H, W, radius, white, black, skip)
            hit = np.maximum.reduce(qs) if qs else np.zeros((H, W), np.int64)
            share = float((hit > 0).mean())
            assert share >= 0.02, (b, t, share)
            assert any(((q > 0) & (q < 255)).any() for q in qs), (b, t)
            least = min(least, share)
    return least
