#!/usr/bin/env python3
"""The parity-plane walk of conv3x3_s2_planes_kernel (csrc/conv.hip), restated in numpy with the kernel's tables and index arithmetic, so that
the walk can be checked on a CPU (tests/test_conv_stride2_plane_walk.py): which input pixel every (plane, slot) of a workgroup's LDS tile
holds, which slot every (output pixel, tap) reads, and where every output pixel's pooling partial goes.

    python3 tools/conv_s2_plane_walk.py            # a few shapes, both tile heights
"""
import numpy as np

PW = 33                                         # ConvGeomS2P::PW
TAP_ORDER = (4, 3, 5, 1, 7, 0, 2, 6, 8)         # s2p_tap: the tap of a chunk's k-th step
STEP_PLANE = (0, 1, 1, 2, 2, 3, 3, 3, 3)        # s2p_plane: its plane = (row parity) * 2 + (column parity)
WAVE_GRID = {8: (4, 1), 4: (2, 2)}              # tile height -> (WM, WN) of the launch table


def cdiv(a, b):
    return -(-a // b)


def npix(TH):
    return (TH + 1) * PW                        # ConvGeomS2P::NPIX


def gap_tiles(H, W):
    """eg_conv3x3_gap_tiles for stride 2: the count of 2 x 32 output blocks."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return cdiv(Ho, 2) * cdiv(Wo, 32)


def stage_plane(H, W, TH, ty, tx, pl):
    """The plane image a workgroup stages: slot p -> input pixel id gy * W + gx, -1 = zero (outside the plane or the image).  The kernel's roles:
    pr = p / PW, pc = p % PW, (gy0, gx0) = (2 (oy0 + pr), 2 (ox0 + pc)), plane (rp, cp) reads (gy0 - rp, gx0 - cp), masked by pmask."""
    oy0, ox0 = ty * TH, tx * 32
    rp, cp = pl >> 1, pl & 1
    img = np.full(npix(TH), -1, dtype=np.int64)
    for p in range(npix(TH)):
        pr, pc = divmod(p, PW)
        gy, gx = 2 * (oy0 + pr) - rp, 2 * (ox0 + pc) - cp
        if pr < TH + rp and pc < 32 + cp and 0 <= gy < H and 0 <= gx < W:
            img[p] = gy * W + gx
    return img


def tap_slot(TH, wm, t, li, tap):
    """The slot lane li of pixel tile t of wave row wm reads for `tap` (read_x: pbase + toff), and the tile-local output pixel it belongs to."""
    r, c = 2 * wm + (t >> 1), (t & 1) * 16 + li
    kh, kw = divmod(tap, 3)
    return (r + (kh == 2)) * PW + c + (kw == 2), (r, c)


def partial_index(H, W, TH, ty, wm, tx):
    """The pooling partial a wave row writes (gbase of the epilogue), None where its block lies below the map."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if ty * TH + 2 * wm >= Ho:
        return None
    return (ty * (TH // 2) + wm) * cdiv(Wo, 32) + tx


def walk(H, W, TH):
    """Every (workgroup, output pixel, tap) of one map: yields (oy, ox, tap, input pixel id or -1, partial index)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    WM = WAVE_GRID[TH][0]
    for ty in range(cdiv(Ho, TH)):
        for tx in range(cdiv(Wo, 32)):
            planes = [stage_plane(H, W, TH, ty, tx, pl) for pl in range(4)]
            for k, tap in enumerate(TAP_ORDER):
                img = planes[STEP_PLANE[k]]
                for wm in range(WM):
                    part = partial_index(H, W, TH, ty, wm, tx)
                    for t in range(4):
                        for li in range(16):
                            slot, (r, c) = tap_slot(TH, wm, t, li, tap)
                            oy, ox = ty * TH + r, tx * 32 + c
                            if oy < Ho and ox < Wo:             # pixo >= 0: the pixel is stored and pooled
                                yield oy, ox, tap, int(img[slot]), part


if __name__ == "__main__":
    for H, W in ((5, 7), (17, 65), (64, 66)):
        for TH in (4, 8):
            n = bad = 0
            for oy, ox, tap, src, part in walk(H, W, TH):
                kh, kw = divmod(tap, 3)
                gy, gx = 2 * oy + kh - 1, 2 * ox + kw - 1
                want = gy * W + gx if 0 <= gy < H and 0 <= gx < W else -1
                n += 1
                bad += src != want
            print(f"H={H} W={W} TH={TH}: {n} (pixel, tap) reads, {bad} wrong")
