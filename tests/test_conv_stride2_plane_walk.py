"""The parity-plane walk of the stride-2 stage-entry convolutions (csrc/conv.hip: conv3x3_s2_planes_kernel), checked without a GPU:
tools/conv_s2_plane_walk.py restates the kernel's plane / tap / offset tables and its staging and read index arithmetic in numpy.  This checks
the walk as restated there, not the kernel: what binds the kernel to it is tests/test_gpu_conv_stride2_planes.py, element by element against
float64."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_s2_plane_walk", os.path.join(ROOT, "tools", "conv_s2_plane_walk.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)

HS = (5, 7, 16, 17, 64, 65, 66)
WS = (5, 7, 33, 62, 65, 66)


def test_tap_order_is_a_permutation_grouped_by_plane():
    assert sorted(P.TAP_ORDER) == list(range(9))
    # a tap (kh, kw) reads input (2 oy + kh - 1, 2 ox + kw - 1): odd rows for kh != 1, odd columns for kw != 1
    for k, tap in enumerate(P.TAP_ORDER):
        kh, kw = divmod(tap, 3)
        assert P.STEP_PLANE[k] == (kh != 1) * 2 + (kw != 1)
    assert list(P.STEP_PLANE) == sorted(P.STEP_PLANE)           # one plane after the other: the tile holds one plane at a time
    assert P.STEP_PLANE[-4:] == (3, 3, 3, 3)                    # the four-tap plane is a chunk's last


@pytest.mark.parametrize("TH", [4, 8])
@pytest.mark.parametrize("H", HS)
def test_every_tap_reads_its_input_pixel_or_padding(H, TH):
    for W in WS:
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        seen = np.zeros((Ho, Wo, 9), dtype=np.int64)
        tiles = P.gap_tiles(H, W)
        for oy, ox, tap, src, part in P.walk(H, W, TH):
            kh, kw = divmod(tap, 3)
            gy, gx = 2 * oy + kh - 1, 2 * ox + kw - 1
            want = gy * W + gx if 0 <= gy < H and 0 <= gx < W else -1
            assert src == want, (H, W, TH, oy, ox, tap)
            seen[oy, ox, tap] += 1
            # the partial of the pixel's 2 x 32 block in the numbering of eg_conv3x3_gap_tiles
            assert part == (oy // 2) * P.cdiv(Wo, 32) + ox // 32 and 0 <= part < tiles, (H, W, TH, oy, ox)
        assert (seen == 1).all(), (H, W, TH)                    # every output pixel takes every tap exactly once


@pytest.mark.parametrize("TH", [4, 8])
@pytest.mark.parametrize("H", HS)
def test_every_halo_pixel_is_in_exactly_one_plane(H, TH):
    for W in WS:
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        for ty in range(P.cdiv(Ho, TH)):
            for tx in range(P.cdiv(Wo, 32)):
                count = np.zeros(H * W, dtype=np.int64)
                for pl in range(4):
                    img = P.stage_plane(H, W, TH, ty, tx, pl)
                    assert img.shape == (P.npix(TH),)
                    ids = img[img >= 0]
                    assert len(np.unique(ids)) == len(ids)
                    gy, gx = ids // W, ids % W
                    assert ((gy & 1) == (pl >> 1)).all() and ((gx & 1) == (pl & 1)).all()
                    count[ids] += 1
                # the halo of a TH x 32 output tile: input rows 2 oy0 - 1 .. 2 (oy0 + TH) - 1, columns 2 ox0 - 1 .. 2 (ox0 + 32) - 1, clipped to the image
                halo = np.zeros((H, W), dtype=np.int64)
                halo[max(2 * ty * TH - 1, 0):2 * (ty * TH + TH), max(2 * tx * 32 - 1, 0):2 * (tx * 32 + 32)] = 1
                assert (count == halo.ravel()).all(), (H, W, TH, ty, tx)
