"""Preview frames without a GPU (emotiongestures_amd/preview.py): the numpy path against the restatement tests/preview_np.py byte for byte, the
three symbols of the header, every refusal before a launch, the YUV4MPEG2 writer, the orbit camera and the BT.601 conversion."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import preview_cases as PC
import preview_np as PN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import preview as PV
from emotiongestures_amd import skeleton as SK


@pytest.mark.parametrize("name", PC.NAMES)
def test_numpy_path_equals_the_restatement_byte_for_byte(name):
    joints, frames, spec, want = PC.case(name)
    got = PV.render_joints(joints, spec, frames)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    if frames is not None:                                                               # zeros behind a recording's frames
        for u, n in enumerate(frames):
            assert not got[u, :, n:].any() and got[u, :, :n].any()
    t = PV.render_joints(torch.from_numpy(joints), spec, frames)                         # a CPU tensor in: a CPU tensor out
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and np.array_equal(t.numpy(), want)


def test_later_bones_paint_over_earlier_ones_and_a_dict_is_a_spec():
    body = SK.JointTree([-1, 0, 1], np.zeros((3, 3)))
    j = np.array([[(2.0, 8.0, 0), (14.0, 8.0, 0), (8.0, 8.0, 0)]], np.float32)            # bone 1 lies on the right half of bone 0
    pal = np.array([(255, 0, 0), (0, 0, 255)], np.uint8)
    img = PV.render_joints(j, dict(body=body, height=16, width=16, camera=PC.flat_camera(1.0, 0.0, 0.0), radius=1.0, palette=pal))[0]
    assert tuple(img[8, 4]) == (255, 0, 0) and tuple(img[8, 11]) == (0, 0, 255) and tuple(img[2, 2]) == (255, 255, 255)


def test_the_header_symbols_are_exported_and_agree_with_python():
    lib = L.load()
    for name in ("eg_preview_raster", "eg_preview_check", "eg_preview_max_bones"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.eg_preview_max_bones() == L.EG_PREVIEW_MAX_BONES == PV.MAX_BONES == 64
    spec = PC.case("chain")[2]
    w = spec.words()
    assert len(w) == L.EG_PREVIEW_TABLE_WORDS and w[0] == 4 and w[1] == 5 and w[2] == 0xFFFFFF
    assert list(w[4:9]) == [0, 1, 2, 3, 4] and w[4 + 128] == 0 and w[4 + 192] == 1 and w[4 + 256] == 31 | 119 << 8 | 180 << 16


def _raster(lib, bones, J=5, H=16, W=16, radius=1.5, layout=0, rows=1, T=1, draws=1, unit=1, camera=None, joints=16, out=16, table=16, d_frames=None):
    """eg_preview_raster with addresses that are never dereferenced on the device side: every refusal returns before the launch."""
    b = np.ascontiguousarray(bones, np.int32)
    cam = np.ascontiguousarray([1, 0, 0, 0, 1, 0, 0, 0] if camera is None else camera, np.float32)
    P = lambda v: None if v is None else C.c_void_p(v)
    rc = lib.eg_preview_raster(P(joints), rows, T, J, b.ctypes.data_as(C.c_void_p), len(b), P(table), cam.ctypes.data_as(C.c_void_p), radius, H, W,
                               layout, draws, unit, P(d_frames), P(out), None)
    return rc, lib.eg_last_error().decode()


def test_the_c_entry_point_refuses_by_name_before_the_launch():
    lib = L.load()
    ok = [(0, 1), (1, 2)]
    for kw, word in ((dict(H=7), "height=7"), (dict(W=2049), "width=2049"), (dict(radius=0.2), "radius=0.2"), (dict(radius=16.5), "radius=16.5"),
                     (dict(radius=float("nan")), "radius="), (dict(layout=2), "layout=2"), (dict(rows=3, draws=2), "multiple of draws"),
                     (dict(unit=0), "frame_unit=0"), (dict(d_frames=18), "d_frames not 4-byte aligned"), (dict(joints=20), "not 16-byte aligned"),
                     (dict(out=8), "not 16-byte aligned"), (dict(table=4), "not 16-byte aligned"), (dict(joints=None), "null joints"),
                     (dict(out=None), "null out"), (dict(T=0), "frames=0"), (dict(camera=[1, 0, 0, 0, np.inf, 0, 0, 0]), "camera[4]")):
        rc, msg = _raster(lib, ok, **kw)
        assert rc < 0 and word in msg, (kw, rc, msg)
    rc, msg = _raster(lib, [(0, 5)])
    assert rc < 0 and "bone 0 names joint 5 of J=5" in msg
    rc, msg = _raster(lib, [(0, 1), (-1, 2)])
    assert rc < 0 and "bone 1 names joint -1" in msg
    rc, msg = _raster(lib, [(0, 1)] * 65)
    assert rc < 0 and "bones=65" in msg and "64" in msg
    bones = np.array([(0, 1), (1, 4)], np.int32)
    assert lib.eg_preview_check(bones.ctypes.data_as(C.c_void_p), 2, 5) == 0
    assert lib.eg_preview_check(bones.ctypes.data_as(C.c_void_p), 2, 4) < 0 and b"joint 4 of J=4" in lib.eg_last_error()
    assert lib.eg_preview_check(None, 2, 4) < 0 and lib.eg_preview_check(bones.ctypes.data_as(C.c_void_p), 0, 4) < 0


def test_python_refuses_by_name():
    sk = SK.ted_expressive()
    for kw, word in ((dict(height=7), "height=7"), (dict(width=2049), "width=2049"), (dict(height=16.0), "height=16.0"), (dict(radius=0.1), "radius=0.1"),
                     (dict(radius=17), "radius=17"), (dict(radius=float("nan")), "radius=nan"), (dict(layout="nhwc"), "layout='nhwc'"),
                     (dict(colorspace="yuv"), "colorspace='yuv'"), (dict(bones=[(0, 43)]), "joint 43 of J=43"), (dict(bones=[(0, 1)] * 65), "65 bones"),
                     (dict(bones=[]), "0 bones"), (dict(palette=np.zeros((3, 3), np.uint8)), "palette shape (3, 3)"),
                     (dict(background=(0, 0, 256)), "background="), (dict(camera=np.eye(3)), "camera=")):
        with pytest.raises(L.EgError, match=word.replace("(", r"\(").replace(")", r"\)")):
            PV.PreviewSpec(**dict(dict(body=sk, height=16, width=16), **kw))
    with pytest.raises(L.EgError, match="body= takes"):
        PV.PreviewSpec([1, 2], 16, 16)
    with pytest.raises(L.EgError, match="need \\[2, 3\\]"):
        PV.Camera(np.eye(3), [0, 0])
    with pytest.raises(L.EgError, match="up='w'"):
        PV.Camera.orbit(height=16, width=16, up="w")
    with pytest.raises(L.EgError, match="elev=90"):
        PV.Camera.orbit(elev=90, height=16, width=16)
    spec = PV.PreviewSpec(sk, 16, 16)
    j = np.zeros((2, 3, 43, 3), np.float32)
    with pytest.raises(L.EgError, match="frames has 3 entries for 2 recordings"):
        PV.render_joints(j, spec, [1, 2, 3])
    with pytest.raises(L.EgError, match=r"every value must be in \[0, 3\]"):
        PV.render_joints(j, spec, [1, 4])
    with pytest.raises(L.EgError, match="joint 42 of J=42"):                              # J against the largest joint the bones name
        PV.render_joints(j[:, :, :42], spec)
    with pytest.raises(L.EgError, match="need \\[..., T >= 1, J >= 1, 3\\]"):
        PV.render_joints(j[..., :2], spec)
    with pytest.raises(L.EgError, match="at most two leading axes"):
        PV.render_joints(j[None, None], spec)
    small = PV.PreviewSpec(sk, 16, 16, max_bytes=2 * 3 * 16 * 16 * 3 - 1)
    with pytest.raises(L.EgError, match="4608 bytes.*max_bytes=4607.*fewer takes per call or a smaller picture"):
        PV.render_joints(j, small)
    assert PV.render_joints(j, PV.PreviewSpec(sk, 16, 16, max_bytes=4608)).shape == (2, 3, 16, 16, 3)


def _parse_y4m(data):
    head, _, rest = data.partition(b"\n")
    fields = head.decode("ascii").split(" ")
    assert fields[0] == "YUV4MPEG2"
    tags = {f[0]: f[1:] for f in fields[1:]}
    W, H = int(tags["W"]), int(tags["H"])
    frames = []
    while rest:
        assert rest[:6] == b"FRAME\n"
        frames.append(np.frombuffer(rest[6:6 + 3 * H * W], np.uint8).reshape(3, H, W))
        rest = rest[6 + 3 * H * W:]
    return tags, frames


def test_write_y4m_round_trips(tmp_path):
    joints, frames, spec, want = PC.case("ted-chw-ycbcr")
    take = PV.render_joints(joints, spec, frames)[1, 0]                                  # [7, 3, 48, 64], 4 valid frames
    buf = io.BytesIO()
    n = PV.write_y4m(buf, take, 15, n=frames[1], spec=spec)
    data = buf.getvalue()
    assert n == len(data) and not buf.closed
    tags, got = _parse_y4m(data)
    assert (tags["W"], tags["H"], tags["F"], tags["C"], tags["I"], tags["A"]) == ("64", "48", "15:1", "444", "p", "1:1")
    assert len(got) == 4 and all(np.array_equal(g, want[1, 0, t]) for t, g in enumerate(got))
    path = tmp_path / "take.y4m"
    assert PV.write_y4m(path, torch.from_numpy(take), (30000, 1001)) == path.stat().st_size
    tags, got = _parse_y4m(path.read_bytes())
    assert tags["F"] == "30000:1001" and len(got) == 7 and np.array_equal(np.stack(got), take)
    assert _parse_y4m_rate(take, 29.97) == "2997:100" and _parse_y4m_rate(take, 12.5) == "25:2"
    # the background of a Y, Cb, Cr rendering is white in BT.601: (235, 128, 128)
    assert tuple(take[0, :, 0, 0]) == (235, 128, 128)


def _parse_y4m_rate(take, fps):
    buf = io.BytesIO()
    PV.write_y4m(buf, take, fps, n=0)
    return _parse_y4m(buf.getvalue())[0]["F"]


def test_write_y4m_and_side_by_side_refuse_by_name():
    sk = SK.ted_expressive()
    chw = np.zeros((2, 3, 16, 24), np.uint8)
    for kw, word in ((dict(layout="hwc", colorspace="ycbcr"), "layout='hwc'"), (dict(layout="chw", colorspace="rgb"), "colorspace='rgb'")):
        with pytest.raises(L.EgError, match=word):
            PV.write_y4m(io.BytesIO(), chw, 15, spec=PV.PreviewSpec(sk, 16, 24, **kw))
    good = PV.PreviewSpec(sk, 16, 24, layout="chw", colorspace="ycbcr")
    with pytest.raises(L.EgError, match="made with layout='chw'"):
        PV.write_y4m(io.BytesIO(), np.zeros((2, 16, 24, 3), np.uint8), 15)
    with pytest.raises(L.EgError, match="of several takes pass one"):
        PV.write_y4m(io.BytesIO(), chw[None], 15, spec=good)
    with pytest.raises(L.EgError, match="dtype float32"):
        PV.write_y4m(io.BytesIO(), chw.astype(np.float32), 15, spec=good)
    with pytest.raises(L.EgError, match="16 x 24 pixels, the spec's are 16 x 32"):
        PV.write_y4m(io.BytesIO(), chw, 15, spec=PV.PreviewSpec(sk, 16, 32, layout="chw", colorspace="ycbcr"))
    with pytest.raises(L.EgError, match="n=3 frames of a take of 2"):
        PV.write_y4m(io.BytesIO(), chw, 15, n=3, spec=good)
    with pytest.raises(L.EgError, match="fps=0"):
        PV.write_y4m(io.BytesIO(), chw, 0, spec=good)
    a, b = np.full((2, 3, 16, 24), 1, np.uint8), np.full((2, 3, 16, 8), 2, np.uint8)
    both = PV.side_by_side(a, b)
    assert both.shape == (2, 3, 16, 32) and (both[..., :24] == 1).all() and (both[..., 24:] == 2).all()
    hw = PV.side_by_side(torch.zeros(4, 2, 16, 24, 3, dtype=torch.uint8), torch.ones(4, 2, 16, 24, 3, dtype=torch.uint8))
    assert tuple(hw.shape) == (4, 2, 16, 48, 3) and not hw[..., :24, :].any() and hw[..., 24:, :].all()
    with pytest.raises(L.EgError, match="one is layout='chw' and the other 'hwc'"):
        PV.side_by_side(a, np.zeros((2, 16, 24, 3), np.uint8))
    with pytest.raises(L.EgError, match="the heights differ"):
        PV.side_by_side(a, np.zeros((2, 3, 17, 24), np.uint8))


@pytest.mark.parametrize("up", ["-y", "z", "x"])
def test_orbit_rows_are_orthogonal_and_of_length_width_over_span(up):
    for azim, elev, span, W in ((-60, 20, 1.0, 64), (35, -40, 2.5, 320), (180, 0, 0.7, 50)):
        cam = PV.Camera.orbit(azim, elev, span, height=48, width=W, target=(0.1, -0.2, 0.3), up=up)
        m = cam.matrix.astype(np.float64)
        s = W / span
        assert cam.matrix.dtype == np.float32 and cam.centre.dtype == np.float32
        assert abs(np.linalg.norm(m[0]) / s - 1) < 1e-6 and abs(np.linalg.norm(m[1]) / s - 1) < 1e-6 and abs(m[0] @ m[1]) / (s * s) < 1e-6
        assert np.allclose(m @ np.array([0.1, -0.2, 0.3]) + cam.centre, (W / 2, 24), atol=1e-3)      # the target is the middle of the picture
        axis = np.eye(3)["xyz".index(up[-1])] * (-1 if up[0] == "-" else 1)
        assert (m @ axis)[1] < 0 and abs((m @ axis)[0]) < 1e-4 * s                        # up is up: image y runs downwards
    assert np.array_equal(PV.PreviewSpec(SK.ted_expressive(), 48, 64).camera.matrix, PV.Camera.orbit(-60, 20, 1.0, height=48, width=64).matrix)


def test_bt601_limited_range_of_black_white_and_the_primaries():
    rgb = np.array([(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)], np.uint8)
    want = [(16, 128, 128), (235, 128, 128), (82, 90, 240), (144, 54, 34), (41, 240, 110)]
    assert PV.rgb_to_ycbcr(rgb).tolist() == [list(w) for w in want] and PV.rgb_to_ycbcr(rgb).dtype == np.uint8
    assert [PN.ycbcr(c) for c in rgb.tolist()] == want
    spec = PV.PreviewSpec(SK.ted_expressive(), 16, 16, colorspace="ycbcr")
    assert spec.ground.tolist() == [235, 128, 128] and spec.colours[0].tolist() == list(PN.ycbcr(PN.CYCLE[0]))
    assert PV.PALETTE.tolist() == [list(c) for c in PN.CYCLE]
