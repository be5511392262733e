"""Euler channels, the Euler filter and BVH in and out, without a GPU: the float64 definitions of emotiongestures_amd.skeleton against scipy and
numpy, the restatement tests/euler_np.py against both, the BVH parser and writer on a hand-written text, and an independent BVH forward
kinematics against joints_from_rot6d."""
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import articulate_np as AN
import euler_np as EN
from conftest import ROOT
from emotiongestures_amd import _lib as L
from emotiongestures_amd import bvh as BVH
from emotiongestures_amd import skeleton as S

NEW_SYMBOLS = ("eg_articulate_euler", "eg_articulate_rot6d_euler", "eg_angle_unwrap_workspace_bytes", "eg_angle_unwrap")


def _mod360(d):
    return (np.asarray(d) + 180.0) % 360.0 - 180.0


def _tree(J):
    return S.JointTree([-1] + list(range(J - 1)), np.zeros((J, 3)))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header, re.S)
        assert decl, name
        assert name in L.SIGNATURES and getattr(lib, name) is not None
        assert len(decl.group(1).split(",")) == len(L.SIGNATURES[name][1]), name
    assert re.search(r"#define EG_UNWRAP_TILE_FRAMES %d\b" % S.UNWRAP_TILE_FRAMES, header)


def test_host_checks_refuse_by_name():
    import ctypes as C
    lib = L.load()
    p = C.c_void_p(256)
    good = (C.c_int32 * 2)(0, 5)
    bad = (C.c_int32 * 2)(0, 6)
    assert lib.eg_articulate_euler(p, 1, 4, 2, bad, p, None, 1, 1, None, 0, 1, 1, 1, p, 4, None) != 0
    assert "order code 6" in lib.eg_last_error().decode()
    assert lib.eg_articulate_euler(p, 1, 4, 65, good, p, None, 1, 1, None, 0, 1, 1, 1, p, 4, None) != 0
    assert "joints=65" in lib.eg_last_error().decode()
    assert lib.eg_articulate_rot6d_euler(p, 1, 4, 2, bad, p, None, 1, 1, None, 0, 1, p, None) != 0
    assert "order code 6" in lib.eg_last_error().decode()
    assert lib.eg_articulate_rot6d_euler(p, 1, 4, 0, good, p, None, 1, 1, None, 0, 1, p, None) != 0
    assert "joints=0" in lib.eg_last_error().decode()
    for period in (float("nan"), float("inf"), 0.0, -360.0, 1e300):
        assert lib.eg_angle_unwrap(p, 1, 4, 3, None, 1, 1, period, None, 0, None) != 0
        assert "period=" in lib.eg_last_error().decode()
    assert lib.eg_angle_unwrap(p, 1, 1000, 3, None, 1, 1, 360.0, None, 0, None) != 0 and "null workspace" in lib.eg_last_error().decode()
    assert lib.eg_angle_unwrap(p, 1, 1000, 3, None, 1, 1, 360.0, p, 8, None) != 0 and "workspace too small" in lib.eg_last_error().decode()
    assert lib.eg_angle_unwrap_workspace_bytes(0, 4, 3) == 0 and lib.eg_angle_unwrap_workspace_bytes(2, 1000, 3) >= 2 * 16 * 3 * 8


# ---- the definitions ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_rotations():
    R = Rot.random(6 * 4000, random_state=11).as_matrix().reshape(4000, 6, 3, 3)
    return R, R[..., :2, :].reshape(4000, 36)


def test_float64_definition_against_scipy(random_rotations):
    R, x = random_rotations
    tree = _tree(6)
    for fn in (lambda: S.euler_from_rot6d(x, tree, list(S.ORDERS)), lambda: EN.euler(x[None], list(range(6)))[0]):
        e = fn()
        for j, o in enumerate(S.ORDERS):
            i, _j, k, eps = EN.axes(j)
            keep = 1.0 - np.abs(R[:, j, i, k]) >= 2.0 ** -19
            assert keep.mean() > 0.99
            ref = Rot.from_matrix(R[keep, j]).as_euler(o, degrees=True)          # uppercase: intrinsic
            assert np.abs(_mod360(e[keep, j] - ref)).max() < 1e-11, o
    rad = S.euler_from_rot6d(x, tree, "ZXY", degrees=False)
    assert np.abs(np.degrees(rad) - S.euler_from_rot6d(x, tree, "ZXY")).max() < 1e-12
    assert np.abs(rad[..., 1]).max() <= np.pi / 2


def test_euler_matrix_euler_identity_and_inverse(random_rotations):
    R, x = random_rotations
    tree = _tree(6)
    e = S.euler_from_rot6d(x, tree, list(S.ORDERS))
    back = S.rot6d_from_euler(e, tree, list(S.ORDERS))
    assert np.abs(back - x).max() < 1e-12                                        # rot6d_from_euler o euler_from_rot6d on orthonormal input
    assert np.abs(_mod360(S.euler_from_rot6d(back, tree, list(S.ORDERS)) - e)).max() < 1e-8
    assert np.abs(EN.matrices_of_euler(e, list(range(6))) - R.reshape(4000, 6, 9)).max() < 1e-12
    assert np.abs(EN.matrices_of_euler_product(e, list(range(6))) - R.reshape(4000, 6, 9)).max() < 1e-12
    assert np.abs(EN.rot6d(e[None], list(range(6)))[0] - x).max() < 1e-12
    mean = np.linspace(-0.3, 0.3, 36)
    tc = S.JointTree([-1] + list(range(5)), np.zeros((6, 3)), basis="columns")
    xc = np.swapaxes(R, -1, -2)[..., :2, :].reshape(4000, 36) - mean
    ec = S.euler_from_rot6d(xc, tc, list(S.ORDERS), mean=mean)
    assert np.abs(_mod360(ec - e)).max() < 1e-9
    assert np.abs(S.rot6d_from_euler(ec, tc, list(S.ORDERS), mean=mean) - xc).max() < 1e-12
    t = torch_cpu(x)
    assert isinstance(S.euler_from_rot6d(t, tree, "XYZ"), type(t)) and S.euler_from_rot6d(t, tree, "XYZ").dtype == t.dtype


def torch_cpu(x):
    import torch
    return torch.from_numpy(np.asarray(x, np.float64))


def test_lock_branch_rebuilds_the_matrix():
    for code, o in enumerate(S.ORDERS):
        for sign in (1.0, -1.0):
            e = np.array([[[37.0, sign * 90.0, 0.0]]])
            R = EN.matrices_of_euler_product(e, [code]).reshape(1, 1, 3, 3)
            tree = _tree(1)
            got = S.euler_from_rot6d(R[..., :2, :].reshape(1, 6), tree, o)
            assert got[0, 0, 2] == 0.0 and abs(got[0, 0, 1] - sign * 90.0) < 1e-6
            assert np.abs(EN.matrices_of_euler_product(got[None], [code]).reshape(3, 3) - R[0, 0]).max() < 1e-9


def test_frames_fps_and_shapes():
    tr = AN.rotation_tracks(5, 12, 2, B=3).astype(np.float64)
    tree = S.JointTree(*AN.chain(5))
    e, n = S.euler_from_rot6d(tr, tree, "ZXY", frames=[12, 7, 1], fps=(2, 3))
    assert e.shape == (3, 18, 5, 3) and n == [18, 11, 2]
    assert np.all(e[1, 11:] == 0) and np.all(e[2, 2:] == 0)
    ref = EN.euler(tr, [4] * 5, frames=[12, 7, 1], L=3, M=2)
    assert np.abs(e - ref).max() < 1e-11
    e2 = S.euler_from_rot6d(np.stack([tr, tr], 1), tree, "ZXY", frames=[12, 7, 1])[0]
    assert e2.shape == (3, 2, 12, 5, 3) and np.array_equal(e2[:, 0], e2[:, 1])
    with pytest.raises(L.EgError, match="repeats an axis"):
        S.euler_from_rot6d(tr, tree, "ZXZ")
    with pytest.raises(L.EgError, match="need one of"):
        S.euler_from_rot6d(tr, tree, "ABC")
    with pytest.raises(L.EgError, match="2 orders for 5 joints"):
        S.euler_from_rot6d(tr, tree, ["XYZ", "ZXY"])
    with pytest.raises(L.EgError, match="period="):
        S.unwrap_angles(np.zeros((4, 3)), period=float("nan"))


def test_unwrap_against_numpy():
    rng = np.random.default_rng(5)
    walk = np.cumsum(rng.uniform(-170.0, 170.0, (3, 400, 7)), axis=1)            # steps below half a period: tie-free
    wrapped = _mod360(walk)
    ref = np.degrees(np.unwrap(np.radians(wrapped), axis=1))
    assert np.abs(S.unwrap_angles(wrapped) - ref).max() < 1e-10
    assert np.abs(EN.unwrap(wrapped, dtype=np.float64) - ref).max() < 1e-10
    rad = np.radians(wrapped)
    assert np.abs(S.unwrap_angles(rad, period=2 * np.pi) - np.unwrap(rad, axis=1)).max() < 1e-12
    got = S.unwrap_angles(wrapped, frames=[400, 100, 1])
    assert np.array_equal(got[1, 100:], wrapped[1, 100:]) and np.array_equal(got[2], wrapped[2])
    assert np.abs(got[1, :100] - ref[1, :100]).max() < 1e-10
    w32 = wrapped.astype(np.float32)
    r32 = EN.unwrap(w32)
    assert r32.dtype == np.float32 and np.abs(r32 - ref).max() < 2e-3 * np.abs(ref).max() / 360 + 1e-3
    tr = AN.rotation_tracks(4, 300, 9).astype(np.float64)
    tree = S.JointTree(*AN.chain(4))
    e = S.euler_from_rot6d(tr, tree, "YXZ")[0]
    u = S.euler_from_rot6d(tr, tree, "YXZ", unwrap=True)[0]
    assert np.array_equal(u, S.unwrap_angles(e.reshape(300, 12)).reshape(300, 4, 3))
    assert np.abs(_mod360(u - e)).max() < 1e-9 and np.abs(np.diff(u, axis=0)).max() <= 180.0


# ---- BVH ------------------------------------------------------------------------------------------------------------------------------------------
HIERARCHY = """HIERARCHY
ROOT Hips
{
\tOFFSET 0.000000 92.500000 1.250000
\tCHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation
\tJOINT Spine
\t{
\t\tOFFSET 0.0 10.5 -0.75
\t\tCHANNELS 3 Zrotation Xrotation Yrotation
\t\tJOINT Chest
\t\t{
\t\t\tOFFSET 0.25 12.0 0.5
\t\t\tCHANNELS 3 Xrotation Yrotation Zrotation
\t\t\tJOINT Neck
\t\t\t{
\t\t\t\tOFFSET 0.0 15.25 1.0
\t\t\t\tCHANNELS 3 Yrotation Xrotation Zrotation
\t\t\t\tJOINT Head
\t\t\t\t{
\t\t\t\t\tOFFSET 0.0 8.0 1.5
\t\t\t\t\tCHANNELS 3 Zrotation Yrotation Xrotation
\t\t\t\t\tEnd Site
\t\t\t\t\t{
\t\t\t\t\t\tOFFSET 0.0 9.0 0.0
\t\t\t\t\t}
\t\t\t\t}
\t\t\t}
\t\t\tJOINT LeftCollar
\t\t\t{
\t\t\t\tOFFSET 3.5 11.0 0.25
\t\t\t\tCHANNELS 3 Yrotation Zrotation Xrotation
\t\t\t\tJOINT LeftArm
\t\t\t\t{
\t\t\t\t\tOFFSET 14.0 0.5 -0.25
\t\t\t\t\tCHANNELS 3 Xrotation Zrotation Yrotation
\t\t\t\t\tJOINT LeftHand
\t\t\t\t\t{
\t\t\t\t\t\tOFFSET 27.5 0.0 0.75
\t\t\t\t\t\tCHANNELS 3 Zrotation Xrotation Yrotation
\t\t\t\t\t\tEnd Site
\t\t\t\t\t\t{
\t\t\t\t\t\t\tOFFSET 8.0 0.0 0.0
\t\t\t\t\t\t}
\t\t\t\t\t}
\t\t\t\t}
\t\t\t}
\t\t}
\t}
}
"""
NAMES = ["Hips", "Spine", "Chest", "Neck", "Head", "LeftCollar", "LeftArm", "LeftHand"]
FILE_ORDERS = ["ZXY", "ZXY", "XYZ", "YXZ", "ZYX", "YZX", "XZY", "ZXY"]
SUBSET = ["Hips", "Chest", "Head", "LeftArm", "LeftHand"]                         # Spine, Neck and LeftCollar are skipped


def _motion_text(F=5, seed=3, zero=()):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-80.0, 80.0, (F, 27)).round(4)
    rows[:, :3] = rng.uniform(-5.0, 100.0, (F, 3)).round(4)
    for name in zero:                                                             # the rotation channels of these joints
        j = NAMES.index(name)
        rows[:, 3 + 3 * j:6 + 3 * j] = 0.0
    body = "\n".join(" ".join("%.4f" % v for v in r) for r in rows)
    return HIERARCHY + "MOTION\nFrames: %d\nFrame Time: 0.033333\n%s\n" % (F, body), rows


def test_parse_reads_every_node_and_the_motion():
    text, rows = _motion_text()
    f = BVH.parse(text)
    assert f.names == NAMES and len(f.nodes) == 10 and [nd.name for nd in f.nodes].count(None) == 2
    assert f.channels == 27 and f.frames == 5 and f.frame_time == pytest.approx(0.033333)
    assert f.nodes[0].channels[:3] == ["Xposition", "Yposition", "Zposition"] and f.nodes[0].offset == [0.0, 92.5, 1.25]
    assert [f.nodes[i].parent for i in range(10)] == [-1, 0, 1, 2, 3, 4, 2, 6, 7, 8]
    assert f.hierarchy == HIERARCHY and np.array_equal(f.motion, rows)
    assert f.orders() == FILE_ORDERS and f.orders(SUBSET) == [FILE_ORDERS[NAMES.index(n)] for n in SUBSET]
    assert np.array_equal(f.euler(), rows[:, 3:].reshape(5, 8, 3)) and np.array_equal(f.root_position(), rows[:, :3])
    assert np.array_equal(f.euler(SUBSET), rows[:, 3:].reshape(5, 8, 3)[:, [NAMES.index(n) for n in SUBSET]])
    h = BVH.parse(HIERARCHY)
    assert h.motion is None and h.frames is None and h.frame_time is None and h.names == NAMES
    with pytest.raises(L.EgError, match="no MOTION"):
        h.euler()


def test_tree_equals_from_bvh():
    f = BVH.parse(_motion_text()[0])
    for joints in (None, SUBSET):
        for kw in ({}, {"unit": 1.0, "basis": "columns"}):
            a, b = f.tree(joints, **kw), S.JointTree.from_bvh(_motion_text()[0], joints, **kw)
            assert a == b and a.names == b.names and np.array_equal(a.offsets, b.offsets) and a.basis == b.basis
    assert f.tree(SUBSET).names == SUBSET


def test_format_round_trip():
    text, rows = _motion_text()
    f = BVH.parse(text)
    rng = np.random.default_rng(8)
    e = rng.uniform(-180.0, 180.0, (7, 8, 3))
    rp = rng.uniform(-50.0, 150.0, (7, 3))
    g = BVH.parse(f.format(e, root_position=rp))
    assert g.hierarchy == HIERARCHY and g.frames == 7 and g.frame_time == pytest.approx(0.033333)
    assert np.abs(g.euler() - e).max() <= 5e-7 and np.abs(g.root_position() - rp).max() <= 5e-7
    g = BVH.parse(f.format(e[:, :5], joints=SUBSET, frame_time=1 / 15))              # the other joints: zero channels; the root: its OFFSET
    assert g.frame_time == pytest.approx(1 / 15, abs=1e-6)
    assert np.abs(g.euler(SUBSET) - e[:, :5]).max() <= 5e-7
    assert np.all(g.euler(["Spine", "Neck", "LeftCollar"]) == 0) and np.all(g.root_position() == [0.0, 92.5, 1.25])
    import torch
    assert f.format(torch.from_numpy(e)) == f.format(e)
    h = BVH.parse(HIERARCHY)
    assert BVH.parse(h.format(e, frame_time=0.05)).frames == 7
    with pytest.raises(L.EgError, match="frame_time"):
        h.format(e)
    with pytest.raises(L.EgError, match="euler shape"):
        f.format(e[:, :5])
    with pytest.raises(L.EgError, match="root_position shape"):
        f.format(e, root_position=rp[:3])


def test_write_and_read(tmp_path):
    text, _rows = _motion_text()
    f = BVH.parse(text)
    path = str(tmp_path / "take.bvh")
    f.write(path, f.euler(), root_position=f.root_position())
    g = BVH.read(path)
    assert np.abs(g.motion - f.motion).max() <= 5e-7 and g.hierarchy == f.hierarchy


def test_parser_refusals_by_name():
    text, _rows = _motion_text()
    with pytest.raises(L.EgError, match="CHANNELS 3 is followed by 2 channel words"):
        BVH.parse(text.replace("CHANNELS 3 Xrotation Yrotation Zrotation", "CHANNELS 3 Xrotation Yrotation"))
    with pytest.raises(L.EgError, match="unknown channel word 'Wrotation'"):
        BVH.parse(text.replace("Yrotation Zrotation Xrotation", "Yrotation Wrotation Xrotation"))
    with pytest.raises(L.EgError, match="repeat an axis"):
        BVH.parse(text.replace("CHANNELS 3 Xrotation Yrotation Zrotation", "CHANNELS 3 Zrotation Xrotation Zrotation"))
    lines = text.rstrip("\n").split("\n")
    with pytest.raises(L.EgError, match="MOTION row 4 has 26 numbers, the hierarchy has 27 channels"):
        BVH.parse("\n".join(lines[:-1] + [lines[-1].rsplit(" ", 1)[0]]))
    with pytest.raises(L.EgError, match="Frames: 5 but 4 rows"):
        BVH.parse("\n".join(lines[:-1]))
    f = BVH.parse(text)
    with pytest.raises(L.EgError, match="unknown joint name 'Tail'"):
        f.orders(["Hips", "Tail"])
    with pytest.raises(L.EgError, match="with names"):
        f.rot6d(S.JointTree([-1], np.zeros((1, 3))))


def _bvh_fk(f, unit):
    """Joint positions [F, nodes with a name, 3] straight from the channels and OFFSETs: the textbook BVH recursion, the root held at its
    OFFSET (a JointTree has no root translation)."""
    axis = {"X": 0, "Y": 1, "Z": 2}
    F = len(f.motion)
    G, p = {}, {}
    for n, nd in enumerate(f.nodes):
        if nd.name is None:
            continue
        R = np.tile(np.eye(3), (F, 1, 1))
        for i, w in enumerate(nd.channels):
            if w.endswith("rotation"):
                R = R @ Rot.from_euler(w[0].lower(), f.motion[:, nd.first + i], degrees=True).as_matrix()
        off = np.asarray(nd.offset) * unit
        if nd.parent < 0:
            G[n], p[n] = R, np.tile(off, (F, 1))
        else:
            G[n], p[n] = G[nd.parent] @ R, p[nd.parent] + G[nd.parent] @ off
    names = {nd.name: n for n, nd in enumerate(f.nodes) if nd.name is not None}
    return lambda keep: np.stack([p[names[k]] for k in keep], 1)


def test_bvh_forward_kinematics_equals_joints_from_rot6d():
    for joints, zero in ((None, ()), (SUBSET, ("Spine", "Neck", "LeftCollar"))):
        f = BVH.parse(_motion_text(F=9, seed=21, zero=zero)[0])
        for basis in ("rows", "columns"):
            tree = f.tree(joints, basis=basis)
            track = f.rot6d(tree)
            assert track.shape == (9, 6 * tree.J) and track.dtype == np.float64
            got = S.joints_from_rot6d(track, tree)
            ref = _bvh_fk(f, 0.01)(tree.names)
            assert np.abs(got - ref).max() < 1e-12
            e = S.euler_from_rot6d(track, tree, f.orders(joints))
            assert np.abs(_mod360(e - f.euler(joints))).max() < 1e-9              # |b| <= 80 degrees here: the principal values are the file's
        mean = np.linspace(-0.2, 0.2, 6 * tree.J)
        assert np.abs(f.rot6d(tree, mean=mean) + mean - track).max() < 1e-15
