"""Articulated bodies without a GPU: skeleton.JointTree, the float64 path of joints_from_rot6d / rotations_from_rot6d / rot6d_from_rotations
against the restatement tests/articulate_np.py, the properties a rig relies on, JointTree.from_bvh, and every refusal by name."""
import ctypes as C

import numpy as np
import pytest
import torch

import articulate_np as AN
import skeleton_np as SN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd import streaming as ST

RATES = [(1, 1), (2, 1), (5, 3), (2, 3)]
FPS = {(1, 1): None, (2, 1): (15, 30), (5, 3): (15, 25), (2, 3): (15, 10)}


def tree_of(name, basis="rows"):
    parents, offsets = AN.BODIES[name]()
    return (parents, offsets), SK.JointTree(parents, offsets, basis=basis)


def up_to_sign(a, b):
    return np.minimum(np.abs(a - b), np.abs(a + b))


def test_joint_tree_holds_the_table_and_its_levels():
    (parents, offsets), tree = tree_of("upper47")
    assert tree.J == 47 and tree.pose_dim == 282 and tree.basis == "rows" and tree.names is None
    assert tree.depth.tolist() == AN.depth(parents) and tree.depth.max() >= 10 and tree.levels == tree.depth.max() + 1
    assert "joints=47" in repr(tree) and f"levels={tree.levels}" in repr(tree) and "rows" in repr(tree)
    assert tree == SK.JointTree(parents, offsets) and tree != SK.JointTree(parents, offsets, basis="columns")
    assert tree != SK.JointTree(parents, offsets * 2) and tree != "upper47"
    # the level table: count | 65 level offsets | order | parents | offsets (fp32 bits)
    w = tree.words
    assert len(w) == SK.articulate_level_words(47) == 66 + 5 * 47 and w[0] == tree.levels
    order = w[66:66 + 47].tolist()
    assert sorted(order) == list(range(47)) and [tree.depth[j] for j in order] == sorted(tree.depth.tolist())
    for l in range(tree.levels):
        assert all(tree.depth[j] == l for j in order[w[1 + l]:w[2 + l]])
    assert (w[1 + tree.levels:66] == 47).all()
    assert w[66 + 47:66 + 94].tolist() == parents
    assert np.array_equal(w[66 + 94:].view(np.float32).reshape(47, 3), offsets.astype(np.float32))
    assert L.load().eg_articulate_tile_frames() == SK.ARTICULATE_TILE_FRAMES == L.EG_ARTICULATE_TILE_FRAMES
    named = SK.JointTree([-1, 0], np.zeros((2, 3)), names=["a", "b"])
    assert named.names == ["a", "b"] and named.depth.tolist() == [0, 1]
    chain64 = SK.JointTree(*AN.chain(64))
    assert chain64.levels == 64 and chain64.words[1:66].tolist() == list(range(64)) + [64]


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(AN.BODIES))
def test_float64_path_equals_the_restatement(name, rate):
    Lf, M = rate
    frames = [1, 11, 6]
    for basis in ("rows", "columns"):
        body, tree = tree_of(name, basis)
        J, cols = tree.J, basis == "columns"
        mean = (np.random.default_rng(4).standard_normal(6 * J) * 0.2).astype(np.float32) if cols else None
        v = AN.rotation_tracks(J, 11, 21, B=3, columns=cols, mean=mean)
        for b, n in enumerate(frames):
            v[b, n:] = np.nan
        m64 = None if mean is None else mean.astype(np.float64)
        for space in ("local", "global"):
            wj, wq = AN.articulate(v, body, cols, frames, m64, space, Lf, M)
            gj, n_out = SK.joints_from_rot6d(v, tree, frames=frames, mean=mean, fps=FPS[rate])
            gq, n_q = SK.rotations_from_rot6d(v, tree, frames=frames, mean=mean, fps=FPS[rate], space=space)
            assert n_out == n_q == [SN.out_frames(n, Lf, M) for n in frames]
            assert gj.dtype == gq.dtype == np.float64 and gj.shape == wj.shape and gq.shape == wq.shape
            assert np.isfinite(gj).all() and np.isfinite(gq).all()
            assert np.abs(gj - wj).max() <= 1e-14 and np.abs(gq - wq).max() <= 1e-14, (name, rate, basis, space)
            for b, n in enumerate(n_out):
                assert not gj[b, n:].any() and not gq[b, n:].any() and gq[b, :n].any()
    # tensors, the draws axis, a single track
    body, tree = tree_of(name)
    J = tree.J
    v = AN.rotation_tracks(J, 8, 22, B=2)
    x = torch.from_numpy(v.reshape(1, 2, 8, 6 * J))
    got = SK.rotations_from_rot6d(x, tree)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == (1, 2, 8, J, 4)
    assert np.abs(got.numpy().reshape(2, 8, J, 4) - AN.articulate(v, body)[1]).max() <= 1e-14
    one, n1 = SK.joints_from_rot6d(v[1], tree, frames=5)
    assert one.shape == (8, J, 3) and n1 == [5] and not one[5:].any() and np.abs(one[:5] - AN.articulate(v[1:, :5], body)[0][0]).max() <= 1e-14


@pytest.mark.parametrize("basis", ["rows", "columns"])
@pytest.mark.parametrize("name", ["upper47", "chain", "random64"])
def test_rotations_and_joints_describe_one_pose(name, basis):
    """Local rotations are unit with w >= 0; the product of the locals along a path is the global, up to sign; forward kinematics from the
    returned local rotations and the offsets reproduces the returned joints -- also on resampled frames."""
    body, tree = tree_of(name, basis)
    parents, offsets = body
    v = AN.rotation_tracks(tree.J, 9, 31, B=2, columns=basis == "columns")
    for fps in (None, (15, 25)):
        res = [f(v, tree, fps=fps) for f in (SK.joints_from_rot6d, SK.rotations_from_rot6d)]
        joints, loc = (r if fps is None else r[0] for r in res)
        glob = SK.rotations_from_rot6d(v, tree, fps=fps, space="global")
        glob = glob if fps is None else glob[0]
        assert np.abs(np.sqrt((loc * loc).sum(-1)) - 1).max() <= 1e-14 and (loc[..., 0] >= 0).all() and (glob[..., 0] >= 0).all()
        assert up_to_sign(AN.globals_from_locals(parents, loc), glob).max() <= 1e-12
        assert np.abs(AN.fk(body, loc) - joints).max() <= 1e-12 * max(1.0, AN.path_length(body))
        assert np.array_equal(joints[:, :, 0], np.broadcast_to(offsets[0], joints[:, :, 0].shape))


@pytest.mark.parametrize("basis", ["rows", "columns"])
def test_rot6d_round_trip(basis):
    body, tree = tree_of("upper47", basis)
    cols = basis == "columns"
    J = tree.J
    mean = (np.random.default_rng(5).standard_normal(6 * J) * 0.2).astype(np.float64)
    x = AN.rotation_tracks(J, 7, 41, B=2, columns=cols).astype(np.float64)
    q = SK.rotations_from_rot6d(x, tree)
    d = SK.rot6d_from_rotations(q, tree)
    gs = np.concatenate(AN.gram_schmidt(x.reshape(2, 7, J, 6))[:2], -1).reshape(2, 7, 6 * J)       # b1 | b2: the Gram-Schmidt rows (columns)
    assert d.shape == x.shape and np.abs(d - gs).max() <= 1e-14
    assert np.abs(SK.rotations_from_rot6d(d, tree) - q).max() <= 1e-14
    assert np.abs(d - AN.rot6d(q, cols)).max() <= 1e-15
    # the mean, ragged rows, quaternions of any length, tensors, the draws axis
    got = SK.rot6d_from_rotations(3.0 * q, tree, frames=[7, 2], mean=mean)
    assert np.abs(got - AN.rot6d(3.0 * q, cols, [7, 2], mean)).max() <= 1e-14 and not got[1, 2:].any()
    assert np.abs(got[0] + mean - d[0]).max() <= 1e-14
    t = SK.rot6d_from_rotations(torch.from_numpy(q.reshape(1, 2, 7, J, 4)), tree, frames=[3])
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (1, 2, 7, 6 * J) and not t[:, :, 3:].any()
    assert np.array_equal(t.numpy()[0, :, :3], d[:, :3])
    zero = SK.rot6d_from_rotations(np.zeros((1, J, 4)), tree)                                      # a zero quaternion: finite
    assert np.isfinite(zero).all()


def test_degenerate_groups_stay_finite_and_identity_is_exact():
    body, tree = tree_of("upper47")
    parents, offsets = body
    J = tree.J
    ident = np.tile(np.array([1.0, 0, 0, 0, 1, 0]), (1, 3, J))
    j, q = SK.joints_from_rot6d(ident, tree), SK.rotations_from_rot6d(ident, tree, space="global")
    assert np.array_equal(q, np.broadcast_to(np.array([1.0, 0, 0, 0]), q.shape))
    want = np.zeros((J, 3))
    for k in range(J):
        want[k] = offsets[k] + (0 if parents[k] < 0 else want[parents[k]])
    assert np.array_equal(j, np.broadcast_to(want, j.shape))
    for bad in (np.zeros((1, 2, 6 * J)), np.tile(np.array([1.0, 2, 3, 2, 4, 6]), (1, 2, J))):
        for space in ("local", "global"):
            assert np.isfinite(SK.rotations_from_rot6d(bad, tree, space=space)).all() and np.isfinite(SK.joints_from_rot6d(bad, tree)).all()


BVH = """HIERARCHY
ROOT Hips
{
  OFFSET 0.0 90.0 0.0
  CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation
  JOINT Spine
  {
    OFFSET 0.0 10.0 0.5
    CHANNELS 3 Zrotation Xrotation Yrotation
    JOINT Neck
    {
      OFFSET 0.0 30.0 1.0
      CHANNELS 3 Zrotation Xrotation Yrotation
      End Site
      {
        OFFSET 0.0 5.0 0.0
      }
    }
    JOINT LeftArm
    {
      OFFSET 10.0 25.0 0.0
      CHANNELS 3 Zrotation Xrotation Yrotation
      JOINT LeftHand
      {
        OFFSET 20.0 0.0 0.0
        CHANNELS 3 Zrotation Xrotation Yrotation
        End Site
        {
          OFFSET 8.0 0.0 0.0
        }
      }
    }
  }
  JOINT Leg
  {
    OFFSET 5.0 -10.0 0.0
    CHANNELS 3 Zrotation Xrotation Yrotation
    End Site
    {
      OFFSET 0.0 -40.0 0.0
    }
  }
}
MOTION
Frames: 1
Frame Time: 0.0333
0 90 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0
"""


def test_from_bvh():
    tree = SK.JointTree.from_bvh(BVH)
    assert tree.names == ["Hips", "Spine", "Neck", "LeftArm", "LeftHand", "Leg"] and tree.parents.tolist() == [-1, 0, 1, 1, 3, 0]
    want = np.array([[0, 90, 0], [0, 10, 0.5], [0, 30, 1], [10, 25, 0], [20, 0, 0], [5, -10, 0]]) * 0.01
    assert np.abs(tree.offsets - want).max() <= 1e-15 and tree.basis == "rows" and tree.pose_dim == 36
    # a subset, given in any order, kept in file order: the offsets of the skipped joints are summed
    sub = SK.JointTree.from_bvh(BVH, joints=["LeftHand", "Hips", "Neck"], unit=1.0, basis="columns")
    assert sub.names == ["Hips", "Neck", "LeftHand"] and sub.parents.tolist() == [-1, 0, 0] and sub.basis == "columns"
    assert np.array_equal(sub.offsets, np.array([[0, 90, 0], [0, 40, 1.5], [30, 35, 0.5]]))
    # exact while the skipped joints stay at identity: the subset's joints are the full body's
    full = SK.JointTree.from_bvh(BVH, unit=1.0, basis="columns")
    x = AN.rotation_tracks(6, 4, 3, columns=True).astype(np.float64).reshape(1, 4, 6, 6)
    x[:, :, [1, 3]] = [1, 0, 0, 0, 1, 0]                                                          # Spine and LeftArm at identity
    jf = SK.joints_from_rot6d(x.reshape(1, 4, 36), full)
    js = SK.joints_from_rot6d(x[:, :, [0, 2, 4]].reshape(1, 4, 18), sub)
    assert np.abs(js - jf[:, :, [0, 2, 4]]).max() <= 1e-12
    # a subtree: the first kept joint is the root
    arm = SK.JointTree.from_bvh(BVH, joints=["LeftArm", "LeftHand"])
    assert arm.parents.tolist() == [-1, 0] and np.abs(arm.offsets - np.array([[0.1, 0.25, 0], [0.2, 0, 0]])).max() <= 1e-15
    with pytest.raises(L.EgError, match="from_bvh: joints: unknown joint name 'Tail'"):
        SK.JointTree.from_bvh(BVH, joints=["Hips", "Tail"])
    with pytest.raises(L.EgError, match="from_bvh: joints: duplicate joint name 'Neck'"):
        SK.JointTree.from_bvh(BVH, joints=["Hips", "Neck", "Neck"])
    with pytest.raises(L.EgError, match="from_bvh: joints: 'Leg' does not descend from 'Spine'"):
        SK.JointTree.from_bvh(BVH, joints=["Spine", "Leg"])
    with pytest.raises(L.EgError, match="from_bvh: no ROOT / JOINT"):
        SK.JointTree.from_bvh("MOTION\nFrames: 0\n")


def test_tree_and_table_refusals_by_name():
    lib = L.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    off = np.zeros((65, 3), np.float32)
    for parents, word in (([0, 0], "joint 0: parent=0"), ([-1, 1], "joint 1: parent=1 is not an earlier joint"),
                          ([-1, 0, 3, 0], "joint 2: parent=3 is not an earlier joint"), ([-1, -1], "joint 1: parent=-1 is not an earlier joint"),
                          ([-1] + [0] * 64, r"joints=65 \(1..64\)"), ([], r"joints=0 \(1..64\)")):
        with pytest.raises(L.EgError, match=f"eg_articulate_check: {word}"):
            SK.JointTree(parents, np.zeros((len(parents), 3)))
        p = np.array(parents, np.int32)
        assert lib.eg_articulate_check(ptr(p) if len(p) else ptr(off), ptr(off), len(p)) != 0
        words = np.zeros(66 + 5 * 65, np.int32)
        assert lib.eg_articulate_levels(ptr(p) if len(p) else ptr(off), ptr(off), len(p), ptr(words)) != 0 and b"eg_articulate_levels" in lib.eg_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        o = np.zeros((3, 3))
        o[2, 1] = bad
        with pytest.raises(L.EgError, match="eg_articulate_check: joint 2: offset .* is not finite"):
            SK.JointTree([-1, 0, 1], o)
    assert lib.eg_articulate_check(None, ptr(off), 2) != 0 and b"null parents / offsets" in lib.eg_last_error()
    p = np.array([-1, 0], np.int32)
    assert lib.eg_articulate_check(ptr(p), ptr(off), 2) == 0
    assert lib.eg_articulate_levels(ptr(p), ptr(off), 2, None) != 0 and b"null words" in lib.eg_last_error()
    with pytest.raises(L.EgError, match="JointTree: basis='xyz'"):
        SK.JointTree([-1], np.zeros((1, 3)), basis="xyz")
    with pytest.raises(L.EgError, match=r"JointTree: offsets shape \(2, 2\)"):
        SK.JointTree([-1, 0], np.zeros((2, 2)))
    with pytest.raises(L.EgError, match="JointTree: names: need 2 distinct names"):
        SK.JointTree([-1, 0], np.zeros((2, 3)), names=["a", "a"])


def test_function_refusals_by_name():
    _body, tree = tree_of("chain")
    v = np.zeros((2, 4, 30), np.float32)
    for f in (SK.joints_from_rot6d, SK.rotations_from_rot6d):
        who = f.__name__
        with pytest.raises(L.EgError, match=f"{who}: tree must be a JointTree, got Skeleton"):
            f(np.zeros((4, 126)), SK.ted_expressive())
        with pytest.raises(L.EgError, match=f"{who}: track shape .*J=5 joints takes 6J=30 columns per frame, not 29"):
            f(np.zeros((4, 29)), tree)
        with pytest.raises(L.EgError, match=f"{who}: track shape"):
            f(np.zeros((0, 30)), tree)
        with pytest.raises(L.EgError, match="frames has 1 entries for 2"):
            f(v, tree, frames=[3])
        with pytest.raises(L.EgError, match="every value must be in"):
            f(v, tree, frames=[3, 5])
        with pytest.raises(L.EgError, match=f"{who}: fps"):
            f(v, tree, fps=(1, 65))
        with pytest.raises(L.EgError, match="mean has 15 values, the skeleton's tracks have 30"):
            f(v, tree, mean=np.zeros(15))
        with pytest.raises(L.EgError, match="at most two leading axes"):
            f(np.zeros((1, 1, 1, 4, 30)), tree)
    with pytest.raises(L.EgError, match="rotations_from_rot6d: space='world'"):
        SK.rotations_from_rot6d(v, tree, space="world")
    with pytest.raises(L.EgError, match=r"rot6d_from_rotations: quat shape \(4, 5, 3\): need \[..., T >= 1, 5, 4\]"):
        SK.rot6d_from_rotations(np.zeros((4, 5, 3)), tree)
    with pytest.raises(L.EgError, match="rot6d_from_rotations: tree must be a JointTree"):
        SK.rot6d_from_rotations(np.zeros((4, 5, 4)), None)
    with pytest.raises(L.EgError, match="mean has 5 values"):
        SK.rot6d_from_rotations(np.zeros((4, 5, 4)), tree, mean=np.zeros(5))
    with pytest.raises(L.EgError, match="frames has 2 entries for 1"):
        SK.rot6d_from_rotations(np.zeros((4, 5, 4)), tree, frames=[1, 2])


def test_device_calls_refuse_before_any_launch():
    """No GPU here: the arguments are checked before the launch, each with a message that names the argument."""
    lib = L.load()
    _body, tree = tree_of("chain")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    buf = np.zeros(4096, np.float32)
    a = buf[(-buf.ctypes.data % 16) // 4:]                        # 16-byte aligned
    odd = a[1:]
    words = tree.words

    def forward(track=a, rows=2, T=4, J=5, table=words, draws=1, unit=1, mean=None, basis=0, space=0, Lf=1, M=1, oj=a, oq=a, stride=4):
        return lib.eg_articulate_forward(None if track is None else ptr(track), rows, T, *tree.host_ptrs(), J, None if table is None else ptr(table),
                                         None, draws, unit, None if mean is None else ptr(mean), basis, space, Lf, M,
                                         None if oj is None else ptr(oj), None if oq is None else ptr(oq), stride, None)

    for kw, word in ((dict(oj=None, oq=None), "null out_joints and out_rotations"), (dict(table=None), "null d_table"), (dict(track=None), "null input"),
                     (dict(J=65), r"joints=65 (1..64)"), (dict(track=odd), "input not 16-byte aligned"), (dict(oj=odd), "out_joints / out_rotations not 16-byte aligned"),
                     (dict(oq=odd, oj=None), "out_joints / out_rotations not 16-byte aligned"), (dict(mean=buf.view(np.uint8)[1:]), "d_mean not 4-byte aligned"),
                     (dict(table=words.view(np.uint8)[2:]), "d_table not 4-byte aligned"), (dict(rows=0), "rows=0 frames=4"), (dict(T=0), "rows=2 frames=0"),
                     (dict(rows=3, draws=2), "rows=3 is not a multiple of draws=2"), (dict(draws=0), "rows=2 is not a multiple of draws=0"),
                     (dict(unit=0), "frame_unit=0"), (dict(basis=2), "basis=2 (0: rows, 1: columns)"), (dict(space=2), "space=2 (0: local, 1: global)"),
                     (dict(Lf=0), "rate L=0 / M=1"), (dict(Lf=65), "max(L, M) <= 64"), (dict(stride=3), "out_stride=3 < 4 output frames"),
                     (dict(Lf=2, stride=7), "out_stride=7 < 8 output frames"), (dict(rows=1 << 30, T=1 << 20), "index range")):
        assert forward(**kw) != 0, kw
        msg = lib.eg_last_error().decode()
        assert msg.startswith("eg_articulate_forward: ") and word in msg, (kw, msg)

    def inverse(quat=a, rows=2, T=4, J=5, draws=1, unit=1, mean=None, basis=0, out=a):
        return lib.eg_articulate_rot6d(None if quat is None else ptr(quat), rows, T, J, None, draws, unit, None if mean is None else ptr(mean), basis,
                                       None if out is None else ptr(out), None)

    for kw, word in ((dict(out=None), "null output"), (dict(quat=None), "null input"), (dict(J=0), "joints=0 (1..64)"), (dict(quat=odd), "input not 16-byte aligned"),
                     (dict(out=odd), "output not 16-byte aligned"), (dict(mean=buf.view(np.uint8)[1:]), "d_mean not 4-byte aligned"),
                     (dict(rows=3, draws=2), "rows=3 is not a multiple of draws=2"), (dict(T=0), "rows=2 frames=0"), (dict(unit=0), "frame_unit=0"),
                     (dict(basis=-1), "basis=-1 (0: rows, 1: columns)"), (dict(rows=1 << 30, T=1 << 20), "grid / index range")):
        assert inverse(**kw) != 0, kw
        msg = lib.eg_last_error().decode()
        assert msg.startswith("eg_articulate_rot6d: ") and word in msg, (kw, msg)
    # the wrappers
    x = torch.zeros(2, 4, 30)
    with pytest.raises(L.EgError, match="launch_articulate: a tree of 5 joints takes tracks of 30 columns, got 24"):
        SK.launch_articulate(torch.zeros(2, 4, 24), tree)
    with pytest.raises(L.EgError, match="launch_articulate: neither joints nor rotations"):
        SK.launch_articulate(x, tree, joints=False, rotations=False)
    with pytest.raises(L.EgError, match="launch_articulate: space='world'"):
        SK.launch_articulate(x, tree, space="world")
    with pytest.raises(L.EgError, match="out_joints has 4 frames per row, out_rotations 5"):
        SK.launch_articulate(x, tree, out_joints=torch.zeros(2, 4, 5, 3), out_rotations=torch.zeros(2, 5, 5, 4))


def test_callers_check_the_joint_tree():
    _body, tree = tree_of("upper47")
    _b5, small = tree_of("chain")
    audio, text = torch.zeros(1, 10), torch.zeros(1, 1, 60)
    beat_seed, ted_seed = torch.zeros(1, 10, 282), torch.zeros(1, 4, 126)
    syn = lambda seed, **kw: Hs.synthesize((None, None), audio, text, seed, **kw)
    with pytest.raises(L.EgError, match=r"synthesize: joints=: the joint tree has J=47 joints, 6J=282 != pose_dim=126"):
        syn(ted_seed, joints=tree)
    with pytest.raises(L.EgError, match=r"synthesize: joints=: the joint tree has J=5 joints, 6J=30 != pose_dim=282"):
        syn(beat_seed, joints=small)
    with pytest.raises(L.EgError, match=r"synthesize: joints=.*3K=126 != pose_dim=282 \(the BEAT generators' 282 columns hold rotations.*JointTree"):
        syn(beat_seed, joints=SK.ted_expressive())
    with pytest.raises(L.EgError, match="synthesize: joints_unit=True with joints=JointTree"):
        syn(beat_seed, joints=tree, joints_unit=True)
    for rest in (np.zeros((47, 3)), False, 1, "local"):
        with pytest.raises(L.EgError, match="synthesize: rotations= with joints=JointTree takes True, got .* there is no rest"):
            syn(beat_seed, joints=tree, rotations=rest)
    with pytest.raises(L.EgError, match="synthesize: rotations_space without rotations=rest"):
        syn(beat_seed, joints=tree, rotations_space="global")
    with pytest.raises(L.EgError, match="synthesize: rotations_space: space='world'"):
        syn(beat_seed, joints=tree, rotations=True, rotations_space="world")
    with pytest.raises(L.EgError, match="synthesize: joints_fps"):
        syn(beat_seed, joints=tree, joints_fps=(1, 65))
    with pytest.raises(L.EgError, match="synthesize: rotations= without joints=skeleton"):
        syn(beat_seed, rotations=True)
    with pytest.raises(L.EgError, match="synthesize_takes: joints=: the joint tree has J=5 joints"):
        Hs.synthesize_takes((None, None), audio, text, beat_seed, draws=2, joints=small)
    # the stream: the same checks, and what a stream refuses with any body
    with pytest.raises(L.EgError, match="GestureStream: joints_fps= is not supported"):
        ST.GestureStream((None, None, None), 1, beat_seed, joints=tree, joints_fps=(15, 30))
    with pytest.raises(L.EgError, match="GestureStream: smooth= together with joints= is not supported"):
        ST.GestureStream((None, None, None), 1, beat_seed, joints=tree, smooth=(9, 3))
    assert SK.TrackOutputs("x", tree, None, False, None, None, "local", pose_dim=282).want_rotations is False
    assert SK.TrackOutputs("x", tree, None, False, (15, 30), True, "global", pose_dim=282).want_rotations is True
    with pytest.raises(L.EgError, match="x: joints=: the joint tree has J=47 joints, 6J=282 != pose_dim=126"):
        SK.TrackOutputs("x", tree, None, False, None, True, "local", pose_dim=126, streaming=True)
    with pytest.raises(L.EgError, match="x: joints_unit=True with joints=JointTree"):
        SK.TrackOutputs("x", tree, None, True, None, None, "local", pose_dim=282, streaming=True)
