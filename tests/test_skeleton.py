"""Skeleton output without a GPU: the float64 restatement (tests/skeleton_np.py) and emotiongestures_amd.skeleton's float64 path against
tests/golden/skeleton.npz (the reference's convert_dir_vec_to_pose / convert_pose_seq_to_dir_vec on hashed inputs), the drop-ins of
utils.data_utils_expressive, the frame-rate change against datapath.resample_pose_seq, and every refusal by name."""
import os

import numpy as np
import pytest
import torch

import skeleton_np as SN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import datapath as DP
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.utils import data_utils_expressive as DU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skeleton.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ted():
    return SK.ted_expressive()


def table_of(sk):
    return sk.parents.tolist(), sk.children.tolist(), sk.lengths.tolist()


def test_restatement_equals_the_reference(z, ted):
    t = table_of(ted)
    for tag in ("4d", "3d", "2d"):
        v = z[f"vec_{tag}"]
        got = SN.joints(v.reshape(1, -1, 126), t).reshape(z[f"pose_{tag}"].shape)
        assert np.abs(got - z[f"pose_{tag}"]).max() <= 1e-15, tag
    for tag in ("3d", "4d"):
        pose = z[f"pose_{tag}"]
        got = SN.dir_vec(pose.reshape(1, -1, 43, 3), t).reshape(z[f"dir_vec_{tag}"].shape)
        assert z[f"dir_vec_{tag}"].dtype == np.float32
        assert np.abs(got - z[f"dir_vec_{tag}"]).max() <= SN.INVERSE_BOUND, tag


def test_one_bone_inputs_pin_the_ted_table(z, ted):
    assert (ted.K, ted.J) == (42, 43) and int(ted.depth.max()) == 7
    got = SK.joints_from_tracks(z["vec_one_bone"], ted)
    assert got.dtype == np.float64 and got.shape == (42, 43, 3)
    assert np.abs(got - z["pose_one_bone"]).max() <= 1e-15
    # bone k alone moves exactly the joints below its child, by its length along x
    moved = np.abs(z["pose_one_bone"][..., 0]) > 0
    assert all(moved[k, ted.children[k]] and not moved[k, ted.parents[k]] for k in range(42))


def test_drop_ins_reproduce_the_golden(z):
    for tag, rank in (("2d", 2), ("3d", 3), ("4d", 4)):
        v, want = z[f"vec_{tag}"], z[f"pose_{tag}"]
        for inp in (v, v.reshape(v.shape[:-1] + (42, 3)), v.tolist()):
            got = DU.convert_dir_vec_to_pose(inp)
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape and got.ndim == rank
            assert np.abs(got - want).max() <= 1e-15
    for tag in ("3d", "4d"):
        pose, want = z[f"pose_{tag}"], z[f"dir_vec_{tag}"]
        for inp in (pose, pose.reshape(pose.shape[:-2] + (129,))):
            got = DU.convert_pose_seq_to_dir_vec(inp)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == want.shape
            assert np.abs(got.numpy().astype(np.float64) - want).max() <= SN.INVERSE_BOUND
    with pytest.raises(ValueError, match="convert_dir_vec_to_pose"):
        DU.convert_dir_vec_to_pose(np.zeros((2, 2, 2, 126)))
    with pytest.raises(ValueError, match="convert_pose_seq_to_dir_vec"):
        DU.convert_pose_seq_to_dir_vec(np.zeros((43, 3)))


def test_dir_vec_pairs_build_the_same_skeleton(ted):
    pairs = DU.dir_vec_pairs
    assert len(pairs) == 42 and pairs == ted.dir_vec_pairs and all(len(p) == 3 for p in pairs)
    a, b, l = zip(*pairs)
    assert SK.Skeleton(a, b, l) == ted
    assert SK.Skeleton(a, b, [2 * v for v in l]) != ted


def test_importing_the_drop_ins_does_not_load_the_library(monkeypatch):
    import importlib

    def refuse():
        raise AssertionError("the shared library was asked for at import")
    with monkeypatch.context() as m:
        m.setattr(L, "load", refuse)
        mod = importlib.reload(DU)                                      # the audio helpers are there, the body is built on first use
        assert callable(mod.make_audio_fixed_length) and callable(mod.convert_dir_vec_to_pose)
        with pytest.raises(AttributeError):
            mod.no_such_name
    assert len(DU.dir_vec_pairs) == 42 and "dir_vec_pairs" not in vars(DU)


def tracks(B, T, K, seed, scale=1.0):
    return np.random.default_rng(seed).standard_normal((B, T, 3 * K)) * scale


@pytest.mark.parametrize("dst", [30, 60])
def test_upsampling_equals_resample_pose_seq(ted, dst):
    v = tracks(2, 11, 42, 5)
    mean = tracks(1, 1, 42, 6, 0.1)[0, 0]
    native = SK.joints_from_tracks(v, ted, mean=mean)
    got, n_out = SK.joints_from_tracks(v, ted, mean=mean, fps=(15, dst))
    assert n_out == [11 * dst // 15] * 2 and got.shape == (2, 11 * dst // 15, 43, 3)
    for u in range(2):
        want = DP.resample_pose_seq(native[u], 11 / 15.0, dst)          # step 0.5 / 0.25: the reference's float positions are exact
        assert want.shape == got[u].shape and np.abs(got[u] - want).max() <= 1e-12


@pytest.mark.parametrize("dst", [25, 10])
def test_other_ratios_agree_with_the_restatement(ted, dst):
    Lf, M = SK.rate_ratio((15, dst))
    assert (Lf, M) == ((5, 3) if dst == 25 else (2, 3))
    v = tracks(3, 13, 42, 7)
    v[1, 7:] = np.nan
    v[2, 1:] = np.nan
    frames = [13, 7, 1]
    got, n_out = SK.joints_from_tracks(v, ted, frames=frames, unit=True, fps=(15, dst))
    want = SN.joints(v, table_of(ted), frames, None, True, Lf, M)
    assert n_out == [-(-n * Lf // M) for n in frames] == [SK.out_frames(n, (15, dst)) for n in frames]
    assert got.shape == want.shape == (3, -(-13 * Lf // M), 43, 3) and np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-15
    for u, n in enumerate(n_out):
        assert not got[u, n:].any() and got[u, :n].any()
    lib = L.load()
    assert [lib.eg_skeleton_out_frames(n, dst, 15) for n in frames] == n_out and lib.eg_skeleton_tile_frames() == SK.TILE_FRAMES


def test_leading_axes_and_draws_share_frames(ted):
    v = tracks(2 * 3, 6, 42, 9).reshape(2, 3, 6, 126)
    got, n_out = SK.joints_from_tracks(v, ted, frames=[6, 4])
    assert got.shape == (2, 3, 6, 43, 3) and n_out == [6, 4] and not got[1, :, 4:].any()
    flat = SN.joints(v.reshape(6, 6, 126), table_of(ted), [6, 6, 6, 4, 4, 4])
    assert np.array_equal(got.reshape(flat.shape), flat)
    one = SK.joints_from_tracks(v[0, 0], ted)
    assert one.shape == (6, 43, 3) and np.array_equal(one, got[0, 0])
    t = SK.joints_from_tracks(torch.from_numpy(v[0]), ted)             # a CPU tensor: float64 tensor out
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and np.array_equal(t.numpy(), got[0])


def test_round_trip_returns_the_unit_vectors(ted):
    for sk in (ted, SK.Skeleton(*SN.random_table())):
        v = tracks(2, 5, sk.K, 11)
        unit = (v.reshape(2, 5, sk.K, 3) / np.linalg.norm(v.reshape(2, 5, sk.K, 3), axis=-1, keepdims=True)).reshape(v.shape)
        back = SK.dir_vec_from_joints(SK.joints_from_tracks(v, sk, unit=True), sk)
        assert back.shape == v.shape and np.abs(back - unit).max() <= 1e-13
        mean = tracks(1, 1, sk.K, 12, 0.1)[0, 0]
        assert np.abs(SK.dir_vec_from_joints(SK.joints_from_tracks(v, sk, unit=True), sk, mean=mean) - (unit - mean)).max() <= 1e-13
    p = np.zeros((1, 1, 6, 3))
    assert not SK.dir_vec_from_joints(p, SK.Skeleton(*SN.chain_table())).any()      # zero-length bones: zero vectors


@pytest.mark.parametrize("table, words", [
    (([], [], []), r"bones=0 \(1\.\.63\)"),
    ((list(range(64)), list(range(1, 65)), [0.1] * 64), r"bones=64 \(1\.\.63\)"),
    (([0, 1], [1, 0], [0.1, 0.1]), "bone 1: child is joint 0, the root"),
    (([0, 0], [1, 1], [0.1, 0.1]), "bone 1: child=1 is the child of an earlier bone"),
    (([0, 0], [1, 3], [0.1, 0.1]), r"bone 1: child=3 outside the joints 1\.\.2"),
    (([2, 0], [1, 2], [0.1, 0.1]), "bone 0: parent=2 is neither the root nor the child of an earlier bone"),
    (([0, 1], [1, 2], [0.1, 0.0]), r"bone 1: length=0 \(need finite and > 0\)"),
    (([0, 1], [1, 2], [float("inf"), 0.1]), r"bone 0: length=inf"),
    (([0, 1], [1, 2], [0.1, float("nan")]), r"bone 1: length=nan"),
    (([0, 1], [1, 2], [-0.1, 0.1]), r"bone 0: length=-0\.1"),
])
def test_a_bad_table_is_refused_by_name(table, words):
    with pytest.raises(L.EgError, match="eg_skeleton_check.*" + words):
        SK.Skeleton(*table)


def test_other_refusals_by_name(ted):
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd import streaming as S
    v = tracks(2, 4, 42, 1)
    with pytest.raises(L.EgError, match=r"fps=\(1, 65\) is the frame-rate ratio L=65 / M=1: supported up to max\(L, M\) <= 64"):
        SK.joints_from_tracks(v, ted, fps=(1, 65))
    with pytest.raises(L.EgError, match=r"L=1 / M=65"):
        SK.joints_from_tracks(v, ted, fps=(130, 2))
    assert L.load().eg_skeleton_out_frames(10, 65, 1) == -1 and L.load().eg_skeleton_out_frames(10, 128, 2) == 640
    with pytest.raises(L.EgError, match="frames has 3 entries for 2 recordings"):
        SK.joints_from_tracks(v, ted, frames=[1, 2, 3])
    with pytest.raises(L.EgError, match="frames has 1 entries for 2 recordings"):
        SK.dir_vec_from_joints(np.zeros((2, 4, 43, 3)), ted, frames=[4])
    with pytest.raises(L.EgError, match=r"every value must be in \[0, 4\]"):
        SK.joints_from_tracks(v, ted, frames=[4, 5])
    with pytest.raises(L.EgError, match="3K=126 columns per frame, not 282"):
        SK.joints_from_tracks(np.zeros((1, 4, 282)), ted)
    with pytest.raises(L.EgError, match=r"synthesize: joints=.*3K=126 != pose_dim=282"):
        Hs.synthesize((None, None), torch.zeros(1, 10), torch.zeros(1, 1, 60), torch.zeros(1, 10, 282), joints=ted)
    with pytest.raises(L.EgError, match="synthesize: joints_fps.*L=65 / M=1"):
        Hs.synthesize((None, None), torch.zeros(1, 10), torch.zeros(1, 1, 60), torch.zeros(1, 4, 126), joints=ted, joints_fps=(1, 65))
    with pytest.raises(L.EgError, match="GestureStream: joints_fps= is not supported"):
        S.GestureStream((None, None, None), 2, torch.zeros(2, 4, 126), joints=ted, joints_fps=(15, 30))
    with pytest.raises(L.EgError, match="GestureStream: joints_fps= is not supported"):
        Hs.open_stream((None, None), 2, torch.zeros(2, 4, 126), joints=ted, joints_fps=(15, 30))
