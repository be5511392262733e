"""Rotation output without a GPU: the restatement tests/rotations_np.py against its own consequences (G_k o rest_k = x^_k, forward kinematics of
the locals = the unit joints), the stated edge cases, the float64 path of emotiongestures_amd.skeleton against the restatement, the host side
of the C ABI (eg_skeleton_rest_check / eg_skeleton_levels), the tolerance rule of the GPU tests (that it discriminates), and every refusal by name."""
import ctypes as C

import numpy as np
import pytest
import torch

import rotations_np as RN
import skeleton_np as SN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd import streaming as ST

TABLES = {"ted": None, "chain": SN.chain_table(), "star": SN.star_table(), "random63": SN.random_table()}
RATES = [(1, 1), (2, 1), (5, 3), (2, 3)]
FPS = {(1, 1): None, (2, 1): (15, 30), (5, 3): (15, 25), (2, 3): (15, 10)}


def table(name):
    if name == "ted":
        sk = SK.ted_expressive()
        return sk.parents.tolist(), sk.children.tolist(), sk.lengths.tolist()
    return TABLES[name]


def rest_of(name, seed=5):
    return RN.random_rest(len(table(name)[0]), seed)


@pytest.mark.parametrize("name", list(TABLES))
def test_bone_parents(name):
    t = table(name)
    sk = SK.Skeleton(*t)
    pb = sk.bone_parents
    assert pb.tolist() == RN.bone_parents(t) and len(pb) == sk.K
    for k in range(sk.K):
        assert pb[k] < k
        assert (pb[k] == -1 and t[0][k] == 0) or t[1][pb[k]] == t[0][k]
    if name == "chain":
        assert pb.tolist() == [-1, 0, 1, 2, 3]
    if name == "star":
        assert pb.tolist() == [-1] * 5


@pytest.mark.parametrize("name", list(TABLES))
def test_level_table_and_rest_rows_of_the_host_call(name):
    """eg_skeleton_levels: levels by depth in table order, pb, and the rest rows normalised in float64 -- the bits numpy gives."""
    t = table(name)
    sk = SK.Skeleton(*t)
    raw = np.random.default_rng(11).standard_normal((sk.K, 3)) * 7.0
    pose = sk.rest_pose(raw)
    assert sk.rest_pose(raw) is pose                                     # built once per pose
    w, K = pose.words, sk.K
    assert len(w) == 65 + 5 * K
    pb = RN.bone_parents(t)
    depth = [0] * K
    for k in range(K):
        depth[k] = 0 if pb[k] < 0 else depth[pb[k]] + 1
    nlev = max(depth) + 1
    assert w[0] == nlev and w[65 + K:65 + 2 * K].tolist() == pb
    order = sorted(range(K), key=lambda k: (depth[k], k))
    assert w[65:65 + K].tolist() == order
    offs = [sum(d < l for d in depth) for l in range(64)]
    assert w[1:65].tolist() == offs and offs[nlev] == K
    assert np.array_equal(w[65 + 2 * K:].view(np.float32).reshape(K, 3), RN.unit_rest(raw))
    assert np.array_equal(pose.unit32, RN.unit_rest(raw))
    if name == "ted":
        assert nlev == 7 and max(np.diff(offs[:nlev + 1])) == 10


@pytest.mark.parametrize("name", list(TABLES))
def test_the_host_call_fills_level_words_and_no_more(name):
    """skeleton.level_words(K) is the table eg_skeleton_levels writes: every word of it, and nothing behind it."""
    sk = SK.Skeleton(*table(name))
    n, mark = SK.level_words(sk.K), 0x7F7F7F7F                           # no offset, bone number or component of a unit vector
    words = np.full(n + 8, mark, np.int32)
    raw = rest_of(name).astype(np.float64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.load().eg_skeleton_levels(*sk.host_ptrs(), sk.K, ptr(raw), ptr(words)) == 0
    assert (words[:n] != mark).all() and (words[n:] == mark).all()


@pytest.mark.parametrize("name", list(TABLES))
def test_globals_turn_the_rest_pose_into_the_track(name):
    t, rest = table(name), rest_of(name)
    K = len(rest)
    mean = (np.random.default_rng(3).standard_normal(3 * K) * 0.2).astype(np.float32)
    # The rest rows are unit only to fp32 rounding, |rest_k| = 1 + e with |e| <= 2^-24 or so, and arc() takes them for unit: the image of rest_k
    # misses x^_k by about e (1 + tan(theta / 2)) per bone -- below 1e-7 for swings up to 100 degrees, while at 175 degrees tan is 22.9.
    for cap, m, tol in ((100, None, 1e-7), (100, mean, 1e-7), (175, mean, 2.0 ** -23 * (1 + np.tan(np.deg2rad(87.5))))):
        v, _loc = RN.swing_tracks(t, rest, 64, cap, 7, B=2, mean=m)
        G = RN.rotations(v, t, rest, mean=m, space="global")
        x = RN.unit_vectors(v, t, mean=m)
        assert np.abs(RN.directions(G, rest) - x).max() <= tol
        loc = RN.rotations(v, t, rest, mean=m)
        assert np.abs(np.sqrt((loc * loc).sum(-1)) - 1).max() <= 1e-12 and (loc[..., 0] >= 0).all()
        assert np.abs(RN.globals_from_locals(t, loc) - G).max() <= 1e-12


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(TABLES))
def test_forward_kinematics_of_the_locals_gives_the_unit_joints(name, rate):
    t, rest = table(name), rest_of(name)
    Lf, M = rate
    v, _loc = RN.swing_tracks(t, rest, 40, 100, 9, B=2, smooth=True)
    loc = RN.rotations(v, t, rest, L=Lf, M=M)
    if rate == (1, 1):
        want = SN.joints(v, t, unit=True)
    else:                                                                  # the vectors are blended, so the joints are those of the blended frame
        x = RN.unit_vectors(v, t, L=Lf, M=M)
        want = SN.chain(t, x)
    assert np.abs(RN.fk(t, rest, loc) - want).max() <= 1e-6


def test_known_swings_are_recovered():
    t, rest = table("ted"), rest_of("ted")
    v, loc = RN.swing_tracks(t, rest, 256, 100, 13)
    got, cmin = RN.rotations(v, t, rest, want_c=True)
    assert 1 + cmin >= 0.5
    assert np.abs(got - loc).max() <= 1e-6                                # the track is fp32


def test_the_generators_stay_away_from_the_half_turn():
    """min(1 + c) >= 0.5 for the inputs the accuracy tests use: cap 100 degrees, per-frame and smooth, at every rate."""
    t, rest = table("ted"), rest_of("ted")
    v, _ = RN.swing_tracks(t, rest, 4096, 100, 1)
    assert 1 + RN.rotations(v, t, rest, want_c=True)[1] >= 0.5
    for Lf, M in RATES:
        v, _ = RN.swing_tracks(t, rest, 300, 100, 1, smooth=True)
        assert 1 + RN.rotations(v, t, rest, L=Lf, M=M, want_c=True)[1] >= 0.5


def test_rest_pose_and_zero_vectors_give_identities():
    t, rest = table("ted"), rest_of("ted")
    K = len(rest)
    scales = np.random.default_rng(2).uniform(0.1, 9.0, (1, 5, K, 1))
    v = (rest.astype(np.float64) * scales).reshape(1, 5, 3 * K).astype(np.float32)
    ident = np.array([1.0, 0, 0, 0])
    for space in ("local", "global"):
        assert np.abs(RN.rotations(v, t, rest, space=space) - ident).max() <= 1e-7
    v[0, 2, 3 * 4:3 * 4 + 3] = 0                                          # bone 4 (the left elbow) collapses in frame 2
    loc = RN.rotations(v, t, rest)
    assert np.array_equal(loc[0, 2, 4], ident) and np.isfinite(loc).all()
    mine = SK.rotations_from_tracks(v, SK.ted_expressive(), rest)
    assert np.array_equal(mine[0, 2, 4], ident)


@pytest.mark.parametrize("rest,want", [((0, 0, 1), (0, 0, 1, 0)), ((1, 0, 0), (0, 0, 0, 1))])
def test_exact_half_turn(rest, want):
    t = ([0], [1], [0.5])
    r = np.array([rest], np.float32)
    v = (-1.5 * r).reshape(1, 1, 3)
    for dt in (np.float64, np.float32):
        assert np.array_equal(RN.rotations(v, t, r, dtype=dt)[0, 0, 0], np.array(want, dt))
    assert np.array_equal(SK.rotations_from_tracks(v, SK.Skeleton(*t), r)[0, 0, 0], np.array(want, np.float64))
    assert np.abs(RN.directions(RN.rotations(v, t, r, space="global"), r)[0, 0, 0] + r[0]).max() <= 1e-15


def test_tolerance_rule_discriminates():
    """8 x E32 (the fp32 restatement's own error) is far below what a wrong chain gives on the same inputs."""
    t, rest = table("ted"), rest_of("ted")
    v, _ = RN.swing_tracks(t, rest, 96, 100, 17, B=2)
    for space in ("local", "global"):
        want = RN.rotations(v, t, rest, space=space)
        q32 = RN.rotations(v, t, rest, space=space, dtype=np.float32)
        assert q32.dtype == np.float32
        E32 = np.minimum(np.abs(q32 - want), np.abs(q32 + want)).max() if space == "global" else np.abs(q32 - want).max()
        print(f"{space}: E32 = {E32:.3e}")
        assert 0 < 8 * E32 <= 1e-4
        for variant in ("swapped", "previous", "noconj"):
            wrong = RN.rotations(v, t, rest, space=space, variant=variant)
            dev = np.minimum(np.abs(wrong - want), np.abs(wrong + want)).max()
            assert dev > 1e-2, (space, variant, dev)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(TABLES))
def test_float64_path_equals_the_restatement(name, rate):
    t, rest = table(name), rest_of(name)
    sk = SK.Skeleton(*t)
    Lf, M = rate
    K = sk.K
    frames = [1, 20, 9]
    mean = (np.random.default_rng(4).standard_normal(3 * K) * 0.2).astype(np.float32)
    v, _ = RN.swing_tracks(t, rest, 20, 140, 21, B=3, mean=mean, smooth=True)
    for b, n in enumerate(frames):
        v[b, n:] = np.nan
    for space in ("local", "global"):
        want = RN.rotations(v, t, rest, frames, mean.astype(np.float64), space, Lf, M)
        got, n_out = SK.rotations_from_tracks(v, sk, rest, frames=frames, mean=mean, fps=FPS[rate], space=space)
        assert n_out == [SN.out_frames(n, Lf, M) for n in frames]
        assert got.dtype == np.float64 and got.shape == want.shape and np.isfinite(got).all()
        assert np.abs(got - want).max() <= 1e-15
        for b, n in enumerate(n_out):
            assert not got[b, n:].any()
    # tensors, the draws axis, a single track
    x = torch.from_numpy(np.nan_to_num(v[:2]).reshape(1, 2, 20, 3 * K))
    got = SK.rotations_from_tracks(x, sk, torch.from_numpy(rest))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == (1, 2, 20, K, 4)
    assert np.abs(got.numpy().reshape(2, 20, K, 4) - RN.rotations(np.nan_to_num(v[:2]), t, rest)).max() <= 1e-15
    one, n1 = SK.rotations_from_tracks(v[1], sk, rest, frames=7)
    assert one.shape == (20, K, 4) and n1 == [7] and not one[7:].any()


def test_refusals_by_name():
    sk = SK.ted_expressive()
    rest = rest_of("ted").astype(np.float64)
    v = np.zeros((2, 4, 126), np.float32)
    lib = L.load()
    for bad, word in ((np.nan, "not finite"), (np.inf, "not finite"), (0.0, "norm")):
        r = rest.copy()
        r[17] = [bad, 0.0, 0.0] if bad != 0.0 else [1e-7, 0.0, 0.0]
        with pytest.raises(L.EgError, match=f"rest row 17.*{word}"):
            SK.rotations_from_tracks(v, sk, r)
        assert lib.eg_skeleton_rest_check(r.ctypes.data_as(C.c_void_p), 42) != 0 and b"rest row 17" in lib.eg_last_error()
    assert lib.eg_skeleton_rest_check(rest.ctypes.data_as(C.c_void_p), 42) == 0
    assert lib.eg_skeleton_rest_check(None, 42) != 0 and b"null rest" in lib.eg_last_error()
    assert lib.eg_skeleton_rest_check(rest.ctypes.data_as(C.c_void_p), 64) != 0 and b"bones=64" in lib.eg_last_error()
    with pytest.raises(L.EgError, match=r"rest pose shape \(41, 3\).*K=42"):
        SK.rotations_from_tracks(v, sk, rest[:41])
    with pytest.raises(L.EgError, match="space='world'"):
        SK.rotations_from_tracks(v, sk, rest, space="world")
    with pytest.raises(L.EgError, match="3K=126 columns"):
        SK.rotations_from_tracks(np.zeros((4, 125), np.float32), sk, rest)
    with pytest.raises(L.EgError, match="frames has 1 entries for 2"):
        SK.rotations_from_tracks(v, sk, rest, frames=[3])
    with pytest.raises(L.EgError, match="fps"):
        SK.rotations_from_tracks(v, sk, rest, fps=(1, 65))
    with pytest.raises(L.EgError, match="rest pose of"):
        SK.rotations_from_tracks(np.zeros((4, 15), np.float32), SK.Skeleton(*SN.chain_table()), sk.rest_pose(rest))
    # the device call refuses before any launch (no GPU here): the arguments are checked in the header's order
    track = np.zeros(16 * 126, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    words = np.zeros(65 + 5 * 42, np.int32)
    aligned = track[(-track.ctypes.data % 16) // 4:]
    assert lib.eg_skeleton_rotations(ptr(aligned), 1, 4, *sk.host_ptrs(), 42, ptr(rest), ptr(words), None, 1, 1, None, 2, 1, 1, ptr(aligned), 4, None) != 0
    assert b"space=2" in lib.eg_last_error()
    r = rest.copy()
    r[3] = 0
    assert lib.eg_skeleton_rotations(ptr(aligned), 1, 4, *sk.host_ptrs(), 42, ptr(r), ptr(words), None, 1, 1, None, 0, 1, 1, ptr(aligned), 4, None) != 0
    assert b"eg_skeleton_rotations: rest row 3" in lib.eg_last_error()
    assert lib.eg_skeleton_rotations(ptr(aligned), 1, 4, *sk.host_ptrs(), 42, ptr(rest), ptr(words), None, 1, 1, None, 0, 1, 1, ptr(aligned), 3, None) != 0
    assert b"out_stride=3" in lib.eg_last_error()


def test_callers_refuse_rotations_without_joints():
    sk = SK.ted_expressive()
    rest = rest_of("ted")
    seed = torch.zeros(1, 4, 126)
    with pytest.raises(L.EgError, match="synthesize: rotations= without joints=skeleton"):
        Hs.synthesize((None, None), torch.zeros(1, 10), torch.zeros(1, 1, 60), seed, rotations=rest)
    with pytest.raises(L.EgError, match="synthesize: rotations_space without rotations=rest"):
        Hs.synthesize((None, None), torch.zeros(1, 10), torch.zeros(1, 1, 60), seed, joints=sk, rotations_space="global")
    with pytest.raises(L.EgError, match="rotations_space: space='world'"):
        Hs.synthesize((None, None), torch.zeros(1, 10), torch.zeros(1, 1, 60), seed, joints=sk, rotations=rest, rotations_space="world")
    bad = rest.copy()
    bad[2] = np.nan
    with pytest.raises(L.EgError, match="rest row 2"):
        Hs.synthesize((None, None), torch.zeros(1, 10), torch.zeros(1, 1, 60), seed, joints=sk, rotations=bad)
    with pytest.raises(L.EgError, match="GestureStream: rotations= without joints=skeleton"):
        ST.GestureStream((None, None, None), 1, seed, rotations=rest)
    with pytest.raises(L.EgError, match="joints_fps= is not supported"):
        ST.GestureStream((None, None, None), 1, seed, joints=sk, joints_fps=(15, 30), rotations=rest)
