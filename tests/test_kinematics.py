"""The motion statistics without a GPU: the host path of kinematics.kinematics_of_joints against the numpy restatement tests/kinematics_np.py
(histograms equal, means inside the bound stated there), eg_kin_edges2 bit for bit, tracks whose figures are known in closed form, the
Hellinger distance, and the refusals by name of eg_kin_edges2, eg_kin_stats (which refuses before any launch), the Python front end and the
callers."""
import ctypes as C

import numpy as np
import pytest
import torch

import kinematics_np as KN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import kinematics as KM


def figures(res):
    """The dict of kinematics_of_joints -> mean [rows, 3, J], hist [rows, J, B + 1] as numpy."""
    J = res["speed"].shape[-1]
    mean = np.stack([np.asarray(res[k], np.float64).reshape(-1, J) for k in ("speed", "accel", "jerk")], 1)
    hist = np.concatenate([np.asarray(res["speed_hist"]).reshape(-1, J, res["speed_hist"].shape[-1]),
                           np.asarray(res["speed_over"]).reshape(-1, J, 1)], 2)
    return mean, hist


def test_host_path_against_the_restatement():
    rng = np.random.default_rng(11)
    for shape, frames, fps, edges in (((70, 5, 3), None, 15, None), ((3, 40, 7, 3), [4, 17, 40], 30, np.linspace(0, 3, 13)),
                                      ((2, 3, 33, 2, 3), [33, 5], 25, [0, 0.7])):
        p = (rng.standard_normal(shape) * 0.02).astype(np.float32)
        U = 1 if frames is None else len(frames)
        R = shape[1] if len(shape) == 5 else 1
        per_row = [n for n in (frames or [shape[-3]]) for _ in range(R)]
        for u, n in enumerate(frames or []):
            p[u, ..., n:, :, :] = np.nan
        got = KM.kinematics_of_joints(p, fps, frames=frames, edges=edges)
        e = np.arange(41) / 20.0 if edges is None else np.asarray(edges, np.float64)
        assert np.array_equal(got["edges"], e) and got["edges"].dtype == np.float64
        want, count, hist = KN.stats(p.reshape((U * R,) + shape[-3:]), per_row, KN.edges2_of(e, fps), fps)
        mean, h = figures(got)
        assert got["speed"].shape == shape[:-3] + shape[-2:-1] and got["speed_hist"].shape == shape[:-3] + (shape[-2], len(e) - 1)
        assert got["speed"].dtype == np.float64 and got["speed_hist"].dtype == np.int32 and got["speed_over"].dtype == np.int32
        assert np.array_equal(h, hist)
        ok, ratio = KN.within(mean, want, count)
        assert ok, ratio
        assert np.array_equal(h.sum(-1), np.repeat(np.asarray(per_row)[:, None] - 1, shape[-2], 1))
    # a CPU tensor takes the same path and gives tensors
    t = KM.kinematics_of_joints(torch.from_numpy(p), fps, frames=frames, edges=edges)
    assert all(isinstance(t[k], torch.Tensor) for k in ("speed", "accel", "jerk", "speed_hist", "speed_over"))
    assert np.array_equal(t["jerk"].numpy(), got["jerk"]) and np.array_equal(t["speed_hist"].numpy(), got["speed_hist"])


def test_edges2_bit_for_bit_and_its_refusals():
    lib = L.load()
    for fps in (15, 30, 25, 29.97, 1):
        for edges in (np.arange(41) / 20.0, np.array([0.0, 1e-3]), np.linspace(0, 7.3, 257)):
            out = np.zeros_like(edges)
            assert lib.eg_kin_edges2(edges.ctypes.data_as(C.c_void_p), len(edges), fps, out.ctypes.data_as(C.c_void_p)) == 0
            assert np.array_equal(out, (edges / fps) ** 2) and np.array_equal(out, KN.edges2_of(edges, fps))
            assert np.array_equal(KM.SpeedBins(edges, fps).edges2, out)
    b = KM.SpeedBins()
    assert b.bins == 40 and b.fps == 15.0 and b.edges[0] == 0.0 and b.edges[-1] == 2.0 and b.edges[1] == 0.05 and b.edges.dtype == np.float64
    for edges, fps, match in (([0.0], 15, "n_edges=1"), (np.arange(258.0), 15, "n_edges=258"), ([0.1, 0.2], 15, r"edges\[0\]=0.1"),
                              ([0, 0.2, 0.2], 15, "strictly ascending"), ([0, 0.3, 0.2], 15, "strictly ascending"),
                              ([0, float("inf")], 15, "not finite"), ([0, float("nan"), 1], 15, "not finite"), ([0, 1], 0, "fps=0"),
                              ([0, 1], -15, "fps=-15"), ([0, 1], float("nan"), "fps=nan"), ([0, 1], float("inf"), "fps=inf")):
        with pytest.raises(L.EgError, match=match):
            KM.SpeedBins(edges, fps)
    assert lib.eg_kin_edges2(None, 2, 15.0, None) != 0 and b"null" in lib.eg_last_error()


def test_constant_velocity_has_no_acceleration_and_fills_one_bin():
    t = np.arange(50, dtype=np.float32)[:, None, None]
    v = np.array([[0.5, 0.25, 0.0], [0.0, 0.0, 0.0], [-0.125, 0.0, 1.0]], np.float32) / 16   # per frame; every position t * v is exact in fp32
    got = KM.kinematics_of_joints(t * v[None], 15)
    assert not got["accel"].any() and not got["jerk"].any()
    speed = 15.0 * np.sqrt((v.astype(np.float64) ** 2).sum(1))
    assert np.abs(got["speed"] - speed).max() <= 1e-14 and got["speed"][1] == 0.0
    for j in range(3):
        full = np.concatenate([got["speed_hist"][j], got["speed_over"][j:j + 1]])
        assert full.max() == 49 and full.sum() == 49
        at = int(np.argmax(full))
        assert got["edges"][at] <= speed[j] and (at == 40 or speed[j] < got["edges"][at + 1])


def test_a_parabola_has_the_acceleration_two_a_fps_squared():
    a = 0.125
    t = np.arange(40, dtype=np.float32)
    p = np.zeros((40, 2, 3), np.float32)
    p[:, 0, 0] = a * t * t
    p[:, 1, 2] = -2 * a * t * t
    got = KM.kinematics_of_joints(p, 15)
    assert np.array_equal(got["accel"], [2 * a * 225.0, 4 * a * 225.0]) and not got["jerk"].any()


def test_a_step_on_an_edge_belongs_to_the_upper_bin():
    p = np.zeros((5, 1, 3), np.float32)
    p[:, 0, 0] = [0, 0.5, 1.5, 2.0, 3.0]                                                   # steps 0.5, 1, 0.5, 1 at fps = 1
    got = KM.kinematics_of_joints(p, 1, edges=[0, 0.5, 1])
    assert got["speed_hist"].tolist() == [[0, 2]] and got["speed_over"].tolist() == [2]
    p[:, 0, 0] = [0, 0.25, 0.5, 0.75, 1.0]
    got = KM.kinematics_of_joints(p, 1, edges=[0, 0.5, 1])
    assert got["speed_hist"].tolist() == [[4, 0]] and got["speed_over"].tolist() == [0]


def test_hellinger():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 50, (3, 5, 12)), rng.integers(1, 50, (3, 5, 12))
    a[..., 0] += 1
    assert not KM.hellinger(a, a).any() and KM.hellinger(a, a).shape == (3, 5) and not KM.hellinger(a, a, pool=True).any()
    assert np.array_equal(KM.hellinger(a, b), KM.hellinger(b, a)) and ((KM.hellinger(a, b) > 0) & (KM.hellinger(a, b) < 1)).all()
    lo, hi = np.array([3, 4, 0, 0]), np.array([0, 0, 9, 1])
    assert KM.hellinger(lo, hi) == 1.0 and KM.hellinger(lo, lo) == 0.0
    pa, pb = a.sum(-2) / a.sum((-2, -1))[:, None], b.sum(-2) / b.sum((-2, -1))[:, None]
    want = np.sqrt(np.maximum(0, 1 - np.sqrt(pa * pb).sum(-1)))
    assert np.abs(KM.hellinger(a, b, pool=True) - want).max() <= 1e-12 and KM.hellinger(a, b, pool=True).shape == (3,)
    t = KM.hellinger(torch.from_numpy(a), torch.from_numpy(b))
    assert t.dtype == torch.float64 and np.abs(t.numpy() - KM.hellinger(a, b)).max() <= 1e-12
    empty = a.copy()
    empty[1, 2] = 0
    with pytest.raises(L.EgError, match="hist_b holds an empty histogram"):
        KM.hellinger(a, empty)
    with pytest.raises(L.EgError, match="hist_a holds an empty histogram"):
        KM.hellinger(empty, a)
    assert KM.hellinger(empty, a, pool=True).shape == (3,)
    with pytest.raises(L.EgError, match="need one shape"):
        KM.hellinger(a, b[..., :5])


def test_front_end_refusals_by_name():
    with pytest.raises(L.EgError, match="recording 1 has 3 valid frames < 4"):
        KM.kinematics_of_joints(np.zeros((2, 20, 5, 3), np.float32), 15, frames=[20, 3])
    with pytest.raises(L.EgError, match="recording 0 has 3 valid frames < 4"):
        KM.kinematics_of_joints(torch.zeros(3, 5, 3), 15)
    with pytest.raises(L.EgError, match="frames has 1 entries for 2"):
        KM.kinematics_of_joints(np.zeros((2, 20, 5, 3), np.float32), 15, frames=[20])
    with pytest.raises(L.EgError, match="at most two leading axes"):
        KM.kinematics_of_joints(np.zeros((1, 1, 1, 20, 5, 3), np.float32), 15)
    with pytest.raises(L.EgError, match=r"need \[\.\.\., T, J, 3\]"):
        KM.kinematics_of_joints(np.zeros((20, 5, 4), np.float32), 15)
    with pytest.raises(L.EgError, match=r"need \[\.\.\., T, J, 3\]"):
        KM.kinematics_of_joints(np.zeros((20, 65, 3), np.float32), 15)
    with pytest.raises(L.EgError, match="SpeedBins are at fps=30, the joints at fps=15"):
        KM.kinematics_of_joints(np.zeros((20, 5, 3), np.float32), 15, edges=KM.SpeedBins(fps=30))
    with pytest.raises(L.EgError, match="fps=0"):
        KM.kinematics_of_joints(np.zeros((20, 5, 3), np.float32), 0)


def test_eg_kin_stats_refuses_before_any_launch():
    """No GPU here and none needed: every refusal returns before the first launch (the addresses are never touched)."""
    lib = L.load()
    P = C.c_void_p
    frames = (C.c_int32 * 2)(20, 3)
    ok = dict(joints=P(1 << 20), rows=2, T=20, J=5, frames=None, d_frames=None, draws=1, unit=1, fps=15.0, edges2=P(1 << 16), bins=40,
              ws=P(1 << 24), ws_bytes=1 << 20, mean=P(1 << 26), hist=P(1 << 28))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.eg_kin_stats(a["joints"], a["rows"], a["T"], a["J"], a["frames"], a["d_frames"], a["draws"], a["unit"], a["fps"], a["edges2"],
                              a["bins"], a["ws"], a["ws_bytes"], a["mean"], a["hist"], None)
        return rc, lib.eg_last_error().decode()

    for kw, word in [(dict(joints=None), "null joints"), (dict(edges2=None), "null d_edges2"), (dict(ws=None), "null workspace"),
                     (dict(mean=None), "null mean"), (dict(hist=None), "null hist"), (dict(joints=P((1 << 20) + 4)), "16-byte"),
                     (dict(ws=P((1 << 24) + 8)), "16-byte"), (dict(mean=P((1 << 26) + 8)), "16-byte"), (dict(hist=P((1 << 28) + 4)), "16-byte"),
                     (dict(rows=0), "rows=0"), (dict(T=3), "frames=3"), (dict(J=0), "joints=0"), (dict(J=65), "joints=65"),
                     (dict(bins=0), "bins=0"), (dict(bins=257), "bins=257"), (dict(rows=3, draws=2), "multiple of draws"),
                     (dict(unit=0), "frame_unit"), (dict(fps=0.0), "fps=0"), (dict(fps=float("nan")), "fps=nan"),
                     (dict(fps=float("inf")), "fps=inf"), (dict(fps=-15.0), "fps=-15"),
                     (dict(frames=frames, d_frames=P(1 << 12)), "recording 1 has 3 valid frames < 4"), (dict(frames=frames), "go together"),
                     (dict(d_frames=P(1 << 12)), "go together"), (dict(ws_bytes=8 * 2 * 1 * 3 * 5 - 1), "workspace of 239 bytes, need 240"),
                     (dict(rows=1 << 20, T=1 << 20, J=4), "index range")]:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    TF = KM.TILE_FRAMES
    assert lib.eg_kin_tile_frames() == TF == L.EG_KIN_TILE_FRAMES == 64 and (KM.MAX_JOINTS, KM.MAX_BINS) == (64, 256)
    assert lib.eg_kin_workspace_bytes(2, 20, 5, 40) == 8 * 2 * 1 * 3 * 5
    assert lib.eg_kin_workspace_bytes(3, TF + 1, 43, 1) == 8 * 3 * 1 * 3 * 43 and lib.eg_kin_workspace_bytes(3, TF + 2, 43, 1) == 8 * 3 * 2 * 3 * 43
    assert 8 * 3 * 2 * 3 * 43 < 4 * 3 * (TF + 2) * 43 * 3                          # the workspace stays below the size of the input
    for bad in ((0, 20, 5, 40), (2, 3, 5, 40), (2, 20, 0, 40), (2, 20, 65, 40), (2, 20, 5, 0), (2, 20, 5, 257)):
        assert lib.eg_kin_workspace_bytes(*bad) == 0


def test_callers_refuse_kinematics_without_joints_before_anything_runs():
    from emotiongestures_amd import harness as Hs
    with pytest.raises(L.EgError, match="synthesize: kinematics= without joints="):
        Hs.synthesize((None, None), torch.zeros(2, 1000), torch.zeros(2, 1, 60), torch.zeros(2, 4, 126), kinematics=True)
    with pytest.raises(L.EgError, match="synthesize_takes: kinematics= without joints="):
        Hs.synthesize_takes((None, None), torch.zeros(2, 1000), torch.zeros(2, 1, 60), torch.zeros(2, 4, 126), draws=2, kinematics=[0, 1, 2])
    from emotiongestures_amd import skeleton as SK
    with pytest.raises(L.EgError, match="strictly ascending"):
        Hs.synthesize((None, None), torch.zeros(2, 1000), torch.zeros(2, 1, 60), torch.zeros(2, 4, 126), joints=SK.ted_expressive(),
                      kinematics=[0, 2, 1])
    with pytest.raises(L.EgError, match="SpeedBins are at fps=15, the joints at fps=30"):
        Hs.synthesize((None, None), torch.zeros(2, 1000), torch.zeros(2, 1, 60), torch.zeros(2, 4, 126), joints=SK.ted_expressive(),
                      joints_fps=(15, 30), kinematics=KM.SpeedBins())
