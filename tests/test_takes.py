"""Take diversity, CPU side: the meta table (a host function of the library) against its numpy restatement, the workspace size (0 for every
refused argument), the C ABI's refusals by name before any device use, the restatement against harness.calculate_diversity, and the Python
surface's refusals.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import takes_np as T
from conftest import build_mirror
from emotiongestures_amd import _lib as L

NEW_SYMBOLS = ("eg_take_meta_ints", "eg_take_meta", "eg_track_rows_pack", "eg_take_distance_workspace_bytes", "eg_take_distance")


def _i32(v):
    a = np.ascontiguousarray(v, np.int32)
    return a, C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("frames", [[9, 4, 1], [5], [7, 7, 7, 7], [54000, 1, 9000]])
def test_meta_table_equals_numpy_restatement(frames):
    lib = L.load()
    U = len(frames)
    n = lib.eg_take_meta_ints(U)
    assert n == 2 * U
    meta = np.full(n, -7, np.int32)
    _f, pf = _i32(frames)
    L.check(lib.eg_take_meta(pf, U, C.c_void_p(meta.ctypes.data)), "eg_take_meta")
    assert np.array_equal(meta, T.meta_np(frames))
    # the packed order the table stands for: row R*off[u] + r*frames[u] + t holds pose (u, r, t)
    R = 3
    u, r, t = T.packed_index(frames, R)
    rows = R * meta[U + u].astype(np.int64) + r * meta[u].astype(np.int64) + t
    assert np.array_equal(rows, np.arange(R * sum(frames)))


def test_meta_ints_and_meta_refusals():
    lib = L.load()
    assert lib.eg_take_meta_ints(0) == 0 and lib.eg_take_meta_ints(-3) == 0 and lib.eg_take_meta_ints(65536) == 0
    assert lib.eg_take_meta_ints(65535) == 2 * 65535
    meta = np.zeros(64, np.int32)
    pm = C.c_void_p(meta.ctypes.data)
    _f, pf = _i32([9, 0, 1])
    assert lib.eg_take_meta(pf, 3, pm) != 0 and "eg_take_meta: frames[1]=0" in lib.eg_last_error().decode()
    _g, pg = _i32([9, 4, 1])
    assert lib.eg_take_meta(pg, 0, pm) != 0 and "U=0" in lib.eg_last_error().decode()
    assert lib.eg_take_meta(None, 3, pm) != 0 and "null frames" in lib.eg_last_error().decode()
    assert lib.eg_take_meta(pg, 3, None) != 0 and "null meta" in lib.eg_last_error().decode()
    big = np.full(3, 2 ** 30, np.int32)
    assert lib.eg_take_meta(C.c_void_p(big.ctypes.data), 3, pm) != 0 and "index range" in lib.eg_last_error().decode()


def test_workspace_is_positive_for_valid_and_zero_for_every_refused_argument():
    lib = L.load()
    _f, pf = _i32([70, 34, 5, 1])
    chunk = 16                                                                  # EG_TAKE_CHUNK_FRAMES
    chunks = sum(-(-f // chunk) for f in [70, 34, 5, 1])
    for R in (2, 3, 5, 64):
        got = lib.eg_take_distance_workspace_bytes(pf, 4, R)
        assert got >= chunks * (R * (R - 1) // 2) * 8, (R, got)                  # one fp64 partial per (chunk, pair) at least
    assert lib.eg_take_distance_workspace_bytes(pf, 4, 5) > lib.eg_take_distance_workspace_bytes(pf, 4, 3)
    bad = [(None, 4, 3),                                                        # null frames
           (pf, 0, 3), (pf, -1, 3), (pf, 70000, 3),                             # U
           (pf, 4, 1), (pf, 4, 0), (pf, 4, -2), (pf, 4, 65),                    # draws: 2..64
           (_i32([70, 0, 5, 1])[1], 4, 3), (_i32([70, 34, -5, 1])[1], 4, 3)]    # frames[u] < 1
    for args in bad:
        assert lib.eg_take_distance_workspace_bytes(*args) == 0, args


def _pack(lib, **over):
    """eg_track_rows_pack with dummy non-null pointers: every refusal comes before the launch, so nothing is dereferenced."""
    frames = over.pop("frames", [9, 4, 1])
    keep = None if frames is None else _i32(frames)
    dummy = C.c_void_p(256)
    a = dict(track=dummy, U=3, R=3, Tmax=9, D=282, frames=None if keep is None else keep[1], d_meta=dummy, rows=dummy, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    rc = lib.eg_track_rows_pack(*a.values())
    return rc, lib.eg_last_error().decode()


def _dist(lib, **over):
    frames = over.pop("frames", [9, 4, 1])
    keep = None if frames is None else _i32(frames)
    dummy = C.c_void_p(256)
    a = dict(feat=dummy, U=3, R=3, K=512, frames=None if keep is None else keep[1], d_meta=dummy, span=0, ws=dummy, ws_bytes=1 << 40,
             distance=dummy, diversity=dummy, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    rc = lib.eg_take_distance(*a.values())
    return rc, lib.eg_last_error().decode()


PACK_REFUSALS = [
    (dict(track=None), "null track"), (dict(d_meta=None), "null d_meta"), (dict(rows=None), "null rows"), (dict(frames=None), "null frames"),
    (dict(rows=C.c_void_p(264)), "rows not 16-byte aligned"),
    (dict(U=0), "U=0"), (dict(U=-1), "U=-1"), (dict(U=65536), "U=65536"),
    (dict(R=0), "draws=0"), (dict(R=65), "draws=65"),
    (dict(Tmax=0), "Tmax=0"), (dict(D=0), "pose_dim=0"),
    (dict(frames=[9, 0, 1]), "frames[1]=0"), (dict(frames=[10, 4, 1]), "frames[0]=10 (1..Tmax=9)"),
    (dict(frames=[2 ** 30] * 3, Tmax=2 ** 30, R=64), "index range"),
]
DIST_REFUSALS = [
    (dict(feat=None), "null feat"), (dict(d_meta=None), "null d_meta"), (dict(ws=None), "null workspace"),
    (dict(distance=None), "null distance"), (dict(diversity=None), "null diversity"), (dict(frames=None), "null frames"),
    (dict(feat=C.c_void_p(260)), "feat not 16-byte aligned"), (dict(ws=C.c_void_p(264)), "workspace not 16-byte aligned"),
    (dict(distance=C.c_void_p(264)), "distance not 16-byte aligned"), (dict(diversity=C.c_void_p(264)), "diversity not 16-byte aligned"),
    (dict(U=0), "U=0"), (dict(U=65536), "U=65536"),
    (dict(R=1), "draws=1"), (dict(R=0), "draws=0"), (dict(R=65), "draws=65"),
    (dict(frames=[9, 4, 0]), "frames[2]=0"),
    (dict(K=510), "feat_dim=510"), (dict(K=0), "feat_dim=0"),
    (dict(frames=[2 ** 29] * 3, R=64), "N*K"),                                  # N*K = 64 * 3 * 2^29 * 512 >= 2^40
    (dict(ws_bytes=16), "workspace too small"),
]


@pytest.mark.parametrize("over,needle", PACK_REFUSALS, ids=[f"{list(o)[0]}-{n}" for o, n in PACK_REFUSALS])
def test_pack_refuses_by_name_before_any_device_use(over, needle):
    lib = L.load()
    before = lib.eg_launch_count()
    rc, msg = _pack(lib, **over)
    assert rc != 0 and "eg_track_rows_pack" in msg and needle in msg, (rc, msg)
    assert lib.eg_launch_count() == before


@pytest.mark.parametrize("over,needle", DIST_REFUSALS, ids=[f"{list(o)[0]}-{n}" for o, n in DIST_REFUSALS])
def test_distance_refuses_by_name_before_any_device_use(over, needle):
    lib = L.load()
    before = lib.eg_launch_count()
    rc, msg = _dist(lib, **over)
    assert rc != 0 and "eg_take_distance" in msg and needle in msg, (rc, msg)
    assert lib.eg_launch_count() == before


def test_restatement_is_the_pair_distance_inside_calculate_diversity():
    """With frames == span the restated distance is np.sqrt(((a - b) ** 2).sum()) on the same activations: the expression inside
    harness.calculate_diversity (model/FHD_score.py:270-286), which is called here with one random pair whose indices the seed fixes."""
    from emotiongestures_amd import harness as H
    rng = np.random.default_rng(11)
    R, F = 5, 60
    feat = (rng.standard_normal((R * F, 512)) * 8).astype(np.float32)
    dist, div = T.take_distance_np(feat, [F], R, span=F)
    raw, _ = T.take_distance_np(feat, [F], R)
    assert np.array_equal(dist, raw)                                            # scale = span / frames = 1.0 exactly
    act = feat.astype(np.float64).reshape(R, F, 512)                            # what harness.evaluate hands to diversity_score
    for r in range(R):
        for rp in range(R):
            assert dist[0, r, rp] == np.sqrt(((act[r] - act[rp]) ** 2).sum())
    seen = set()
    for seed in range(8):
        np.random.seed(seed)
        i, j = int(np.random.randint(0, R, 1)[0]), int(np.random.randint(0, R, 1)[0])
        np.random.seed(seed)
        got = H.calculate_diversity(act, act, diversity_times=1)
        assert got == np.float32(dist[0, i, j]), (seed, i, j)
        seen.add(i != j)
    assert True in seen
    pairs = [dist[0, r, rp] for r in range(R) for rp in range(r + 1, R)]
    assert np.isclose(div[0], np.mean(pairs), rtol=1e-15)
    # span brings a longer recording to the clip's unit: twice the frames of the same per-frame distance -> the same figure
    both = np.concatenate([act, act], axis=1).reshape(R * 2 * F, 512).astype(np.float32)
    d2, _ = T.take_distance_np(both, [2 * F], R, span=F)
    assert np.allclose(d2, dist, rtol=1e-14)


def test_python_surface_refusals():
    from emotiongestures_amd import harness as H
    from emotiongestures_amd import takes
    gen = build_mirror("spatial", 34, 126, 4, 4, seed=3).eval()
    fgd = H.MLP_Reconstruct(pose_dim=126).eval()
    args = (torch.zeros(1, 64000), torch.zeros(1, 2, 60, dtype=torch.long), torch.zeros(1, 4, 126))
    with pytest.raises(L.EgError, match=re.escape("diversity= needs draws >= 2")):
        H.synthesize((gen, None), *args, diversity=fgd)
    with pytest.raises(L.EgError, match=re.escape("diversity= needs draws >= 2 (got draws=1)")):
        H.synthesize((gen, object()), *args, draws=1, diversity=fgd)
    with pytest.raises(L.EgError, match=re.escape("draws=1: a distance between takes needs draws >= 2")):
        takes.take_distance(torch.zeros(9, 512), [9], 1)
    with pytest.raises(L.EgError, match="draws=65"):
        takes.take_distance(torch.zeros(9, 512), [9], 65)
    with pytest.raises(RuntimeError, match="feat must be a CUDA tensor"):
        takes.take_distance(torch.zeros(18, 512), [9], 2)
    with pytest.raises(RuntimeError, match="track must be a CUDA tensor"):
        takes.track_features(fgd, torch.zeros(1, 2, 9, 126))
    with pytest.raises(L.EgError, match="R >= 2 takes per recording"):
        takes.take_diversity(fgd, torch.zeros(1, 9, 126))
    assert H.take_diversity.__doc__ and H.track_features.__doc__ and H.take_distance.__doc__
    for name in ("track_features", "take_distance", "take_diversity"):
        assert name in H.__all__


def test_new_symbols_are_declared_and_bound():
    import os
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"#define EG_TAKE_CHUNK_FRAMES 16\b", header)
