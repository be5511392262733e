"""SRGR and L1 diversity without a GPU: the host path of jointscore.srgr_of_joints / l1div_of_tracks and the classes SRGR / L1div against the
reference's own figures (tests/golden/jointscore.npz, from tests/golden/make_golden_jointscore.py) and against the numpy restatement
tests/jointscore_np.py; the threshold edge, ragged rows, takes that share a target, and every refusal by name -- of eg_srgr_tracks and
eg_l1div_tracks (which refuse before any launch), of the Python front end, of SemanticTargets and of the callers' arguments."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import jointscore_np as JN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import jointscore as JS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jointscore.npz")
SHAPES = [(37, 47), (5, 1), (70, 43), (9, 64)]


def rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def test_golden_masks_rates_and_pooled_averages_are_the_reference_s():
    z = np.load(GOLDEN)
    assert [tuple(s) for s in z["shapes"].tolist()] == SHAPES and float(z["threshold"]) == 0.1 and float(z["margin"]) > 1e-6
    pool_s, pool_l = JS.SRGR(threshold=0.1), JS.L1div()
    for n, J in SHAPES:
        tag = f"{n}x{J}"
        result, target, sem, mask = z[f"{tag}/result"], z[f"{tag}/target"], z[f"{tag}/semantic"], z[f"{tag}/mask"].astype(bool)
        assert result.dtype == np.float32 and result.shape == (n, J, 3) and not sem[::3].any() and sem[1] > 0
        assert np.array_equal(JN.distance(result, target) < 0.1, mask)                   # the fp32 subtraction changes no cell
        got = JS.srgr_of_joints(result, target, sem)
        assert got["hits"].dtype == np.int32 and np.array_equal(got["hits"], mask.sum(0)) and int(got["frames"]) == n
        assert float(got["recall"]) == mask.sum() / (n * J)
        assert rel(got["srgr"], z[f"{tag}/rate"]) <= 1e-14, tag
        l1 = JS.l1div_of_tracks(result.reshape(n, J * 3))
        assert rel(l1["l1div"], z[f"{tag}/l1div"]) <= 1e-14 and rel(l1["l1_sum"], z[f"{tag}/l1_sum"]) <= 1e-14, tag
        assert l1["mean"].shape == (J * 3,) and l1["mean"].dtype == np.float64
        # the classes, fed as upstream feeds them: flat float64 rows; one SRGR object over the four joint counts, as the golden pooled them
        pool_s.pose_dimes = J
        rate = pool_s.run(result.astype(np.float64).reshape(n, J * 3), target.astype(np.float64).reshape(n, J * 3), sem.astype(np.float64))
        assert rate == float(got["srgr"])
        pool_l.run(result.astype(np.float64).reshape(n, J * 3))
    assert pool_s.counter == int(z["pool/srgr_counter"]) == sum(n for n, _ in SHAPES) and pool_l.counter == int(z["pool/l1_counter"])
    assert rel(pool_s.avg(), z["pool/srgr_avg"]) <= 1e-14 and rel(pool_s.sum, z["pool/srgr_sum"]) <= 1e-14
    assert rel(pool_l.avg(), z["pool/l1_avg"]) <= 1e-14 and rel(pool_l.sum, z["pool/l1_sum"]) <= 1e-14


def test_run_leaves_its_arguments_unchanged_and_push_pools_dicts():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((12, 141))
    g = x + rng.standard_normal((12, 141)) * 0.04
    w = rng.random(12)
    keep = [a.copy() for a in (x, g, w)]
    s, d = JS.SRGR(), JS.L1div()
    s.run(x, g, w)
    d.run(x)
    assert all(np.array_equal(a, b) for a, b in zip((x, g, w), keep))
    xt = torch.from_numpy(x.astype(np.float32))
    d.run(xt)
    assert torch.equal(xt, torch.from_numpy(x.astype(np.float32))) and d.counter == 24
    # push: rows of unequal length are weighted by their own frames
    p = rng.standard_normal((2, 9, 5, 3)).astype(np.float32)
    q = (p + rng.standard_normal(p.shape) * 0.05).astype(np.float32)
    res = JS.srgr_of_joints(p, q, frames=[9, 4])
    s2 = JS.SRGR(joints=5)
    s2.push(res)
    assert s2.counter == 13 and s2.avg() == (float(res["srgr"][0]) * 9 + float(res["srgr"][1]) * 4) / 13
    d2 = JS.L1div()
    l1 = JS.l1div_of_tracks(p.reshape(2, 9, 15), frames=[9, 4])
    d2.push(l1)
    assert d2.counter == 13 and d2.avg() == (float(l1["l1_sum"][0]) + float(l1["l1_sum"][1])) / 13


def test_a_distance_equal_to_the_threshold_is_a_miss():
    r = np.array([[[0.0625, 0.03125, 0.0]]], np.float32)
    g = np.zeros_like(r)
    miss = JS.srgr_of_joints(r, g, threshold=0.09375)
    hit = JS.srgr_of_joints(r, g, threshold=float(np.nextafter(0.09375, 1)))
    assert miss["hits"].tolist() == [0] and float(miss["srgr"]) == 0.0 and float(miss["recall"]) == 0.0
    assert hit["hits"].tolist() == [1] and float(hit["recall"]) == 1.0 and float(hit["srgr"]) == 1 / 0.165
    nan = JS.srgr_of_joints(np.full_like(r, np.nan), g, threshold=1e9)
    assert nan["hits"].tolist() == [0]                                                  # a NaN is a miss, as in numpy


def test_ragged_rows_with_nan_behind_their_frames_and_takes_that_share_a_target():
    rng = np.random.default_rng(5)
    U, R, T, J = 3, 2, 41, 7
    g = rng.standard_normal((U, T, J, 3)).astype(np.float32)
    r = (g[:, None] + rng.standard_normal((U, R, T, J, 3)) * 0.04).astype(np.float32)
    w = (rng.random((U, T)) - 0.3).astype(np.float32)
    frames = [41, 1, 33]
    for u, n in enumerate(frames):
        r[u, :, n:] = np.nan
        g[u, n:] = np.nan
        w[u, n:] = np.nan
    got = JS.srgr_of_joints(r, g, w, frames=frames, threshold=0.1, scale=2.5)
    per = [n for n in frames for _ in range(R)]
    hits, want, bound, recall = JN.srgr(r.reshape(U * R, T, J, 3), g, w, per, R, 0.1, 2.5)
    assert got["srgr"].shape == (U, R) and got["hits"].shape == (U, R, J) and got["frames"].tolist() == [[41, 41], [1, 1], [33, 33]]
    assert np.array_equal(got["hits"].reshape(U * R, J), hits) and np.array_equal(got["recall"].reshape(-1), recall)
    assert (np.abs(got["srgr"].reshape(-1) - want) <= bound).all() and np.isfinite(got["srgr"]).all() and hits.sum() > 0
    # every take alone against its recording's target gives the take's own row
    for u in range(U):
        for k in range(R):
            one = JS.srgr_of_joints(r[u, k], g[u], w[u], frames=frames[u], scale=2.5)
            assert one["srgr"] == got["srgr"][u, k] and np.array_equal(one["hits"], got["hits"][u, k])
    x = r.reshape(U, R, T, J * 3)
    l1 = JS.l1div_of_tracks(x, frames=frames)
    mean, mean_bound, s, s_bound = JN.l1div(x.reshape(U * R, T, J * 3), per)
    assert l1["l1div"].shape == (U, R) and l1["mean"].shape == (U, R, J * 3) and np.isfinite(l1["l1_sum"]).all()
    assert (np.abs(l1["mean"].reshape(U * R, -1) - mean) <= mean_bound).all()
    assert (np.abs(l1["l1_sum"].reshape(-1) - s) <= s_bound).all()
    assert np.array_equal(l1["l1div"], l1["l1_sum"] / np.asarray(per, np.float64).reshape(U, R))
    assert not l1["l1_sum"][1].any()                                                    # one frame: it is its own mean
    # a CPU tensor takes the same path and gives tensors
    t = JS.srgr_of_joints(torch.from_numpy(r), torch.from_numpy(g), torch.from_numpy(w), frames=frames, scale=2.5)
    assert isinstance(t["srgr"], torch.Tensor) and np.array_equal(t["srgr"].numpy(), got["srgr"]) and np.array_equal(t["hits"].numpy(), got["hits"])
    tl = JS.l1div_of_tracks(torch.from_numpy(x), frames=frames)
    assert isinstance(tl["mean"], torch.Tensor) and np.array_equal(tl["l1_sum"].numpy(), l1["l1_sum"])


def test_front_end_refusals_by_name():
    p = np.zeros((2, 20, 5, 3), np.float32)
    for call, match in (
            (lambda: JS.srgr_of_joints(p, p[:1]), "targets shape"),
            (lambda: JS.srgr_of_joints(np.zeros((2, 3, 20, 5, 3), np.float32), np.zeros((2, 3, 20, 5, 3), np.float32)), "one target per recording"),
            (lambda: JS.srgr_of_joints(p, p, np.zeros((2, 19), np.float32)), "semantic shape"),
            (lambda: JS.srgr_of_joints(p, p, frames=[20, 0]), "recording 1 has 0 valid frames < 1"),
            (lambda: JS.srgr_of_joints(p, p, frames=[20]), "frames has 1 entries for 2"),
            (lambda: JS.srgr_of_joints(p, p, frames=[20, 21]), r"every value must be in \[0, 20\]"),
            (lambda: JS.srgr_of_joints(np.zeros((1, 1, 1, 20, 5, 3), np.float32), p), "at most two leading axes"),
            (lambda: JS.srgr_of_joints(np.zeros((20, 5, 4), np.float32), p), r"need \[\.\.\., T >= 1, J, 3\]"),
            (lambda: JS.srgr_of_joints(np.zeros((20, 65, 3), np.float32), p), r"need \[\.\.\., T >= 1, J, 3\]"),
            (lambda: JS.srgr_of_joints(p, p, threshold=float("nan")), "threshold=nan is not finite"),
            (lambda: JS.srgr_of_joints(p, p, scale=float("inf")), "scale=inf is not finite"),
            (lambda: JS.l1div_of_tracks(np.zeros((4, JS.MAX_COLS + 1), np.float32)), r"need \[\.\.\., T >= 1, D\]"),
            (lambda: JS.l1div_of_tracks(np.zeros((0, 4), np.float32)), r"need \[\.\.\., T >= 1, D\]"),
            (lambda: JS.l1div_of_tracks(np.zeros((1, 1, 1, 4, 4), np.float32)), "at most two leading axes"),
            (lambda: JS.l1div_of_tracks(np.zeros((2, 9, 4), np.float32), frames=[0, 9]), "recording 0 has 0 valid frames < 1"),
            (lambda: JS.SemanticTargets(np.zeros((20, 5, 3), np.float32)), r"need \[U, T', J, 3\]"),
            (lambda: JS.SemanticTargets(p, np.zeros((2, 21), np.float32)), "semantic shape"),
            (lambda: JS.SemanticTargets(p, threshold=float("inf")), "threshold=inf is not finite"),
            (lambda: JS.SemanticTargets(p).fit("caller", U=3), "U=2, the call's joints have U=3"),
            (lambda: JS.SemanticTargets(p).fit("caller", U=2, T=21), "T'=20, the call's joints have T'=21"),
            (lambda: JS.SemanticTargets(p).fit("caller", J=43), "J=5, the call's joints have J=43")):
        with pytest.raises(L.EgError, match=match):
            call()
    assert JS.SemanticTargets(p, np.zeros((2, 20)), 0.2).fit("caller", 2, 20, 5).threshold == 0.2


def test_eg_srgr_and_l1div_refuse_before_any_launch():
    """No GPU here and none needed: every refusal returns before the first launch (the addresses are never touched)."""
    lib = L.load()
    P = C.c_void_p
    frames = (C.c_int32 * 2)(20, 0)
    TF = lib.eg_jointscore_tile_frames()
    assert TF == L.EG_JOINTSCORE_TILE_FRAMES == JS.TILE_FRAMES and JS.MAX_JOINTS == 64 and JS.MAX_COLS >= 282 and JS.MAX_COLS >= 3 * 64
    ok = dict(r=P(1 << 20), g=P(1 << 22), w=P(1 << 18), rows=2, T=20, J=5, frames=None, d_frames=None, draws=1, unit=1, thr=0.1, scale=1.0,
              ws=P(1 << 24), ws_bytes=1 << 20, srgr=P(1 << 26), recall=P(1 << 27), hits=P(1 << 28))

    def srgr(**kw):
        a = dict(ok, **kw)
        rc = lib.eg_srgr_tracks(a["r"], a["g"], a["w"], a["rows"], a["T"], a["J"], a["frames"], a["d_frames"], a["draws"], a["unit"], a["thr"],
                                a["scale"], a["ws"], a["ws_bytes"], a["srgr"], a["recall"], a["hits"], None)
        return rc, lib.eg_last_error().decode()

    need = (8 + 4 * 5) * 2 * 1
    for kw, word in [(dict(r=None), "null results"), (dict(g=None), "null targets"), (dict(ws=None), "null workspace"),
                     (dict(srgr=None), "null srgr"), (dict(recall=None), "null recall"), (dict(hits=None), "null hits"),
                     (dict(r=P((1 << 20) + 4)), "16-byte"), (dict(g=P((1 << 22) + 8)), "16-byte"), (dict(ws=P((1 << 24) + 8)), "16-byte"),
                     (dict(srgr=P((1 << 26) + 4)), "8-byte"), (dict(recall=P((1 << 27) + 4)), "8-byte"), (dict(hits=P((1 << 28) + 2)), "4-byte"),
                     (dict(w=P((1 << 18) + 2)), "4-byte"), (dict(rows=0), "rows=0"), (dict(T=0), "frames=0"), (dict(J=0), "joints=0"),
                     (dict(J=65), "joints=65"), (dict(rows=3, draws=2), "multiple of draws"), (dict(draws=0), "multiple of draws"),
                     (dict(unit=0), "frame_unit"), (dict(thr=float("nan")), "threshold=nan"), (dict(thr=float("inf")), "threshold=inf"),
                     (dict(scale=float("nan")), "scale=nan"), (dict(scale=float("-inf")), "scale=-inf"),
                     (dict(frames=frames, d_frames=P(1 << 12)), "recording 1 has 0 valid frames < 1"), (dict(frames=frames), "go together"),
                     (dict(d_frames=P(1 << 12)), "go together"), (dict(ws_bytes=need - 1), f"workspace of {need - 1} bytes, need {need}"),
                     (dict(rows=1 << 20, T=1 << 20, J=4), "index range")]:
        rc, msg = srgr(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert lib.eg_srgr_workspace_bytes(2, 20, 5) == need
    assert lib.eg_srgr_workspace_bytes(3, TF, 43) == (8 + 4 * 43) * 3 and lib.eg_srgr_workspace_bytes(3, TF + 1, 43) == (8 + 4 * 43) * 3 * 2
    for bad in ((0, 20, 5), (2, 0, 5), (2, 20, 0), (2, 20, 65)):
        assert lib.eg_srgr_workspace_bytes(*bad) == 0

    ok = dict(x=P(1 << 20), rows=2, T=20, D=15, frames=None, d_frames=None, draws=1, unit=1, ws=P(1 << 24), ws_bytes=1 << 20, mean=P(1 << 26),
              l1_sum=P(1 << 27), l1div=P(1 << 28))

    def l1(**kw):
        a = dict(ok, **kw)
        rc = lib.eg_l1div_tracks(a["x"], a["rows"], a["T"], a["D"], a["frames"], a["d_frames"], a["draws"], a["unit"], a["ws"], a["ws_bytes"],
                                 a["mean"], a["l1_sum"], a["l1div"], None)
        return rc, lib.eg_last_error().decode()

    need = 8 * 2 * 1 * 16
    for kw, word in [(dict(x=None), "null x"), (dict(ws=None), "null workspace"), (dict(mean=None), "null mean"), (dict(l1_sum=None), "null l1_sum"),
                     (dict(l1div=None), "null l1div"), (dict(x=P((1 << 20) + 4)), "16-byte"), (dict(ws=P((1 << 24) + 8)), "16-byte"),
                     (dict(mean=P((1 << 26) + 4)), "8-byte"), (dict(l1_sum=P((1 << 27) + 4)), "8-byte"), (dict(l1div=P((1 << 28) + 4)), "8-byte"),
                     (dict(rows=0), "rows=0"), (dict(T=0), "frames=0"), (dict(D=0), "columns=0"), (dict(D=JS.MAX_COLS + 1), f"columns={JS.MAX_COLS + 1}"),
                     (dict(rows=3, draws=2), "multiple of draws"), (dict(unit=0), "frame_unit"),
                     (dict(frames=frames, d_frames=P(1 << 12)), "recording 1 has 0 valid frames < 1"), (dict(frames=frames), "go together"),
                     (dict(d_frames=P(1 << 12)), "go together"), (dict(ws_bytes=need - 1), f"workspace of {need - 1} bytes, need {need}"),
                     (dict(rows=1 << 20, T=1 << 20, D=4), "index range")]:
        rc, msg = l1(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert lib.eg_l1div_workspace_bytes(2, 20, 15) == need and lib.eg_l1div_workspace_bytes(3, TF + 1, 282) == 8 * 3 * 2 * 283
    assert 8 * 3 * 2 * 283 < 4 * 3 * (TF + 1) * 282                               # the workspace stays below the size of the input
    for bad in ((0, 20, 5), (2, 0, 5), (2, 20, 0), (2, 20, JS.MAX_COLS + 1)):
        assert lib.eg_l1div_workspace_bytes(*bad) == 0


def test_callers_refuse_the_two_arguments_before_anything_runs():
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd import skeleton as SK
    sk = SK.ted_expressive()
    args = ((None, None), torch.zeros(2, 1000), torch.zeros(2, 1, 60), torch.zeros(2, 4, 126))
    targets = JS.SemanticTargets(np.zeros((2, 34, sk.J, 3), np.float32))
    with pytest.raises(L.EgError, match="synthesize: srgr= without joints="):
        Hs.synthesize(*args, srgr=targets)
    with pytest.raises(L.EgError, match="synthesize: l1div= without joints="):
        Hs.synthesize(*args, l1div=True)
    with pytest.raises(L.EgError, match="synthesize_takes: srgr= without joints="):
        Hs.synthesize_takes(*args, draws=2, srgr=targets)
    with pytest.raises(L.EgError, match="synthesize_takes: l1div= without joints="):
        Hs.synthesize_takes(*args, draws=2, l1div=True)
    with pytest.raises(L.EgError, match="srgr= takes a jointscore.SemanticTargets, got ndarray"):
        Hs.synthesize(*args, joints=sk, srgr=np.zeros((2, 34, sk.J, 3), np.float32))
    with pytest.raises(L.EgError, match="l1div= takes True, got str"):
        Hs.synthesize(*args, joints=sk, l1div="yes")
    with pytest.raises(L.EgError, match="synthesize: srgr=: the targets .* have U=3, the call's joints have U=2"):
        Hs.synthesize(*args, joints=sk, srgr=JS.SemanticTargets(np.zeros((3, 34, sk.J, 3), np.float32)))
    with pytest.raises(L.EgError, match=f"synthesize_takes: srgr=: the targets .* have J=5, the call's joints have J={sk.J}"):
        Hs.synthesize_takes(*args, draws=2, joints=sk, srgr=JS.SemanticTargets(np.zeros((2, 34, 5, 3), np.float32)))


def test_the_beat_module_s_stubs_still_refuse_and_name_this_module():
    from emotiongestures_amd import beat
    for name in ("SRGR", "L1div"):
        with pytest.raises(NotImplementedError, match=f"jointscore.{name}"):
            getattr(beat, name)()
