"""The delayed output stage of a stream on the GPU, alone, without a model (render.StreamRender: eg_render_stream_* and the window form of the
four output kernels): random-but-smooth chunks and a hand-written schedule of valid flags.

(a) every finished row -- cat(steps)[lead:] followed by the tail -- equals the offline composition TrackOutputs.tracks(smooth_tracks(x)) bit for
    bit, the first `lead` entries of a row's first step are zeros and a row that is not valid has zeros;
(b) an independent net: the float64 restatements of the whole-track tests (tests/skeleton_np.py, rotations_np.py, articulate_np.py, euler_np.py) on
    the offline fp32 smoothed track, within those tests' own bounds -- skeleton_np.joints_bound, and 8 x E32 (E32: the restatement in fp32 against
    the restatement in float64 on the same inputs, <= 1e-4 / 8) for the rotations, the tree's joints and the Euler channels
    (tests/test_gpu_euler.py: masks, errors, bounds_of).  No tolerance of its own;
(c) poison: the chunk of a row that is not valid and the stage's window buffer before the first step are NaN; every output stays finite;
(d) the launches of one eager run: the smoother's two, the delay line's two, then the output launches the offline call makes.

Schedule, U = 3, five steps: row 0 runs five steps; row 1 stops being valid after three; row 2 ends after two, is reset, sits out step 2 beside
rows that are valid, and runs a second track in steps 3 and 4.  Shapes: H = 6 with window 5 (lead and limit in one tile) and without a filter
(the delay line holds raw rows, delta = d), H = 30 with windows 9 and 29; ratios 1/1, 2/1 (Hout = 60 spans tiles of both kernels: lead and limit
fall in different tiles), 5/3 and 1/2 (the rate drops: a tile's outputs take several passes over the window)."""
import numpy as np
import pytest
import torch

import articulate_np as AN
import euler_np as EN
import rotations_np as RN
import skeleton_np as SN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import render as RD
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd import smooth as SM
from skeleton_gpu_common import dev, mean_of, skeleton, table_of

pytestmark = pytest.mark.gpu

U, P = 3, 4
VALID = [[1, 1, 1], [1, 1, 1], [1, 1, 0], [1, 0, 1], [1, 0, 1]]
SHAPES = [(6, 5, 2), (6, 0, 0), (30, 9, 3), (30, 29, 3)]        # H, window (0: no filter), polyorder
RATES = {(1, 1): None, (2, 1): (15, 30), (5, 3): (15, 25), (1, 2): (30, 15)}
BODIES = ["chain", "ted", "tree5", "upper47"]
_TREES = {}


def tree_of(name):
    if name not in _TREES:
        body = AN.chain(5) if name == "tree5" else AN.upper47()
        _TREES[name] = (body, SK.JointTree(*body))
    return _TREES[name]


def up_to_sign(a, b):
    return np.minimum(np.abs(a - b), np.abs(a + b))


def setup(name, H, seed):
    """The body's spec arguments, the restatement's view of them, and smooth raw tracks of 5, 3, 2 and 2 steps (+ P)."""
    steps = [5, 3, 2, 2]
    if name in ("chain", "ted"):
        sk = skeleton(name)
        rest, mean = RN.random_rest(sk.K, 5), mean_of(sk.K, seed)
        tracks = [RN.swing_tracks(table_of(sk), rest, s * H + P, 100, seed + 10 * i, mean=mean, smooth=True)[0][0] for i, s in enumerate(steps)]
        space = "global" if name == "chain" else "local"
        return dict(joints=sk, mean=mean, unit=name == "chain", rotations=rest, rotations_space=space), dict(sk=sk, rest=rest, mean=mean, space=space), tracks
    body, tree = tree_of(name)
    mean = (np.random.default_rng(seed).standard_normal(6 * tree.J) * 0.2).astype(np.float32)
    tracks = [AN.rotation_tracks(tree.J, s * H + P, seed + 10 * i, mean=mean)[0] for i, s in enumerate(steps)]
    codes = EN.orders_cyclic(tree.J)
    space = "global" if name == "tree5" else "local"
    return (dict(joints=tree, mean=mean, rotations=True, rotations_space=space, euler=[EN.ORDERS[c] for c in codes]),
            dict(body=body, tree=tree, mean=mean, space=space, codes=codes), tracks)


def restated(ref, y, got, Lf, M, what):
    """(b): the float64 restatements on the offline fp32 smoothed track y [T, D] (numpy) against the stage's outputs `got`."""
    v = y[None]
    g = {n: t.cpu().numpy().astype(np.float64)[None] for n, t in got.items()}
    m64 = ref["mean"].astype(np.float64)
    if "sk" in ref:
        t = table_of(ref["sk"])
        unit = ref["sk"].K == 5
        want, bound = SN.joints(v, t, None, m64, unit, Lf, M), SN.joints_bound(v, t, None, m64, unit, Lf, M)
        err = np.abs(g["joints"] - want)
        assert (err <= bound).all(), (what, "joints", float((err[bound > 0] / bound[bound > 0]).max()))
        q64, cmin = RN.rotations(v, t, ref["rest"], None, m64, ref["space"], Lf, M, want_c=True)
        assert 1 + cmin >= 0.5, (what, cmin)
        q32 = RN.rotations(v, t, ref["rest"], None, ref["mean"], ref["space"], Lf, M, dtype=np.float32)
        dist = up_to_sign if ref["space"] == "global" else (lambda a, b: np.abs(a - b))
        tol = 8 * float(dist(q32.astype(np.float64), q64).max())
        assert 0 < tol <= 1e-4, (what, tol)
        err = dist(g["rotations"], q64)
        assert (err <= tol).all(), (what, "rotations", float(err.max()) / tol)
        return
    import test_gpu_euler as TE                                             # the Euler tests' own masks, errors and bounds
    body, tree, codes = ref["body"], ref["tree"], ref["codes"]
    j64, q64, (n1, n2) = AN.articulate(v, body, False, None, m64, ref["space"], Lf, M, want_norms=True)
    assert n1 >= 0.25 and n2 >= 0.25, (what, n1, n2)
    j32, q32 = AN.articulate(v, body, False, None, ref["mean"], ref["space"], Lf, M, dtype=np.float32)
    tol_j, tol_q = 8 * float(np.abs(j32.astype(np.float64) - j64).max()), 8 * float(up_to_sign(q32.astype(np.float64), q64).max())
    assert 0 < tol_q <= 1e-4 and 0 < tol_j <= 1e-4 * AN.path_length(body), (what, tol_j, tol_q)
    assert (np.abs(g["joints"] - j64) <= tol_j).all(), (what, "joints", float(np.abs(g["joints"] - j64).max()) / tol_j)
    assert (up_to_sign(g["rotations"], q64) <= tol_q).all(), (what, "rotations", float(up_to_sign(g["rotations"], q64).max()) / tol_q)
    e64, R64, s64, _n = EN.euler(v, codes, False, None, m64, Lf, M, True, want=True)
    case = dict(what=what, codes=codes, degrees=True, e64=e64, R64=R64, s64=s64, e32=EN.euler(v, codes, False, None, ref["mean"], Lf, M, True, dtype=np.float32))
    tol_m, tol_a = TE.bounds_of([case])
    ok, band = TE.masks(case)
    em, ea = TE.errors(g["euler"].astype(np.float32), case)
    assert (em[~band] <= tol_m).all(), (what, "euler, matrix space", float(em[~band].max()), tol_m)
    assert (ea[ok & ~band] <= tol_a).all(), (what, "euler, angle space", float(ea[ok & ~band].max(initial=0.0)), tol_a)


@pytest.mark.parametrize("rate", list(RATES), ids=lambda r: f"{r[0]}over{r[1]}")
@pytest.mark.parametrize("H,K,p", SHAPES)
@pytest.mark.parametrize("name", BODIES)
def test_stage_tiles_the_offline_composition_bit_for_bit(name, H, K, p, rate):
    Lf, M = rate
    kw, ref, tracks = setup(name, H, 1000 + 10 * H + K)
    D = tracks[0].shape[1]
    sm = SM.Smoother(K, p) if K else None
    spec = RD.RenderSpec(fps=RATES[rate], smooth=sm, **kw)
    rd = RD.StreamRender(U, H, P, D, spec, device=dev(), src_fps=30 if rate == (1, 2) else 15)
    plan = RD.stream_plan(H, P, K // 2, Lf, M)
    assert (rd.delay, rd.frames, rd.lead, rd.tail_frames) == (plan.d, plan.Hout, plan.lead, plan.n_tail)
    offline = SK.TrackOutputs("offline", kw["joints"], kw["mean"], kw.get("unit", False), RATES[rate], kw["rotations"], kw["rotations_space"],
                              kw.get("euler")).fit(D)
    names = offline.made
    rd._window.fill_(float("nan"))                                          # (c): behind the valid frames of the window buffer
    cur = {0: [tracks[0], 0], 1: [tracks[1], 0], 2: [tracks[2], 0]}         # the row's track and the steps it has emitted
    emitted = {u: [] for u in range(U)}

    def tail_rows():
        t = torch.zeros(U, P, D)
        for u, (x, s) in cur.items():
            t[u] = torch.from_numpy(x[s * H:s * H + P])                     # the raw frames behind the last step emitted: the prior of the row
        return t.to(dev())

    def finished(u, tail):
        x, s = cur[u]
        assert s * H + P == len(x), (u, s)
        y = torch.from_numpy(x).to(dev())
        if sm is not None:
            y = SM.smooth_tracks(y, sm)
        want = offline.tracks(y[None], [len(x)])
        got = {}
        for n in names:
            assert len(emitted[u]) == s
            steps = torch.cat([o[n] for o in emitted[u]], 0)
            assert not steps[:plan.lead].any() and bool(steps[plan.lead:].any()), (u, n)
            got[n] = torch.cat([steps[plan.lead:], tail[n][u]], 0)
            assert got[n].shape == want[n][0].shape and torch.equal(got[n], want[n][0]), (name, H, K, rate, u, n)
        assert want["joint_frames"] == [-(-len(x) * Lf // M)]
        restated(ref, y.cpu().numpy(), got, Lf, M, f"{name} H={H} K={K} L/M={rate} row {u}")

    for k, valid in enumerate(VALID):
        chunk = torch.full((U, H, D), float("nan"))
        for u in range(U):
            if valid[u]:
                x, s = cur[u]
                chunk[u] = torch.from_numpy(x[s * H:(s + 1) * H])
                cur[u][1] = s + 1
        before = L.load().eg_launch_count()
        out = rd.run(chunk.to(dev()), torch.tensor(valid, dtype=torch.int32, device=dev()))
        launches = L.load().eg_launch_count() - before
        made = (2 if not offline.tree and offline.want_rotations else 1) + (offline.euler is not None)
        assert launches == (2 if sm is not None else 0) + 2 + made, (launches, made)       # (d)
        assert set(out) == set(names)
        for n in names:
            assert tuple(out[n].shape[:2]) == (U, plan.Hout) and bool(torch.isfinite(out[n]).all()), (k, n)
        for u in range(U):
            if valid[u]:
                emitted[u].append({n: out[n][u].clone() for n in names})
            else:
                assert not any(bool(out[n][u].any()) for n in names), (k, u)
        if k == 1:                                                          # row 2's first track ends here: two steps
            tail = rd.tail(tail_rows())
            assert all(tuple(tail[n].shape[:2]) == (U, plan.n_tail) and bool(torch.isfinite(tail[n]).all()) for n in names)
            finished(2, tail)
            emitted[2], cur[2] = [], [tracks[3], 0]
            rd.reset(rows=[2])
    tail = rd.tail(tail_rows())
    for u in range(U):
        finished(u, tail)


def test_a_row_that_has_emitted_nothing_has_a_zero_tail_and_snapshot_restores():
    """tail() before any step: zeros; snapshot / restore bring the state back: the same step twice gives the same bits."""
    sk = skeleton("chain")
    rd = RD.StreamRender(2, 6, P, 15, dict(joints=sk, smooth=(5, 2), fps=(15, 30)), device=dev())
    t = rd.tail(torch.randn(2, P, 15, device=dev()))
    assert not t["joints"].any() and tuple(t["joints"].shape) == (2, rd.tail_frames, 6, 3)
    a, b = torch.randn(2, 6, 15, device=dev()), torch.randn(2, 6, 15, device=dev())
    rd.run(a)
    snap = rd.snapshot()
    first = rd.run(b)["joints"].clone()
    rd.restore(snap)
    assert torch.equal(rd.run(b)["joints"], first) and bool(first.any())
