"""The delayed output stage of a stream without a GPU: render.stream_plan against the worked table, every refusal by name, and the geometry of the
stage -- the numpy restatement tests/render_np.py (the delay line) around the package's float64 host paths tiles the whole-track float64 result
exactly."""
import numpy as np
import pytest
import torch

import articulate_np as AN
import render_np as RN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import render as RD
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd import smooth as SM
from emotiongestures_amd import streaming as S

FPS = {(1, 1): None, (2, 1): (15, 30), (4, 1): (15, 60), (5, 3): (15, 25), (1, 2): (30, 15)}
WINDOWS = {0: None, 5: (5, 2), 9: (9, 3), 29: (29, 3)}


@pytest.fixture(scope="module")
def ted():
    return SK.ted_expressive()


@pytest.fixture(scope="module")
def tree():
    return SK.JointTree(*AN.chain(5))


def test_stream_plan_returns_the_worked_table():
    """H = 30: the six rows of the table, and the tail's frames ceil((d + P) L / M) for P = 4."""
    for (half, Lf, M), want in {(4, 2, 1): (5, 1, 60, 10), (4, 5, 3): (6, 2, 50, 10), (0, 2, 1): (1, 1, 60, 2), (14, 5, 3): (15, 1, 50, 25),
                                (4, 1, 1): (4, 0, 30, 4), (0, 1, 2): (2, 2, 15, 1)}.items():
        p = RD.stream_plan(30, 4, half, Lf, M)
        assert tuple(p[:4]) == want == (p.d, p.delta, p.Hout, p.lead), (half, Lf, M)
        assert p.n_tail == -(-(p.d + 4) * Lf // M) and p.window == 30 + (Lf != M)
        assert tuple(p) == RN.plan(30, 4, half, Lf, M)
    assert tuple(RD.stream_plan(30, 4, 0, 1, 1)) == (0, 0, 30, 0, 4, 30)        # no filter, no rate change: the existing stage


def test_plan_refusals_by_name():
    """d > H cannot be reached with window <= H and H a multiple of M (d0 <= (H + 1) / 2 <= H = kM gives ceil(d0 / M) <= k), so stream_plan
    checks it before the window: half = 5 at H = M = 5 is d = 10."""
    with pytest.raises(L.EgError, match=r"H=30 frames per step.*30 \* 8 / 7 = 34.2857 output frames per step, not an integer.*multiple of 7 \(nearest: 28 or 35\)"):
        RD.stream_plan(30, 4, 4, 8, 7)
    with pytest.raises(L.EgError, match=r"H=6 .*multiple of 4 \(nearest: 4 or 8\)"):
        RD.stream_plan(6, 4, 0, 5, 4)
    with pytest.raises(L.EgError, match=r"the delay d=10 frames .* > H=5 frames per step"):
        RD.stream_plan(5, 4, 5, 8, 5)
    with pytest.raises(L.EgError, match="window=9 > H=6"):
        RD.stream_plan(6, 4, 4, 1, 1)
    with pytest.raises(L.EgError, match="window=31 > H=30"):
        RD.stream_plan(30, 4, 15, 2, 1)


def test_spec_refusals_by_name_without_a_model(ted, tree):
    seed = torch.zeros(2, 4, 126)
    for open_ in (lambda **kw: S.GestureStream((None, None, None), 2, seed, **kw), lambda **kw: Hs.open_stream((None, None), 2, seed, **kw)):
        with pytest.raises(L.EgError, match="GestureStream: render: smooth: deriv=1"):
            open_(render=dict(joints=ted, smooth=SM.Smoother(9, 3, deriv=1)))
        with pytest.raises(L.EgError, match="GestureStream: render: euler_unwrap=True is not supported"):
            open_(render=dict(joints=tree, euler="ZXY", euler_unwrap=True))
        with pytest.raises(L.EgError, match="GestureStream: render: euler= with joints=Skeleton"):
            open_(render=RD.RenderSpec(ted, euler="ZXY"))
        with pytest.raises(L.EgError, match=r"GestureStream: render: fps=\(15, 2000\).*L=400 / M=3"):
            open_(render=dict(joints=ted, fps=(15, 2000)))
        with pytest.raises(L.EgError, match="window=8 is even"):
            open_(render=dict(joints=ted, smooth=(8, 3)))
        with pytest.raises(L.EgError, match=r"GestureStream: render: smooth=7: a smooth.Smoother or \(window, polyorder\)"):
            open_(render=dict(joints=ted, smooth=7))
        with pytest.raises(L.EgError, match="GestureStream: render=3: a render.RenderSpec or a dict"):
            open_(render=3)
        with pytest.raises(L.EgError, match="GestureStream: render: joints= is needed"):
            open_(render=dict(joints=None))
        # the existing refusals keep their text (and point at render=)
        with pytest.raises(L.EgError, match=r"GestureStream: joints_fps= is not supported.*render="):
            open_(joints=ted, joints_fps=(15, 30))
        with pytest.raises(L.EgError, match=r"GestureStream: smooth= together with joints= is not supported.*render="):
            open_(joints=ted, smooth=(9, 3))


def test_spec_refusals_against_a_models_geometry(ted, tree):
    """What needs H, P and pose_dim: RenderSpec.plan, which StreamRender runs before it touches a device."""
    with pytest.raises(L.EgError, match=r"GestureStream: render: joints=: the skeleton has K=42 bones, 3K=126 != pose_dim=282"):
        RD.RenderSpec(ted).plan(50, 10, 282)
    with pytest.raises(L.EgError, match=r"GestureStream: render: joints=: the joint tree has J=5 joints, 6J=30 != pose_dim=126"):
        RD.StreamRender(2, 30, 4, 126, dict(joints=tree), device="cpu")
    with pytest.raises(L.EgError, match="GestureStream: render: window=31 > H=30"):
        RD.StreamRender(2, 30, 4, 126, dict(joints=ted, smooth=(31, 3)), device="cpu")
    with pytest.raises(L.EgError, match=r"GestureStream: render: H=30 .* multiple of 4"):
        RD.RenderSpec(ted, fps=(20, 15)).plan(30, 4, 126)
    with pytest.raises(L.EgError, match=r"fps=\(20, 15\): the source rate must be the stream's fps=15"):
        RD.StreamRender(2, 30, 4, 126, dict(joints=ted, fps=(20, 15)), device="cpu")
    with pytest.raises(L.EgError, match="joints_unit=True with joints=JointTree"):
        RD.RenderSpec(tree, unit=True).plan(30, 4, 30)
    with pytest.raises(L.EgError, match="device must be a CUDA device"):
        RD.StreamRender(2, 30, 4, 126, dict(joints=ted, smooth=(9, 3), fps=(15, 30)), device="cpu")
    p = RD.RenderSpec(ted, smooth=(9, 3), fps=(15, 30), rotations=np.eye(3)[np.arange(42) % 3]).plan(30, 4, 126, 15)
    assert (p.d, p.delta, p.Hout, p.lead, p.n_tail) == (5, 1, 60, 10, 18)


def host_outputs(body, mean, fps, rest=None, unit=False, order=None):
    """The whole-track definition in float64 on the host: track [n, D] -> {name: [n_out, ., .]}."""
    take = (lambda r: r[0]) if fps is not None else (lambda r: r)
    if isinstance(body, SK.JointTree):
        return lambda t: {"joints": take(SK.joints_from_rot6d(t, body, mean=mean, fps=fps)),
                          "rotations": take(SK.rotations_from_rot6d(t, body, mean=mean, fps=fps, space="global")),
                          "euler": take(SK.euler_from_rot6d(t, body, order, mean=mean, fps=fps))}
    return lambda t: {"joints": take(SK.joints_from_tracks(t, body, mean=mean, unit=unit, fps=fps)),
                      "rotations": take(SK.rotations_from_tracks(t, body, rest, mean=mean, fps=fps))}


@pytest.mark.parametrize("ratio", list(FPS), ids=lambda r: f"{r[0]}over{r[1]}")
@pytest.mark.parametrize("H", [6, 30])
def test_the_stage_tiles_the_whole_track_result_exactly(H, ratio, ted, tree):
    """H in {6, 30} x P in {1, 4} x windows none / 5 / 9 / 29 (where <= H) x S in {1, 2, 5} x the five ratios, on the TED skeleton (joints with
    unit vectors, rotations) and a 5-joint tree (joints, global rotations, Euler channels): cat(steps)[lead:] + tail == the whole-track float64
    result, exactly; the first `lead` entries of step 0 are zeros."""
    Lf, M = ratio
    fps = FPS[ratio]
    rng = np.random.default_rng(100 * H + 10 * Lf + M)
    rest = rng.standard_normal((42, 3))
    bodies = [(126, host_outputs(ted, rng.standard_normal(126) * 0.2, fps, rest=rest, unit=True)),
              (30, host_outputs(tree, rng.standard_normal(30) * 0.2, fps, order=["ZXY", "XYZ", "YZX", "ZYX", "XZY"]))]
    for K in (k for k in WINDOWS if k <= H):
        half = K // 2
        for P in (1, 4):
            d, delta, Hout, lead, n_tail, W = RD.stream_plan(H, P, half, Lf, M)
            for S_ in (1, 2, 5):
                T = S_ * H + P
                for D, outputs in bodies:
                    x = rng.standard_normal((T, D))
                    y = x if K == 0 else SM.smooth_tracks(x, WINDOWS[K])
                    want = outputs(y)
                    steps, last = RN.chunks(y, H, S_, half)
                    outs, tail = RN.stage(steps, last, H, P, half, Lf, M, outputs)
                    got = RN.tiled(outs, tail, lead)
                    for n, v in want.items():
                        assert v.shape[0] == -(-T * Lf // M) and got[n].shape == v.shape, (K, P, S_, n)
                        assert np.array_equal(got[n], v), (K, P, S_, n, float(np.abs(got[n] - v).max()))
                        assert not outs[0][n][:lead].any() and (lead == 0 or outs[0][n][lead:].any())
                        assert all(o[n].shape[0] == Hout for o in outs) and tail[n].shape[0] == n_tail

