"""GestureStream(render=): the delayed output stage inside a live session (one captured graph per push) against harness.synthesize(smooth=,
joints=, rotations=, euler=, joints_fps=) on the same audio, bit for bit.

The scenario of tests/test_gpu_smooth.py::test_stream_pushes_and_tail_are_the_offline_call_on_the_finished_track: U = 3, six pushes (a window
spans two): row 0 runs through (five windows); row 1 ends inside push 3 (three windows, then not valid); row 2 is reset after push 3 (two
windows) and rejoins with a second recording, so it is not valid in push 4 beside rows that are.  Every finished track: for every output name
the concatenated last_render without the first step's leading render_lead entries, then tail_render(), against synthesize on the row's own
audio, text, labels, z and seed pose (in a batch of two recordings, as tests/test_gpu_stream.py compares rows)."""
import numpy as np
import pytest
import torch

from emotiongestures_amd import harness as Hs
from emotiongestures_amd import render as RD
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.synth import synth_audio
from skeleton_gpu_common import D_, H_, HOP, P_, dev, inputs, mean_of, ted_models

pytestmark = pytest.mark.gpu

U = 3
SEEN = [[0, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 0], [1, 0, 1], [1, 0, 1]]


def scenario(models, g, audio, hop, H, P, render, syn_kw, open_kw=None, other=None):
    """Runs the six pushes with render= (and open_kw); checks every finished track; returns per push (rows, valid, last_render, extras) and the
    final tail.  `other`: a session without render= (same open_kw) that must return the same rows, tail and extras."""
    s = Hs.open_stream(models, U, g["seed_pose"], hop_samples=hop, render=render, **(open_kw or {}))
    spec = RD.RenderSpec.of(render)
    plan = spec.plan(H, P, g["seed_pose"].shape[2], 15)
    assert (s.render_delay, s.render_frames, s.render_lead) == (plan.d, plan.Hout, plan.lead) and s.last_render is None
    names = spec.outputs.made
    lead = plan.lead
    raw, ren = [[] for _ in range(U)], [[] for _ in range(U)]
    log = []

    def syn(a2, W, cols, row):
        """synthesize on a batch of two recordings of one length; text / label / z of the stream's row `row` at the pushes `cols`."""
        pick = lambda t: torch.stack([t[row, cols], t[(row + 1) % U, cols]])
        return Hs.synthesize(models, a2, pick(g["text"]), torch.stack([g["seed_pose"][row], g["seed_pose"][(row + 1) % U]]), labels=pick(g["label"]),
                             hop_samples=hop, z=pick(g["z"]), windows=W, **syn_kw)

    def finished(u, lo, hi, cols):
        """Row u's finished track against synthesize on its audio [lo, hi)."""
        W = len(cols)
        assert len(raw[u]) == W == len(ren[u])
        track = torch.cat(raw[u] + [s.tail()[u]], 0)
        tail = s.tail_render()
        want = syn(torch.stack([audio[u, lo:hi], audio[(u + 1) % U, lo:hi]]), W, cols, u)
        assert torch.equal(track, want["track"][0]), ("the raw track", u)
        n = want["joint_frames"][0]
        for name in names:
            steps = torch.cat([r[name] for r in ren[u]], 0)
            assert tuple(tail[name].shape[:2]) == (U, plan.n_tail)
            assert not steps[:lead].any() and bool(steps[lead:].any()), (u, name)
            got = torch.cat([steps[lead:], tail[name][u]], 0)
            assert got.shape[0] == n == -(-(W * H + P) * spec.ratio[0] // spec.ratio[1]), (u, name, got.shape, n)
            assert torch.equal(got, want[name][0][:n]), (u, name)
        return W

    for k in range(6):
        args = (audio[:, k * hop:(k + 1) * hop].contiguous(), g["text"][:, k], g["label"][:, k], g["z"][:, k])
        ends = [-1, 100, -1] if k == 2 else None
        rows, valid = s.push(*args, ends=ends)
        v = valid.cpu().tolist()
        assert v == SEEN[k] and (rows is None) == (s.last_render is None) == (k == 0)
        if other is not None:
            r2, v2 = other.push(*args, ends=ends)
            assert (rows is None) == (r2 is None) and torch.equal(valid, v2)
            assert rows is None or torch.equal(rows, r2)
            for attr in ("last_joints", "last_rotations", "last_smooth"):
                a, b = getattr(s, attr), getattr(other, attr)
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (k, attr)
        if rows is not None:
            assert set(s.last_render) == set(names) and all(tuple(t.shape[:2]) == (U, plan.Hout) for t in s.last_render.values())
            assert all(bool(torch.isfinite(t).all()) for t in s.last_render.values())
        log.append((rows, v, s.last_render))
        for u in range(U):
            if v[u]:
                raw[u].append(rows[u])
                ren[u].append({n: t[u] for n, t in s.last_render.items()})
            elif rows is not None:
                assert not any(bool(t[u].any()) for t in s.last_render.values())        # a row that is not valid: zeros, and a state that did not move
        if k == 2:                                                      # row 2's first recording: the windows of pushes 2 and 3
            assert finished(2, 0, 3 * hop, [1, 2]) == 2
            raw[2], ren[2] = [], []
            s.reset(rows=[2])
            if other is not None:
                other.reset(rows=[2])
    assert finished(0, 0, 6 * hop, [1, 2, 3, 4, 5]) == 5
    assert finished(1, 0, 2 * hop + 100, [1, 2, 3]) == 3
    assert finished(2, 3 * hop, 6 * hop, [4, 5]) == 2
    if other is not None:
        assert torch.equal(s.tail(), other.tail())
    return s, log


def ted_case():
    sk = SK.ted_expressive()
    mean = torch.from_numpy(mean_of(sk.K, 71))
    rest = np.random.default_rng(72).standard_normal((sk.K, 3))
    g = inputs(U, 6, 90)
    audio = torch.from_numpy(synth_audio(U, 6 * HOP, seed=91)).to(dev())
    return sk, mean, rest, g, audio


@pytest.mark.parametrize("fps", [(15, 30), (15, 25)], ids=["15to30", "15to25"])
def test_ted_stream_render_is_synthesize_on_the_finished_track(fps):
    """render=(joints=ted, mean, unit, rotations=rest, smooth=(9, 3), fps).  At 15 -> 30 the session also has the raw joints= stage and is run
    beside a session without render=: the same rows, tail and last_joints / last_rotations; at 15 -> 25 the same with smooth= and last_smooth.
    An eager session returns the graph's bits."""
    models = ted_models()
    sk, mean, rest, g, audio = ted_case()
    render = dict(joints=sk, mean=mean, unit=True, rotations=rest, smooth=(9, 3), fps=fps)
    syn_kw = dict(smooth=(9, 3), joints=sk, joints_mean=mean, joints_unit=True, rotations=rest, joints_fps=fps)
    open_kw = dict(joints=sk, joints_mean=mean, rotations=rest) if fps == (15, 30) else dict(smooth=(9, 3))
    other = Hs.open_stream(models, U, g["seed_pose"], hop_samples=HOP, **open_kw)
    s, log = scenario(models, g, audio, HOP, H_, P_, render, syn_kw, open_kw, other)
    assert (s.render_delay, s.render_frames, s.render_lead) == ((5, 60, 10) if fps == (15, 30) else (6, 50, 10))
    e = Hs.open_stream(models, U, g["seed_pose"], hop_samples=HOP, render=RD.RenderSpec(**render), graph=False)
    for k in range(3):
        rows, _v = e.push(audio[:, k * HOP:(k + 1) * HOP].contiguous(), g["text"][:, k], g["label"][:, k], g["z"][:, k], ends=[-1, 100, -1] if k == 2 else None)
        assert (rows is None) == (log[k][0] is None) and (rows is None or torch.equal(rows, log[k][0]))
        for n, t in (e.last_render or {}).items():
            assert torch.equal(t, log[k][2][n]), (k, n)


def test_render_without_filter_or_rate_change_is_the_joints_stage():
    """d = 0: render=(joints, mean, rotations) equals last_joints / last_rotations of the existing stage in every push, and the tails agree."""
    models = ted_models()
    sk, mean, rest, g, audio = ted_case()
    s = Hs.open_stream(models, U, g["seed_pose"], hop_samples=HOP, joints=sk, joints_mean=mean, rotations=rest,
                       render=dict(joints=sk, mean=mean, rotations=rest))
    assert (s.render_delay, s.render_frames, s.render_lead) == (0, H_, 0)
    for k in range(4):
        rows, _v = s.push(audio[:, k * HOP:(k + 1) * HOP].contiguous(), g["text"][:, k], g["label"][:, k], g["z"][:, k], ends=[-1, 100, -1] if k == 2 else None)
        assert (rows is None) == (s.last_render is None)
        if rows is not None:
            assert torch.equal(s.last_render["joints"], s.last_joints) and torch.equal(s.last_render["rotations"], s.last_rotations)
            assert bool(s.last_joints.any())
    t = s.tail_render()
    assert torch.equal(t["joints"], s.tail_joints()) and torch.equal(t["rotations"], s.tail_rotations())
    with pytest.raises(RuntimeError, match="tail_render: the session was opened without render="):
        Hs.open_stream(models, U, g["seed_pose"], hop_samples=HOP).tail_render()


def test_beat_stream_render_tree_rotations_and_euler():
    """The BEAT mirror (282 columns, H = 50): joints=tree, rotations=True, euler="ZXY", smooth=(9, 3), 15 -> 30 fps."""
    import test_gpu_articulate as TA
    models = TA.beat_models()
    _body, tree = TA.tree_of("upper47")
    g = TA.beat_inputs(U, 6, 120)
    audio = TA.gpu(synth_audio(U, 6 * TA.HOP, seed=93))
    render = dict(joints=tree, rotations=True, euler="ZXY", smooth=(9, 3), fps=(15, 30))
    syn_kw = dict(smooth=(9, 3), joints=tree, rotations=True, euler="ZXY", joints_fps=(15, 30))
    s, _log = scenario(models, g, audio, TA.HOP, TA.HB, TA.PB, render, syn_kw)
    assert (s.render_delay, s.render_frames, s.render_lead) == (5, 100, 10)
