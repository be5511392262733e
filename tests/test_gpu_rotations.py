"""Rotation output on the GPU (eg_skeleton_rotations through skeleton.rotations_from_tracks / launch_rotations, harness.synthesize(rotations=)
and GestureStream(rotations=)) against the float64 restatement tests/rotations_np.py, and against itself bit for bit.

Tolerance: E32 is the largest element-wise deviation of the restatement run in fp32 (every intermediate rounded) from the restatement in
float64 on the test's own inputs; the device must be within 8 x E32 on every element (the factor covers another operation order and fused
multiply-adds), and 8 x E32 <= 1e-4 so that it cannot grow unnoticed.  Global rotations are compared up to the sign of each quaternion.  The
accuracy inputs keep min(1 + c) >= 0.5, asserted from the restatement: the arc is ill-conditioned near a half turn, which the reconstruction
test (valid at any angle) and the exact half-turn cases cover."""
import numpy as np
import pytest
import torch

import rotations_np as RN
import skeleton_np as SN
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.synth import synth_audio
from skeleton_gpu_common import FPS, H_, HOP, LENGTHS, N, NAMES, P_, RAGGED, RATES, TF, dev, inputs, mean_of, skeleton, table_of, ted_models

pytestmark = pytest.mark.gpu


def up_to_sign(a, b):
    return np.minimum(np.abs(a - b), np.abs(a + b))


def accuracy_cases(name, rate):
    """The inputs of one accuracy test: every length around the tile height, B = 1 and 3, the mean on and off; with the float64 and the fp32
    restatement in both spaces.  Built without the GPU."""
    sk = skeleton(name)
    t, rest = table_of(sk), RN.random_rest(sk.K, 5)
    Lf, M = rate
    cases = []
    for i, T in enumerate(LENGTHS):
        for B in (1, 3):
            mean = mean_of(sk.K, 40 + i) if (i + B) % 2 else None
            v, _loc = RN.swing_tracks(t, rest, T, 100, 100 * i + B, B=B, mean=mean, smooth=True)
            m64 = None if mean is None else mean.astype(np.float64)
            ref = {}
            for space in ("local", "global"):
                want, cmin = RN.rotations(v, t, rest, None, m64, space, Lf, M, want_c=True)
                assert 1 + cmin >= 0.5, (name, rate, T, B, cmin)
                ref[space] = (want, RN.rotations(v, t, rest, None, mean, space, Lf, M, dtype=np.float32))
            cases.append((f"{name} T={T} B={B} L/M={rate} mean={mean is not None}", v, mean, ref))
    return sk, rest, cases


def e32_of(cases, space):
    dist = up_to_sign if space == "global" else (lambda a, b: np.abs(a - b))
    return max(float(dist(ref[space][1].astype(np.float64), ref[space][0]).max()) for _w, _v, _m, ref in cases)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_rotations_against_float64(name, rate):
    sk, rest, cases = accuracy_cases(name, rate)
    for space in ("local", "global"):
        E32 = e32_of(cases, space)
        tol = 8 * E32
        assert 0 < tol <= 1e-4, (space, E32)
        worst = 0.0
        for what, v, mean, ref in cases:
            got = SK.rotations_from_tracks(torch.from_numpy(v).to(dev()), sk, rest, mean=None if mean is None else torch.from_numpy(mean),
                                           fps=FPS[rate], space=space)
            if FPS[rate] is not None:
                got, n_out = got
                assert n_out == [SN.out_frames(v.shape[1], *rate)] * v.shape[0]
            want = ref[space][0]
            g = got.cpu().numpy().astype(np.float64)
            assert g.shape == want.shape and got.dtype == torch.float32 and got.is_cuda, what
            assert np.isfinite(g).all(), what
            err = up_to_sign(g, want) if space == "global" else np.abs(g - want)
            worst = max(worst, float(err.max()))
            assert (err <= tol).all(), (what, space, float(err.max()) / tol)
            if space == "local":
                assert (g[..., 0] >= 0).all(), what
        print(f"{name} L/M={rate} {space}: E32 {E32:.3e}, worst error / tolerance {worst / tol:.3f}")


@pytest.mark.parametrize("cap", [100, 175])
@pytest.mark.parametrize("name", ["ted", "random63"])
def test_globals_turn_the_rest_pose_into_the_track(name, cap):
    """G_k o rest_k against x^_k, within 8 x the reconstruction error of the fp32 restatement: valid at any angle.  That error itself grows
    towards the half turn (the arc's normalisation divides by a norm of about sqrt(2 (1 + c))), so it carries no fixed cap here."""
    sk = skeleton(name)
    t, rest = table_of(sk), RN.random_rest(sk.K, 6)
    for rate in ((1, 1), (5, 3)):
        mean = mean_of(sk.K, 50)
        v, _loc = RN.swing_tracks(t, rest, 2 * TF + 3, cap, 61, B=2, mean=mean, smooth=True)
        x = RN.unit_vectors(v, t, None, mean.astype(np.float64), *rate)
        E = float(np.abs(RN.directions(RN.rotations(v, t, rest, None, mean, "global", *rate, dtype=np.float32), rest) - x).max())
        got = SK.rotations_from_tracks(torch.from_numpy(v).to(dev()), sk, rest, mean=torch.from_numpy(mean), fps=FPS[rate], space="global")
        got = got[0] if FPS[rate] is not None else got
        g = got.cpu().numpy().astype(np.float64)
        err = float(np.abs(RN.directions(g, rest) - x).max())
        print(f"{name} cap={cap} L/M={rate}: reconstruction error {err:.3e}, fp32 restatement {E:.3e}, ratio to 8 x {err / (8 * E):.3f}")
        assert np.isfinite(g).all() and E > 0 and err <= 8 * E
        assert np.abs(np.sqrt((g * g).sum(-1)) - 1).max() <= 1e-5


def test_exact_half_turns():
    for rest, want in (((0, 0, 1), (0, 0, 1, 0)), ((1, 0, 0), (0, 0, 0, 1))):
        sk = SK.Skeleton([0], [1], [0.5])
        r = np.array([rest], np.float32)
        v = torch.from_numpy((-1.5 * r).reshape(1, 1, 3)).to(dev())
        for space in ("local", "global"):
            got = SK.rotations_from_tracks(v, sk, r, space=space).cpu().numpy()
            assert np.array_equal(got[0, 0, 0], np.array(want, np.float32)), (rest, space, got)
    # a half turn in the middle of a chain: every bone below it stays finite and unit, and the directions are reproduced
    sk = skeleton("chain")
    t = table_of(sk)
    rest = RN.unit_rest(np.array([[0, 0, 1.0], [0, 1.0, 0], [1.0, 0, 0], [0, 0, 1.0], [0, 1.0, 0]]))
    x = rest.astype(np.float64).copy()
    x[1] = -x[1]
    v = np.tile((x * 0.7).reshape(1, 1, 15), (1, TF + 1, 1)).astype(np.float32)
    got = SK.rotations_from_tracks(torch.from_numpy(v).to(dev()), sk, rest, space="global").cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.abs(np.sqrt((got * got).sum(-1)) - 1).max() <= 1e-6
    assert np.abs(RN.directions(got, rest) - x).max() <= 1e-6
    assert np.abs(got - RN.rotations(v, t, rest, space="global")).max() <= 1e-6


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_ragged_rows_with_nan_behind_their_end(name, rate):
    sk = skeleton(name)
    t, rest = table_of(sk), RN.random_rest(sk.K, 7)
    T = max(RAGGED) + 2
    for space in ("local", "global"):
        mean = mean_of(sk.K, 9) if space == "global" else None
        v, _loc = RN.swing_tracks(t, rest, T, 100, 8, B=len(RAGGED), mean=mean, smooth=True)
        for b, n in enumerate(RAGGED):
            v[b, n:] = np.nan
        mt = None if mean is None else torch.from_numpy(mean)
        got, n_out = SK.rotations_from_tracks(torch.from_numpy(v).to(dev()), sk, rest, frames=RAGGED, mean=mt, fps=FPS[rate], space=space)
        assert n_out == [SN.out_frames(n, *rate) for n in RAGGED] and torch.isfinite(got).all()
        want = RN.rotations(v, t, rest, RAGGED, None if mean is None else mean.astype(np.float64), space, *rate)
        assert up_to_sign(got.cpu().numpy().astype(np.float64), want).max() <= 1e-4
        for b, n in enumerate(RAGGED):
            assert not got[b, n_out[b]:].any() and got[b, :n_out[b]].any()
            # bit for bit: every recording alone, in a tensor of its own length
            alone = SK.rotations_from_tracks(torch.from_numpy(v[b:b + 1, :n].copy()).to(dev()), sk, rest, mean=mt, fps=FPS[rate], space=space)
            alone = alone[0] if FPS[rate] is not None else alone
            assert alone.shape[1] == n_out[b] and torch.equal(got[b:b + 1, :n_out[b]], alone), (name, rate, space, b)


def test_draws_axis_equals_the_flattened_call():
    sk = skeleton("ted")
    t, rest = table_of(sk), RN.random_rest(sk.K, 7)
    U, R, T = 2, 2, TF + 1
    v, _loc = RN.swing_tracks(t, rest, T, 100, 21, B=U * R, smooth=True)
    v = v.reshape(U, R, T, -1)
    v[1, :, 5:] = np.nan
    x = torch.from_numpy(v).to(dev())
    for fps in (None, (15, 25)):
        got, n_out = SK.rotations_from_tracks(x, sk, rest, frames=[T, 5], fps=fps)
        flat, n_flat = SK.rotations_from_tracks(x.reshape(U * R, T, -1), sk, rest, frames=[T, T, 5, 5], fps=fps)
        assert got.shape[:2] == (U, R) and n_flat == [n for n in n_out for _ in range(R)]
        assert torch.equal(got.reshape(flat.shape), flat) and torch.isfinite(flat).all()
        want = RN.rotations(v.reshape(U * R, T, -1), t, rest, [T, T, 5, 5], None, "local", *SK.rate_ratio(fps))
        assert np.abs(flat.cpu().numpy() - want).max() <= 1e-4


@pytest.mark.parametrize("rate", [(1, 1), (5, 3)])
def test_out_stride_batch_and_tile_do_not_change_the_bits(rate):
    sk = skeleton("ted")
    t, rest = table_of(sk), RN.random_rest(sk.K, 7)
    pose = sk.rest_pose(rest)
    T = 2 * TF + 3
    v, _loc = RN.swing_tracks(t, rest, T, 100, 23, B=3, smooth=True)
    x = torch.from_numpy(v).to(dev())
    base = SK.launch_rotations(x, sk, pose, ratio=rate)
    t_out = base.shape[1]
    wide = torch.full((3, t_out + TF + 5, sk.K, 4), float("nan"), device=dev())
    SK.launch_rotations(x, sk, pose, ratio=rate, out=wide)
    assert torch.equal(wide[:, :t_out], base) and not wide[:, t_out:].any()
    for b in range(3):                                           # another batch, another place in it
        assert torch.equal(SK.launch_rotations(x[b:b + 1].clone(), sk, pose, ratio=rate), base[b:b + 1])
    assert torch.equal(SK.launch_rotations(x.flip(0).contiguous(), sk, pose, ratio=rate), base.flip(0))
    if rate == (1, 1):                                           # the same frames in another tile, at another place of it
        for s in (1, TF - 1, TF + 7):
            assert torch.equal(SK.launch_rotations(x[:, s:].contiguous(), sk, pose), base[:, s:])


def test_graph_replay_equals_the_eager_call():
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    sk = skeleton("ted")
    t, rest = table_of(sk), RN.random_rest(sk.K, 7)
    pose = sk.rest_pose(rest)
    v, _loc = RN.swing_tracks(t, rest, max(RAGGED), 100, 33, B=3, smooth=True)
    x = torch.from_numpy(v).to(dev())
    mean = torch.from_numpy(mean_of(sk.K, 34)).to(dev())
    d_frames = torch.tensor(RAGGED, dtype=torch.int32, device=dev())
    eager = {sp: SK.launch_rotations(x, sk, pose, d_frames, mean=mean, space=sp, ratio=(5, 3)) for sp in ("local", "global")}   # also the warm-up
    out = {sp: torch.full_like(eager[sp], float("nan")) for sp in eager}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        for sp in out:
            SK.launch_rotations(x, sk, pose, d_frames, mean=mean, space=sp, ratio=(5, 3), out=out[sp])
    for sp in out:
        out[sp].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[sp], eager[sp]) for sp in out) and not torch.equal(eager["local"], eager["global"])


# ---- the callers ---------------------------------------------------------------------------------------------------------------------------
def test_synthesize_rotations_equal_the_function_on_its_track():
    model, vae = ted_models()
    sk = skeleton("ted")
    rest = RN.random_rest(sk.K, 7)
    U, W = 2, 2
    g = inputs(U, W, 80)
    mean = torch.from_numpy(mean_of(sk.K, 81)).to(dev())
    # lengths=: recording 1 has one window fewer
    lens = [2 * HOP - 7, HOP - 5]
    audio = torch.from_numpy(synth_audio(U, max(lens), seed=80)).to(dev())
    kw = dict(labels=g["label"][:, 0].contiguous(), hop_samples=HOP, z=g["z"], lengths=lens)
    plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], joints=sk, joints_mean=mean, joints_fps=(15, 30), **kw)
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], joints=sk, joints_mean=mean, joints_fps=(15, 30), rotations=rest,
                        rotations_space="global", **kw)
    assert set(got) == set(plain) | {"rotations"} and torch.equal(got["track"], plain["track"]) and torch.equal(got["joints"], plain["joints"])
    frames = [w * H_ + P_ for w in got["windows_per"]]
    want, n_out = SK.rotations_from_tracks(got["track"], sk, rest, frames=frames, mean=mean, fps=(15, 30), space="global")
    assert n_out == got["joint_frames"] and tuple(got["rotations"].shape) == (U, 2 * (W * H_ + P_), 42, 4) and torch.equal(got["rotations"], want)
    assert not got["rotations"][1, n_out[1]:].any() and got["rotations"][1, :n_out[1]].any()
    # draws=2, rectangular
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=82)).to(dev())
    zz = torch.from_numpy(np.random.default_rng(83).standard_normal((U, 2, W, 32)).astype(np.float32))
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], labels=g["label"], hop_samples=HOP, z=zz, draws=2, joints=sk, rotations=rest)
    assert tuple(got["rotations"].shape) == (U, 2, W * H_ + P_, 42, 4)
    assert torch.equal(got["rotations"], SK.rotations_from_tracks(got["track"], sk, rest))
    assert torch.isfinite(got["rotations"]).all() and (got["rotations"][..., 0] >= 0).all()


def test_stream_last_rotations_and_tail_rotations():
    """A whole session of three emitting pushes: the pushes' rotations followed by tail_rotations() are the rotations of synthesize's track."""
    model, vae = ted_models()
    sk = skeleton("ted")
    rest = RN.random_rest(sk.K, 7)
    U = 2
    g = inputs(U, 4, 80)
    mean = torch.from_numpy(mean_of(sk.K, 85)).to(dev())
    T = 2 * HOP + N - 9000
    audio = torch.from_numpy(synth_audio(U, T, seed=80)).to(dev())
    padded = torch.zeros(U, 4 * HOP, device=dev())
    padded[:, :T] = audio
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=sk, joints_mean=mean, rotations=rest)
    assert s.last_rotations is None
    parts = []
    for k in range(1, 5):
        c = max(0, k - 2)
        rows, valid = s.push(padded[:, (k - 1) * HOP:k * HOP].contiguous(), g["text"][:, c], g["label"][:, c], g["z"][:, c], ends=T - 3 * HOP if k == 4 else None)
        assert (rows is None) == (s.last_rotations is None) == (k == 1)
        if rows is not None:
            assert tuple(s.last_rotations.shape) == (U, H_, 42, 4)
            want, _n = SK.rotations_from_tracks(rows, sk, rest, frames=[H_ * a for a in valid.cpu().tolist()], mean=mean)
            assert torch.equal(s.last_rotations, want)
            parts.append(s.last_rotations)
    assert len(parts) == 3
    assert torch.equal(s.tail_rotations(), SK.rotations_from_tracks(s.tail(), sk, rest, mean=mean))
    W = 3
    syn = Hs.synthesize((model, vae), audio, g["text"][:, :W].contiguous(), g["seed_pose"], labels=g["label"][:, :W].contiguous(), hop_samples=HOP,
                        z=g["z"][:, :W].contiguous(), windows=W, joints=sk, joints_mean=mean, rotations=rest)
    got = torch.cat(parts + [s.tail_rotations()], 1)
    assert got.shape == syn["rotations"].shape and torch.equal(got, syn["rotations"])
    assert torch.equal(syn["rotations"], SK.rotations_from_tracks(syn["track"], sk, rest, mean=mean))
    # a row that is not valid in a step has zero rotations
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=sk, rotations=rest, rotations_space="global")
    short = torch.from_numpy(synth_audio(U, HOP, seed=86)).to(dev())
    rows, valid = s.push(short, g["text"][:, 0], g["label"][:, 0], g["z"][:, 0], ends=[-1, 700])
    assert valid.cpu().tolist() == [0, 1] and not s.last_rotations[0].any() and s.last_rotations[1].any()
