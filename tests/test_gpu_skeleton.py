"""Skeleton output on the GPU (eg_skeleton_joints / eg_skeleton_dir_vec through skeleton.joints_from_tracks / dir_vec_from_joints,
harness.synthesize(joints=), GestureStream(joints=) and the drop-ins) against the float64 restatement tests/skeleton_np.py, element by
element within the bounds derived there, and against itself bit for bit: ragged batch against single rows, [U, R, ...] against the flattened
call, graph replay against eager, the callers against the function."""
import os

import numpy as np
import pytest
import torch

import skeleton_np as SN
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.synth import synth_audio
from skeleton_gpu_common import FPS, H_, HOP, LENGTHS, N, P_, RAGGED, RATES, TF, dev, inputs, mean_of, skeleton, table_of, ted_models

pytestmark = pytest.mark.gpu


def tracks(B, T, K, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((B, T, 3 * K)) * scale).astype(np.float32)


def check_forward(sk, v, frames, mean, unit, rate, what):
    """One call on the device against the restatement, element by element; returns the device result."""
    Lf, M = rate
    kw = dict(frames=frames, mean=None if mean is None else torch.from_numpy(mean), unit=unit, fps=FPS[rate])
    got = SK.joints_from_tracks(torch.from_numpy(v).to(dev()), sk, **kw)
    if frames is not None or FPS[rate] is not None:
        got, n_out = got
        assert n_out == [SN.out_frames(n, Lf, M) for n in (frames if frames is not None else [v.shape[1]] * v.shape[0])]
    m64 = None if mean is None else mean.astype(np.float64)
    want = SN.joints(v, table_of(sk), frames, m64, unit, Lf, M)
    bound = SN.joints_bound(v, table_of(sk), frames, m64, unit, Lf, M)
    g = got.cpu().numpy().astype(np.float64)
    assert g.shape == want.shape and got.dtype == torch.float32 and got.is_cuda, what
    assert np.isfinite(g).all(), what
    err = np.abs(g - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert (err <= bound).all(), (what, ratio)
    if frames is not None:
        for b, n in enumerate(frames):
            assert not g[b, SN.out_frames(n, Lf, M):].any(), (what, b)
    return got


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("unit", [False, True])
def test_ted_tracks_against_float64(unit, rate):
    """Every length around the tile height, B = 1 and 3, mean on and off."""
    sk = skeleton("ted")
    for i, T in enumerate(LENGTHS):
        for B in (1, 3):
            mean = mean_of(sk.K, 40 + i) if (i + B) % 2 else None
            check_forward(sk, tracks(B, T, sk.K, 100 * i + B, scale=[0.01, 1.0, 30.0][i % 3]), None, mean, unit, rate,
                          f"ted T={T} B={B} unit={unit} L/M={rate} mean={mean is not None}")


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", ["ted", "chain", "star", "random63"])
def test_ragged_rows_with_nan_behind_their_end(name, rate):
    sk = skeleton(name)
    T = max(RAGGED) + 2
    for unit in (False, True):
        v = tracks(len(RAGGED), T, sk.K, 7 + unit)
        for b, n in enumerate(RAGGED):
            v[b, n:] = np.nan
        mean = mean_of(sk.K, 9) if unit else None
        got = check_forward(sk, v, RAGGED, mean, unit, rate, f"{name} ragged unit={unit} L/M={rate}")
        # bit for bit: every recording alone, in a tensor of its own length
        for b, n in enumerate(RAGGED):
            alone = SK.joints_from_tracks(torch.from_numpy(v[b:b + 1, :n].copy()).to(dev()), sk, mean=None if mean is None else torch.from_numpy(mean),
                                          unit=unit, fps=FPS[rate])
            alone = alone[0] if FPS[rate] is not None else alone
            assert torch.equal(got[b:b + 1, :alone.shape[1]], alone), (name, rate, b)


def test_draws_axis_equals_the_flattened_call():
    sk = skeleton("ted")
    U, R, T = 2, 2, TF + 1
    v = tracks(U * R, T, sk.K, 21).reshape(U, R, T, -1)
    frames = [T, 5]
    v[1, :, 5:] = np.nan
    mean = torch.from_numpy(mean_of(sk.K, 22))
    x = torch.from_numpy(v).to(dev())
    for fps in (None, (15, 25)):
        got, n_out = SK.joints_from_tracks(x, sk, frames=frames, mean=mean, fps=fps)
        flat, n_flat = SK.joints_from_tracks(x.reshape(U * R, T, -1), sk, frames=[T, T, 5, 5], mean=mean, fps=fps)
        assert got.shape[:2] == (U, R) and n_flat == [n for n in n_out for _ in range(R)]
        assert torch.equal(got.reshape(flat.shape), flat)
        Lf, M = SK.rate_ratio(fps)
        want = SN.joints(v.reshape(U * R, T, -1), table_of(sk), [T, T, 5, 5], mean.numpy().astype(np.float64), False, Lf, M)
        bound = SN.joints_bound(v.reshape(U * R, T, -1), table_of(sk), [T, T, 5, 5], mean.numpy().astype(np.float64), False, Lf, M)
        assert (np.abs(flat.cpu().numpy() - want) <= bound).all()


@pytest.mark.parametrize("rate", [(1, 1), (5, 3), (2, 3)])
@pytest.mark.parametrize("unit", [False, True])
def test_out_stride_batch_and_tile_do_not_change_the_bits(unit, rate):
    """(2, 3) needs more than TF + 2 source frames for a tile and so takes more than one pass."""
    sk = skeleton("ted")
    T = 2 * TF + 3
    x = torch.from_numpy(tracks(3, T, sk.K, 23)).to(dev())
    base = SK.launch_joints(x, sk, unit=unit, ratio=rate)
    t_out = base.shape[1]
    wide = torch.full((3, t_out + TF + 5, sk.J, 3), float("nan"), device=dev())
    SK.launch_joints(x, sk, unit=unit, ratio=rate, out=wide)
    assert torch.equal(wide[:, :t_out], base) and not wide[:, t_out:].any()
    for b in range(3):                                           # another batch, another place in it
        assert torch.equal(SK.launch_joints(x[b:b + 1].clone(), sk, unit=unit, ratio=rate), base[b:b + 1])
    assert torch.equal(SK.launch_joints(x.flip(0).contiguous(), sk, unit=unit, ratio=rate), base.flip(0))
    if rate == (1, 1):                                           # the same frames in another tile, at another place of it
        for s in (1, TF - 1, TF + 7):
            assert torch.equal(SK.launch_joints(x[:, s:].contiguous(), sk, unit=unit), base[:, s:])


@pytest.mark.parametrize("name", ["ted", "chain", "star", "random63"])
def test_inverse_against_float64(name):
    sk = skeleton(name)
    for i, T in enumerate(LENGTHS):
        B = 3 if i % 2 else 1
        p = (np.random.default_rng(50 + i).standard_normal((B, T, sk.J, 3)) * [0.01, 1.0, 30.0][i % 3]).astype(np.float32)
        mean = mean_of(sk.K, 60 + i) if i % 2 else None
        got = SK.dir_vec_from_joints(torch.from_numpy(p).to(dev()), sk, mean=None if mean is None else torch.from_numpy(mean))
        want = SN.dir_vec(p, table_of(sk), None, None if mean is None else mean.astype(np.float64))
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(f"{name} inverse T={T} B={B}: worst error {err / SN.U24:.2f} x 2^-24 (bound 5)")
        assert tuple(got.shape) == want.shape and err <= SN.INVERSE_BOUND
    # ragged, NaN behind every row's end, a zero-length bone; every recording alone bit for bit
    T = max(RAGGED) + 2
    p = np.random.default_rng(70).standard_normal((3, T, sk.J, 3)).astype(np.float32)
    p[2, 0, sk.children[0]] = p[2, 0, sk.parents[0]]
    for b, n in enumerate(RAGGED):
        p[b, n:] = np.nan
    got = SK.dir_vec_from_joints(torch.from_numpy(p).to(dev()), sk, frames=RAGGED)
    g = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and np.abs(g - SN.dir_vec(p, table_of(sk), RAGGED)).max() <= SN.INVERSE_BOUND
    assert not g[2, 0, :3].any()
    for b, n in enumerate(RAGGED):
        assert not g[b, n:].any()
        assert torch.equal(got[b:b + 1, :n], SK.dir_vec_from_joints(torch.from_numpy(p[b:b + 1, :n].copy()).to(dev()), sk))


def test_round_trip_on_the_device():
    sk = skeleton("ted")
    v = tracks(2, TF + 1, sk.K, 31)
    x = torch.from_numpy(v).to(dev())
    back = SK.dir_vec_from_joints(SK.joints_from_tracks(x, sk, unit=True), sk).cpu().numpy().astype(np.float64)
    v64 = v.astype(np.float64).reshape(2, TF + 1, sk.K, 3)
    unit = (v64 / np.linalg.norm(v64, axis=-1, keepdims=True)).reshape(v.shape)
    # the joints carry (d + 6) u S each; a bone is the difference of two of them divided by its length
    S = SN.joints_bound(v, table_of(sk), None, None, True).max()
    assert np.abs(back - unit).max() <= 2 * S / sk.lengths.min() + SN.INVERSE_BOUND


def test_graph_replay_equals_the_eager_call():
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    sk = skeleton("ted")
    v = tracks(3, max(RAGGED), sk.K, 33)
    x = torch.from_numpy(v).to(dev())
    mean = torch.from_numpy(mean_of(sk.K, 34)).to(dev())
    d_frames = torch.tensor(RAGGED, dtype=torch.int32, device=dev())
    eager = SK.launch_joints(x, sk, d_frames, mean=mean, unit=True, ratio=(5, 3))          # also the warm-up: the table is uploaded here
    eager_inv = SK.launch_dir_vec(eager, sk, mean=mean)
    out, out_inv = torch.full_like(eager, float("nan")), torch.full_like(eager_inv, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        SK.launch_joints(x, sk, d_frames, mean=mean, unit=True, ratio=(5, 3), out=out)
        SK.launch_dir_vec(out, sk, mean=mean, out=out_inv)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out_inv, eager_inv)


def test_drop_in_on_a_cuda_tensor_within_the_forward_bound_of_the_golden():
    from emotiongestures_amd.utils import data_utils_expressive as DU
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skeleton.npz"))
    sk = skeleton("ted")
    for tag in ("2d", "3d", "4d", "one_bone"):
        v = z[f"vec_{tag}"].astype(np.float32)
        got = DU.convert_dir_vec_to_pose(torch.from_numpy(v).to(dev()))
        want = z[f"pose_{tag}"]
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
        v3 = v.reshape(1, -1, 126)
        # the golden's inputs are stored as fp32 (the one-bone ones are exact 0 / 1) and the reference worked on them in float64: the cast
        # above changes nothing, the golden is the float64 definition on the values the kernel sees, and the forward bound holds as it is
        assert np.array_equal(v.astype(np.float64), z[f"vec_{tag}"].astype(np.float64))
        bound = SN.joints_bound(v3, table_of(sk)).reshape(want.shape)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= bound).all(), tag
    pose = z["pose_4d"].astype(np.float32)
    back = DU.convert_pose_seq_to_dir_vec(torch.from_numpy(pose).to(dev()))
    assert back.is_cuda and tuple(back.shape) == (2, 5, 42, 3)
    assert np.abs(back.cpu().numpy().astype(np.float64).reshape(1, 10, 126) - SN.dir_vec(pose.reshape(1, 10, 43, 3), table_of(sk))).max() <= SN.INVERSE_BOUND


# ---- the callers ---------------------------------------------------------------------------------------------------------------------------
def test_synthesize_joints_equal_the_function_on_its_track():
    model, vae = ted_models()
    sk = skeleton("ted")
    U, W = 2, 2
    g = inputs(U, W, 80)
    mean = torch.from_numpy(mean_of(sk.K, 81)).to(dev())
    # lengths=: recording 1 has one window fewer
    lens = [2 * HOP - 7, HOP - 5]
    audio = torch.from_numpy(synth_audio(U, max(lens), seed=80)).to(dev())
    kw = dict(labels=g["label"][:, 0].contiguous(), hop_samples=HOP, z=g["z"], lengths=lens)
    plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **kw)
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], joints=sk, joints_mean=mean, joints_unit=True, joints_fps=(15, 30), **kw)
    assert set(got) == set(plain) | {"joints", "joint_frames"} and torch.equal(got["track"], plain["track"])
    frames = [w * H_ + P_ for w in got["windows_per"]]
    assert got["windows_per"] == [2, 1] and got["joint_frames"] == [2 * n for n in frames]
    want, n_out = SK.joints_from_tracks(got["track"], sk, frames=frames, mean=mean, unit=True, fps=(15, 30))
    assert n_out == got["joint_frames"] and tuple(got["joints"].shape) == (U, 2 * (W * H_ + P_), 43, 3) and torch.equal(got["joints"], want)
    assert not got["joints"][1, n_out[1]:].any() and got["joints"][1, :n_out[1]].any()
    # draws=2, rectangular
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=82)).to(dev())
    zz = torch.from_numpy(np.random.default_rng(83).standard_normal((U, 2, W, 32)).astype(np.float32))
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], labels=g["label"], hop_samples=HOP, z=zz, draws=2, joints=sk)
    assert tuple(got["joints"].shape) == (U, 2, W * H_ + P_, 43, 3) and got["joint_frames"] == [W * H_ + P_] * U
    assert torch.equal(got["joints"], SK.joints_from_tracks(got["track"], sk))


def test_stream_last_joints_and_tail_joints():
    """Row 1 ends inside the first push (one window, valid at once); row 0 becomes valid with the second push: every step has a row that is
    not valid beside one that is.  Then a whole session against synthesize's track."""
    model, vae = ted_models()
    sk = skeleton("ted")
    U = 2
    g = inputs(U, 4, 80)
    mean = torch.from_numpy(mean_of(sk.K, 85)).to(dev())
    audio = torch.from_numpy(synth_audio(U, 3 * HOP, seed=86)).to(dev())
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=sk, joints_mean=mean, joints_unit=True)
    assert s.last_joints is None
    seen = []
    for k in range(3):
        rows, valid = s.push(audio[:, k * HOP:(k + 1) * HOP].contiguous(), g["text"][:, 0], g["label"][:, 0], g["z"][:, 0],
                             ends=[-1, 700] if k == 0 else None)
        v = valid.cpu().tolist()
        seen.append(v)
        assert rows is not None and tuple(s.last_joints.shape) == (U, H_, 43, 3)
        want, _n = SK.joints_from_tracks(rows, sk, frames=[H_ * a for a in v], mean=mean, unit=True)
        assert torch.equal(s.last_joints, want)
        for u in range(U):
            assert bool(s.last_joints[u].any()) == bool(v[u])
    assert seen == [[0, 1], [1, 0], [1, 0]]
    assert torch.equal(s.tail_joints(), SK.joints_from_tracks(s.tail(), sk, mean=mean, unit=True))
    # a whole session: pushes + tail_joints = the joints of synthesize's track
    T = 2 * HOP + N - 9000
    audio = torch.from_numpy(synth_audio(U, T, seed=80)).to(dev())
    padded = torch.zeros(U, 4 * HOP, device=dev())
    padded[:, :T] = audio
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=sk, joints_mean=mean)
    parts = []
    for k in range(1, 5):
        c = max(0, k - 2)
        rows, _v = s.push(padded[:, (k - 1) * HOP:k * HOP].contiguous(), g["text"][:, c], g["label"][:, c], g["z"][:, c], ends=T - 3 * HOP if k == 4 else None)
        assert (rows is None) == (s.last_joints is None) == (k == 1)
        if rows is not None:
            parts.append(s.last_joints)
    W = 3
    syn = Hs.synthesize((model, vae), audio, g["text"][:, :W].contiguous(), g["seed_pose"], labels=g["label"][:, :W].contiguous(), hop_samples=HOP,
                        z=g["z"][:, :W].contiguous(), windows=W, joints=sk, joints_mean=mean)
    got = torch.cat(parts + [s.tail_joints()], 1)
    assert got.shape == syn["joints"].shape and torch.equal(got, syn["joints"])
    assert torch.equal(syn["joints"], SK.joints_from_tracks(syn["track"], sk, mean=mean))
