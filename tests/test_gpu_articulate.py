"""Articulated bodies on the GPU (eg_articulate_forward / eg_articulate_rot6d through skeleton.joints_from_rot6d, rotations_from_rot6d,
rot6d_from_rotations and launch_articulate, harness.synthesize(joints=tree) and GestureStream(joints=tree)) against the float64 restatement
tests/articulate_np.py, and against itself bit for bit.

Tolerance: E32 is the largest element-wise deviation of the restatement run in fp32 (every intermediate rounded) from the restatement in
float64 on the test's own inputs; the device must be within 8 x E32 on every element (the factor covers another operation order and fused
multiply-adds).  Quaternions are compared up to sign.  Caps, so that the rule cannot grow unnoticed: 0 < 8 E32 <= 1e-4 for rotations and
0 < 8 E32 <= 1e-4 S for joints, S the longest summed |offset| along a root path (a position error is an angle error times a lever arm).
The one-joint body has p_0 = offsets[0] without any arithmetic: there E32 = 0 for the joints and the device has to be exact.  The accuracy
inputs keep min |a1| >= 0.25 and min |u2| >= 0.25, asserted from the float64 restatement: Gram-Schmidt is ill-conditioned below that.

Run as a program (``--hist-child``) this file is the child process of test_stream_graph_holds_one_launch_more: the launch histogram is
switched on by EG_LAUNCH_HIST=1 when the library is loaded, so reading it needs a process of its own."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import articulate_np as AN
import rollout_np as RO
import skeleton_np as SN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.builders import build_mirror
from emotiongestures_amd.synth import hash_uniform, load_synth_weights, synth_audio

pytestmark = pytest.mark.gpu

TF = SK.ARTICULATE_TILE_FRAMES
RATES = [(1, 1), (2, 1), (5, 3), (2, 3)]                 # L / M
FPS = {(1, 1): None, (2, 1): (15, 30), (5, 3): (15, 25), (2, 3): (15, 10)}
LENGTHS = [1, 2, TF - 1, TF, TF + 1, 2 * TF + 3]
RAGGED = [1, TF + 1, 2 * TF + 3]
NAMES = list(AN.BODIES)
FB, DB, PB, HOP = 60, 282, 10, 53333                      # the BEAT-shaped generator of the caller tests
HB, NS = FB - PB, (124 - 1) * 512
_TREES = {}
_MODELS = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def tree_of(name, basis="rows"):
    if (name, basis) not in _TREES:
        body = AN.BODIES[name]()
        _TREES[name, basis] = (body, SK.JointTree(*body, basis=basis))
    return _TREES[name, basis]


def mean_of(J, seed):
    return (np.random.default_rng(seed).standard_normal(6 * J) * 0.2).astype(np.float32)


def up_to_sign(a, b):
    return np.minimum(np.abs(a - b), np.abs(a + b))


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def beat_models():
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    if "beat" not in _MODELS:
        _MODELS["beat"] = (build_mirror("spatial", FB, DB, PB, 10, seed=31).to(dev()), load_synth_weights(MLP_Reconstruct_v3(), 31).eval().to(dev()))
    return _MODELS["beat"]


def beat_inputs(U, W, seed):
    inp = RO.rollout_inputs(U, W, FB, DB, PB, seed=seed)
    return {k: gpu(inp[k]) for k in ("text", "seed_pose", "label", "z")}


# ---- accuracy --------------------------------------------------------------------------------------------------------------------------------
def accuracy_cases(name, rate):
    """The inputs of one accuracy test: both bases, every length around the tile height, B = 1 and 3, the mean on and off; with the float64 and
    the fp32 restatement of the joints and of the rotations in both spaces.  Built without the GPU."""
    Lf, M = rate
    cases = []
    for basis in ("rows", "columns"):
        body, tree = tree_of(name, basis)
        cols = basis == "columns"
        for i, T in enumerate(LENGTHS):
            for B in (1, 3):
                mean = mean_of(tree.J, 40 + i) if (i + B) % 2 else None
                v = AN.rotation_tracks(tree.J, T, 100 * i + B + (7 if cols else 0), B=B, columns=cols, mean=mean)
                m64 = None if mean is None else mean.astype(np.float64)
                ref = {}
                for space in ("local", "global"):
                    j64, q64, (n1, n2) = AN.articulate(v, body, cols, None, m64, space, Lf, M, want_norms=True)
                    assert n1 >= 0.25 and n2 >= 0.25, (name, rate, basis, T, B, n1, n2)
                    j32, q32 = AN.articulate(v, body, cols, None, mean, space, Lf, M, dtype=np.float32)
                    ref[space] = (q64, q32)
                    ref["joints"] = (j64, j32)
                cases.append((f"{name} {basis} T={T} B={B} L/M={rate} mean={mean is not None}", tree, v, mean, ref))
    return cases


def e32_of(cases, key):
    dist = (lambda a, b: np.abs(a - b)) if key == "joints" else up_to_sign
    return max(float(dist(ref[key][1].astype(np.float64), ref[key][0]).max()) for _w, _t, _v, _m, ref in cases)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_joints_and_rotations_against_float64(name, rate):
    cases = accuracy_cases(name, rate)
    body, _tree = tree_of(name)
    S = AN.path_length(body)
    tol = {k: 8 * e32_of(cases, k) for k in ("joints", "local", "global")}
    assert 0 < tol["local"] <= 1e-4 and 0 < tol["global"] <= 1e-4, tol
    assert tol["joints"] <= 1e-4 * S and (tol["joints"] > 0 or name == "root"), (tol, S)     # one joint: p_0 = offsets[0], exact
    worst = dict.fromkeys(tol, 0.0)
    for what, tree, v, mean, ref in cases:
        x = gpu(v)
        mt = None if mean is None else torch.from_numpy(mean)
        got = {"joints": SK.joints_from_rot6d(x, tree, mean=mt, fps=FPS[rate]),
               "local": SK.rotations_from_rot6d(x, tree, mean=mt, fps=FPS[rate]),
               "global": SK.rotations_from_rot6d(x, tree, mean=mt, fps=FPS[rate], space="global")}
        for key, g in got.items():
            if FPS[rate] is not None:
                g, n_out = g
                assert n_out == [SN.out_frames(v.shape[1], *rate)] * v.shape[0]
            want = ref[key][0]
            assert g.shape == want.shape and g.dtype == torch.float32 and g.is_cuda, (what, key)
            g = g.cpu().numpy().astype(np.float64)
            assert np.isfinite(g).all(), (what, key)
            err = np.abs(g - want) if key == "joints" else up_to_sign(g, want)
            worst[key] = max(worst[key], float(err.max()))
            assert (err <= tol[key]).all(), (what, key, float(err.max()), tol[key])
            if key != "joints":
                assert (g[..., 0] >= 0).all() and np.abs(np.sqrt((g * g).sum(-1)) - 1).max() <= 1e-6, (what, key)
    print(f"{name} L/M={rate} S={S:.2f}: " + ", ".join(f"{k}: E32 {tol[k] / 8:.3e}, worst error {worst[k]:.3e}" for k in tol))


@pytest.mark.parametrize("basis", ["rows", "columns"])
def test_inverse_against_float64(basis):
    body, tree = tree_of("upper47", basis)
    cols = basis == "columns"
    J = tree.J
    rng = np.random.default_rng(11)
    T = 2 * 16 + 3                                               # the inverse walks tiles of 16 frames
    q = rng.standard_normal((3, T, J, 4)) * rng.uniform(0.5, 2.0, (3, T, J, 1))
    q = q.astype(np.float32)
    mean = mean_of(J, 12)
    frames = [1, 17, T]
    q[0, 1:] = np.nan
    q[1, 17:] = np.nan
    want = AN.rot6d(q, cols, frames, mean.astype(np.float64))
    E32 = float(np.abs(AN.rot6d(q, cols, frames, mean, dtype=np.float32).astype(np.float64) - want).max())
    assert 0 < 8 * E32 <= 1e-4
    got = SK.rot6d_from_rotations(gpu(q), tree, frames=frames, mean=torch.from_numpy(mean))
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (3, T, 6 * J) and torch.isfinite(got).all()
    g = got.cpu().numpy().astype(np.float64)
    err = float(np.abs(g - want).max())
    print(f"{basis}: E32 {E32:.3e}, worst error {err:.3e}")
    assert err <= 8 * E32
    for b, n in enumerate(frames):
        assert not got[b, n:].any() and got[b, :n].any()
        alone = SK.rot6d_from_rotations(gpu(q[b:b + 1, :n]), tree, mean=torch.from_numpy(mean))
        assert torch.equal(alone, got[b:b + 1, :n])
    # the draws axis shares frames[u]; no mean
    qq = gpu(np.nan_to_num(q[:2]).reshape(1, 2, T, J, 4))
    d = SK.rot6d_from_rotations(qq, tree, frames=[5])
    assert tuple(d.shape) == (1, 2, T, 6 * J) and not d[:, :, 5:].any() and d[0, 0, :5].any() and d[0, 1, :5].any()
    assert torch.equal(d[0, :, :5], SK.rot6d_from_rotations(qq[0, :, :5].contiguous(), tree))
    # and it inverts the forward kernel: the Gram-Schmidt rows of a track come back
    v = AN.rotation_tracks(J, TF + 1, 13, B=2, columns=cols)
    back = SK.rot6d_from_rotations(SK.rotations_from_rot6d(gpu(v), tree), tree).cpu().numpy().astype(np.float64)
    gs = np.concatenate(AN.gram_schmidt(v.astype(np.float64).reshape(2, TF + 1, J, 6))[:2], -1).reshape(2, TF + 1, 6 * J)
    assert np.abs(back - gs).max() <= 1e-5


def test_inverse_refuses_by_name():
    lib = L.load()
    _body, tree = tree_of("chain")
    q = torch.zeros(4 * 6 * 5 * 4 + 8, device=dev())
    out = torch.zeros(4 * 6 * 30 + 8, device=dev())
    n0 = lib.eg_launch_count()
    for args, word in (((q.data_ptr() + 4, 4, 6, 5, None, 1, 1, None, 0, out.data_ptr(), None), "input not 16-byte aligned"),
                       ((q.data_ptr(), 4, 6, 5, None, 1, 1, None, 0, out.data_ptr() + 8, None), "output not 16-byte aligned"),
                       ((q.data_ptr(), 4, 6, 5, None, 1, 1, None, 2, out.data_ptr(), None), "basis=2 (0: rows, 1: columns)"),
                       ((q.data_ptr(), 4, 6, 5, None, 3, 1, None, 0, out.data_ptr(), None), "rows=4 is not a multiple of draws=3")):
        assert lib.eg_articulate_rot6d(*args) != 0
        msg = lib.eg_last_error().decode()
        assert msg.startswith("eg_articulate_rot6d: ") and word in msg, msg
    assert lib.eg_launch_count() == n0


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_identity_is_exact_and_degenerate_groups_stay_finite(name):
    for basis in ("rows", "columns"):
        (parents, offsets), tree = tree_of(name, basis)
        J = tree.J
        ident = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (2, TF + 1, J))
        for rate in ((1, 1), (5, 3)):
            j, q = SK.launch_articulate(gpu(ident), tree, ratio=rate, space="global")
            assert np.array_equal(q.cpu().numpy(), np.broadcast_to(np.array([1, 0, 0, 0], np.float32), tuple(q.shape)))
            want = np.zeros((J, 3), np.float32)                       # the fp32 running sum of the offsets
            for k in range(J):
                want[k] = offsets[k].astype(np.float32) if parents[k] < 0 else want[parents[k]] + offsets[k].astype(np.float32)
            assert np.array_equal(j.cpu().numpy(), np.broadcast_to(want, tuple(j.shape)))
        zero = np.zeros((1, TF + 1, 6 * J), np.float32)
        par = np.tile(np.array([1, 2, 3, 2, 4, 6], np.float32), (1, TF + 1, J))
        mixed = AN.rotation_tracks(J, TF + 1, 3, columns=basis == "columns")
        mixed[:, ::2, :6] = 0                                         # a degenerate root above healthy joints
        for bad in (zero, par, mixed, 1e30 * par):
            for space in ("local", "global"):
                for rate in ((1, 1), (2, 3)):
                    j, q = SK.launch_articulate(gpu(bad), tree, ratio=rate, space=space)
                    assert torch.isfinite(j).all() and torch.isfinite(q).all(), (name, basis, space, rate)


# ---- ragged rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_ragged_rows_with_nan_behind_their_end(name, rate):
    T = max(RAGGED) + 2
    for basis, space in (("rows", "local"), ("columns", "global")):
        body, tree = tree_of(name, basis)
        cols = basis == "columns"
        mean = mean_of(tree.J, 9) if cols else None
        v = AN.rotation_tracks(tree.J, T, 8, B=len(RAGGED), columns=cols, mean=mean)
        for b, n in enumerate(RAGGED):
            v[b, n:] = np.nan
        mt = None if mean is None else torch.from_numpy(mean)
        x = gpu(v)
        gj, n_out = SK.joints_from_rot6d(x, tree, frames=RAGGED, mean=mt, fps=FPS[rate])
        gq, n_q = SK.rotations_from_rot6d(x, tree, frames=RAGGED, mean=mt, fps=FPS[rate], space=space)
        assert n_out == n_q == [SN.out_frames(n, *rate) for n in RAGGED] and torch.isfinite(gj).all() and torch.isfinite(gq).all()
        wj, wq = AN.articulate(v, body, cols, RAGGED, None if mean is None else mean.astype(np.float64), space, *rate)
        assert up_to_sign(gq.cpu().numpy().astype(np.float64), wq).max() <= 1e-4
        assert np.abs(gj.cpu().numpy().astype(np.float64) - wj).max() <= 1e-4 * max(1.0, AN.path_length(body))
        for b, n in enumerate(RAGGED):
            assert not gj[b, n_out[b]:].any() and not gq[b, n_out[b]:].any() and gq[b, :n_out[b]].any()
            # bit for bit: every row alone, in a tensor of its own length
            xa = gpu(v[b:b + 1, :n])
            aj, aq = SK.joints_from_rot6d(xa, tree, mean=mt, fps=FPS[rate]), SK.rotations_from_rot6d(xa, tree, mean=mt, fps=FPS[rate], space=space)
            aj, aq = (a[0] if FPS[rate] is not None else a for a in (aj, aq))
            assert aj.shape[1] == aq.shape[1] == n_out[b], (name, rate, b)
            assert torch.equal(gj[b:b + 1, :n_out[b]], aj) and torch.equal(gq[b:b + 1, :n_out[b]], aq), (name, rate, basis, b)


def test_draws_share_the_frames_of_their_recording():
    body, tree = tree_of("upper47")
    U, R, T = 2, 2, TF + 1
    v = AN.rotation_tracks(tree.J, T, 21, B=U * R).reshape(U, R, T, -1)
    v[1, :, 5:] = np.nan
    x = gpu(v)
    for fps in (None, (15, 25)):
        for f, tail in ((SK.joints_from_rot6d, 3), (SK.rotations_from_rot6d, 4)):
            got, n_out = f(x, tree, frames=[T, 5], fps=fps)
            flat, n_flat = f(x.reshape(U * R, T, -1), tree, frames=[T, T, 5, 5], fps=fps)
            assert tuple(got.shape) == (U, R, SK.out_frames(T, fps), tree.J, tail) and n_flat == [n for n in n_out for _ in range(R)]
            assert torch.equal(got.reshape(flat.shape), flat) and torch.isfinite(flat).all()
            assert not got[1, :, n_out[1]:].any() and got[1, 0, :n_out[1]].any() and got[1, 1, :n_out[1]].any()


# ---- one launch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [(1, 1), (5, 3), (2, 3)])
def test_one_launch_equals_the_two_single_output_launches(rate):
    lib = L.load()
    for name, basis, space in (("upper47", "rows", "local"), ("random64", "columns", "global")):
        _body, tree = tree_of(name, basis)
        v = AN.rotation_tracks(tree.J, max(RAGGED), 23, B=3, columns=basis == "columns")
        x, d_frames, mean = gpu(v), torch.tensor(RAGGED, dtype=torch.int32, device=dev()), gpu(mean_of(tree.J, 24))
        n0 = lib.eg_launch_count()
        j, q = SK.launch_articulate(x, tree, d_frames, mean=mean, space=space, ratio=rate)
        assert lib.eg_launch_count() - n0 == 1
        j1, none = SK.launch_articulate(x, tree, d_frames, mean=mean, space=space, ratio=rate, rotations=False)
        assert none is None
        none, q1 = SK.launch_articulate(x, tree, d_frames, mean=mean, space=space, ratio=rate, joints=False)
        assert none is None and torch.equal(j, j1) and torch.equal(q, q1) and j.any() and q.any()
        # out_stride, the batch and the place in it do not change the bits
        t_out = j.shape[1]
        wj = torch.full((3, t_out + TF + 5, tree.J, 3), float("nan"), device=dev())
        wq = torch.full((3, t_out + TF + 5, tree.J, 4), float("nan"), device=dev())
        SK.launch_articulate(x, tree, d_frames, mean=mean, space=space, ratio=rate, out_joints=wj, out_rotations=wq)
        assert torch.equal(wj[:, :t_out], j) and torch.equal(wq[:, :t_out], q) and not wj[:, t_out:].any() and not wq[:, t_out:].any()
        fj, fq = SK.launch_articulate(x.flip(0).contiguous(), tree, d_frames.flip(0).contiguous(), mean=mean, space=space, ratio=rate)
        assert torch.equal(fj, j.flip(0)) and torch.equal(fq, q.flip(0))


def test_graph_replay_equals_the_eager_call():
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    _body, tree = tree_of("upper47")
    x = gpu(AN.rotation_tracks(tree.J, max(RAGGED), 33, B=3))
    mean = gpu(mean_of(tree.J, 34))
    d_frames = torch.tensor(RAGGED, dtype=torch.int32, device=dev())
    SK.launch_articulate(x, tree, d_frames, mean=mean, space="global", ratio=(5, 3))                 # the warm-up: the table is uploaded here
    t_out = SK.out_frames(max(RAGGED), (3, 5))
    oj = torch.full((3, t_out, tree.J, 3), float("nan"), device=dev())
    oq = torch.full((3, t_out, tree.J, 4), float("nan"), device=dev())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        SK.launch_articulate(x, tree, d_frames, mean=mean, space="global", ratio=(5, 3), out_joints=oj, out_rotations=oq)
    x.copy_(gpu(AN.rotation_tracks(tree.J, max(RAGGED), 35, B=3)))                                   # new input, new lengths
    d_frames.copy_(torch.tensor([TF, 2, max(RAGGED)], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    ej, eq = SK.launch_articulate(x, tree, d_frames, mean=mean, space="global", ratio=(5, 3))
    assert torch.equal(oj, ej) and torch.equal(oq, eq) and torch.isfinite(oj).all() and oq[1, :4].any() and not oq[1, 4:].any()


# ---- the callers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["alone", "draws", "takes", "fps", "smooth"])
def test_synthesize_with_a_joint_tree_equals_the_functions_on_its_track(case):
    model, vae = beat_models()
    _body, tree = tree_of("upper47")
    U, W = 2, 3
    g = beat_inputs(U, W, 120)
    mean = gpu(mean_of(tree.J, 81))
    lengths = [3 * HOP - 100, HOP + 700]                                                            # 3 and 2 windows
    audio = gpu(synth_audio(U, max(lengths), seed=80))
    zz = torch.from_numpy(hash_uniform("articulate/z", (U, 2, W, 32), -2.0, 2.0, 121))
    kw = dict(hop_samples=HOP, joints=tree, joints_mean=mean, rotations=True)
    fn, fps, space = Hs.synthesize, None, "local"
    if case == "alone":
        kw.update(labels=g["label"][:, 0].contiguous(), z=g["z"], lengths=lengths, rotations_space="global")
        space = "global"
    elif case == "draws":
        audio = audio[:, :2 * HOP + NS].contiguous()
        kw.update(labels=g["label"], z=zz, draws=2)
    elif case == "takes":
        fn = Hs.synthesize_takes
        kw.update(labels=g["label"][:, 0].contiguous(), z=zz, draws=2, lengths=lengths)
    elif case == "fps":
        kw.update(labels=g["label"][:, 0].contiguous(), z=g["z"], lengths=lengths, joints_fps=(15, 30))
        fps = (15, 30)
    else:
        kw.update(labels=g["label"][:, 0].contiguous(), z=g["z"], lengths=lengths, smooth=(9, 3))
    out = fn((model, vae), audio, g["text"], g["seed_pose"], **kw)
    lead = (U, 2) if case in ("draws", "takes") else (U,)
    wp = out["windows_per"] if "windows_per" in out else [W] * U
    frames = [w * HB + PB for w in wp]
    poses = out["track_smooth"] if case == "smooth" else out["track"]
    assert ("track_smooth" in out) == (case == "smooth") and tuple(poses.shape[:-2]) == lead
    wj, n_out = SK.joints_from_rot6d(poses, tree, frames=frames, mean=mean, fps=fps)
    wq, _n = SK.rotations_from_rot6d(poses, tree, frames=frames, mean=mean, fps=fps, space=space)
    assert out["joint_frames"] == n_out == [SK.out_frames(n, fps) for n in frames]
    assert tuple(out["joints"].shape) == lead + (SK.out_frames(poses.shape[-2], fps), 47, 3) and tuple(out["rotations"].shape) == lead + (wj.shape[-3], 47, 4)
    assert torch.equal(out["joints"], wj) and torch.equal(out["rotations"], wq)
    assert torch.isfinite(wj).all() and (wq[..., 0] >= 0).all() and wq[0].any()
    if case != "draws":
        assert wp == [3, 2] and not out["joints"][1, ..., n_out[1]:, :, :].any() and not out["rotations"][1, ..., n_out[1]:, :, :].any()
    if case == "alone":                                                                             # without rotations=: the same joints, no rotations
        del kw["rotations"], kw["rotations_space"]
        plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **kw)
        assert set(out) == set(plain) | {"rotations"} and torch.equal(plain["joints"], out["joints"]) and torch.equal(plain["track"], out["track"])


def test_ted_generator_refuses_a_tree_of_another_width():
    from skeleton_gpu_common import inputs, ted_models
    model, vae = ted_models()
    _body, tree = tree_of("upper47")
    g = inputs(2, 2, 80)
    audio = gpu(synth_audio(2, 32000 + (124 - 1) * 512, seed=82))
    with pytest.raises(L.EgError, match=r"synthesize: joints=: the joint tree has J=47 joints, 6J=282 != pose_dim=126"):
        Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], labels=g["label"], hop_samples=32000, z=g["z"], joints=tree)
    with pytest.raises(L.EgError, match=r"GestureStream: joints=: the joint tree has J=47 joints, 6J=282 != pose_dim=126"):
        Hs.open_stream((model, vae), 2, g["seed_pose"], hop_samples=32000, joints=tree, rotations=True)


def test_stream_last_joints_last_rotations_and_the_tails():
    model, vae = beat_models()
    _body, tree = tree_of("upper47")
    U = 2
    g = beat_inputs(U, 4, 120)
    mean = gpu(mean_of(tree.J, 85))
    T = 2 * HOP + NS - 9000
    audio = gpu(synth_audio(U, T, seed=80))
    padded = torch.zeros(U, 4 * HOP, device=dev())
    padded[:, :T] = audio
    with pytest.raises(L.EgError, match="GestureStream: joints_fps= is not supported"):
        Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=tree, joints_fps=(15, 30))
    with pytest.raises(L.EgError, match="GestureStream: smooth= together with joints= is not supported"):
        Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=tree, smooth=(9, 3))
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=tree, joints_mean=mean, rotations=True, rotations_space="global")
    assert s.last_joints is None and s.last_rotations is None
    emitted = 0
    for k in range(1, 5):
        c = max(0, k - 2)
        rows, valid = s.push(padded[:, (k - 1) * HOP:k * HOP].contiguous(), g["text"][:, c], g["label"][:, c], g["z"][:, c], ends=T - 3 * HOP if k == 4 else None)
        assert (rows is None) == (s.last_joints is None) == (s.last_rotations is None) == (k == 1)
        if rows is not None:
            emitted += 1
            assert tuple(s.last_joints.shape) == (U, HB, 47, 3) and tuple(s.last_rotations.shape) == (U, HB, 47, 4)
            wj, wq = SK.launch_articulate(rows.contiguous(), tree, valid, 1, HB, mean, "global")
            assert torch.equal(s.last_joints, wj) and torch.equal(s.last_rotations, wq) and wq.any()
    assert emitted == 3
    tj, tq = SK.launch_articulate(s.tail().contiguous(), tree, None, 1, 1, mean, "global")
    assert torch.equal(s.tail_joints(), tj) and torch.equal(s.tail_rotations(), tq) and tuple(tj.shape) == (U, PB, 47, 3)
    # a row that is not valid in a step has zero joints and rotations; joints alone leave last_rotations None
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=tree)
    short = gpu(synth_audio(U, HOP, seed=86))
    rows, valid = s.push(short, g["text"][:, 0], g["label"][:, 0], g["z"][:, 0], ends=[-1, 700])
    assert valid.cpu().tolist() == [0, 1] and not s.last_joints[0].any() and s.last_joints[1].any() and s.last_rotations is None
    assert torch.equal(s.last_joints, SK.launch_articulate(rows.contiguous(), tree, valid, 1, HB, rotations=False)[0])
    with pytest.raises(L.EgError, match="tail_rotations: the session was opened without rotations"):
        s.tail_rotations()


def test_stream_graph_holds_one_launch_more():
    """The launch histogram of a session's first emitting push -- two warm-up runs and the capture of the step (GestureStream._capture), or the
    one run of an eager session -- without and with joints=tree, rotations=True: the same launches, plus one articulate_forward per run."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EG_LAUNCH_HIST="1", PYTHONPATH=os.pathsep.join([root, os.path.dirname(os.path.abspath(__file__))]))
    res = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--hist-child"], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    hist = json.loads(next(line for line in res.stdout.splitlines() if line.startswith("HIST "))[5:])
    for mode, runs in (("graph", 3), ("eager", 1)):
        without, with_ = hist[mode]
        assert without and "articulate_forward" not in without
        assert with_ == dict(without, articulate_forward=runs), (mode, without, with_)


def _hist_child():
    def histogram(reset):
        lib = L.load()
        buf = C.create_string_buffer(int(lib.eg_launch_histogram(None, 0, 0)) + 64)
        lib.eg_launch_histogram(buf, len(buf), int(reset))
        return {k: int(n) for k, n in (line.rsplit(" ", 1) for line in buf.value.decode().splitlines())}

    model, vae = beat_models()
    _body, tree = tree_of("upper47")
    U = 2
    g = beat_inputs(U, 2, 120)
    audio = gpu(synth_audio(U, 2 * HOP, seed=5))
    out = {}
    for mode, graph in (("graph", True), ("eager", False)):
        out[mode] = []
        for kw in ({}, dict(joints=tree, rotations=True)):
            s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, graph=graph, **kw)
            if kw:
                tree.table(dev())                                 # the table's upload is no launch of the library, but keep it out of the step
            torch.cuda.synchronize()
            histogram(True)
            emitted = []
            for k in range(2):
                rows, _valid = s.push(audio[:, k * HOP:(k + 1) * HOP].contiguous(), g["text"][:, 0], g["label"][:, 0], g["z"][:, 0])
                emitted.append(rows is not None)
            torch.cuda.synchronize()
            assert emitted == [False, True], emitted
            out[mode].append(histogram(True))
            s.close()
    print("HIST " + json.dumps(out))


if __name__ == "__main__" and sys.argv[1:] == ["--hist-child"]:
    _hist_child()
