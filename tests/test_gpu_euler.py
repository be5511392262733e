"""Euler channels on the GPU (eg_articulate_euler / eg_articulate_rot6d_euler / eg_angle_unwrap through skeleton.euler_from_rot6d,
rot6d_from_euler, unwrap_angles and the launch_* forms) against the float64 restatement tests/euler_np.py, and against itself bit for bit.

Tolerance: E32 is the largest deviation of the restatement run in fp32 (every intermediate rounded) from the restatement in float64 on the
test's own inputs; the device must be within 8 x E32 (the factor of the articulate tests: another operation order, fused multiply-adds, another
library's atan2 / sincos).  E32 is taken in two spaces.  Matrix space: R_i(a) R_j(b) R_k(c) rebuilt in float64 from the angles against the
float64 matrices of the definition; every frame counts.  Angle space, modulo 360 degrees: the joint-frames with |cos b| >= 0.05 in float64 only
(towards the lock a and c are ill-conditioned as 1 / cos b, and at it only their sum or difference means anything).  Joint-frames with 1 - |s|
inside [2^-21, 2^-19], where fp32 and float64 may pick different branches, are checked for finiteness only.  Conditions on the inputs are
asserted from the float64 restatement before the device runs.  The unwrap is exact: integer counts, one rounding.

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
import euler_np as EN
import rollout_np as RO
import skeleton_np as SN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import bvh as BVH
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.builders import build_mirror
from emotiongestures_amd.synth import hash_uniform, load_synth_weights, synth_audio

pytestmark = pytest.mark.gpu

TF = SK.ARTICULATE_TILE_FRAMES
UT = SK.UNWRAP_TILE_FRAMES
RATES = [(1, 1), (2, 1), (5, 3), (2, 3)]                 # L / M
FPS = {(1, 1): None, (2, 1): (15, 30), (5, 3): (15, 25), (2, 3): (15, 10)}
LENGTHS = [1, 2, TF - 1, TF, TF + 1, 2 * TF + 3]
NAMES = list(AN.BODIES)
FB, DB, PB, HOP = 60, 282, 10, 53333                      # the BEAT-shaped generator of the caller tests
HB, NS = FB - PB, (124 - 1) * 512
_TREES = {}
_BOUNDS = {}
_MODELS = {}


def beat_models():
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    if "beat" not in _MODELS:
        _MODELS["beat"] = (build_mirror("spatial", FB, DB, PB, 10, seed=31).to(dev()), load_synth_weights(MLP_Reconstruct_v3(), 31).eval().to(dev()))
    return _MODELS["beat"]


def beat_inputs(U, W, seed):
    inp = RO.rollout_inputs(U, W, FB, DB, PB, seed=seed)
    return {k: gpu(inp[k]) for k in ("text", "seed_pose", "label", "z")}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def tree_of(name, basis="rows"):
    if (name, basis) not in _TREES:
        _TREES[name, basis] = SK.JointTree(*AN.BODIES[name](), basis=basis)
    return _TREES[name, basis]


def mean_of(J, seed):
    return (np.random.default_rng(seed).standard_normal(6 * J) * 0.2).astype(np.float32)


def names_of(codes):
    return [EN.ORDERS[c] for c in codes]


def mod_period(d, period):
    return (d + period / 2) % period - period / 2


def rebuilt(e, codes, degrees):
    return EN.matrices_of_euler_product(np.asarray(e, np.float64), codes, degrees)


# ---- accuracy --------------------------------------------------------------------------------------------------------------------------------
def accuracy_cases(name, rate):
    """Both bases, every length around the tile height, B = 1 and 3, the mean on and off, degrees and radians, all six orders one per joint
    cyclically; with the float64 and the fp32 restatement.  Built without the GPU."""
    Lf, M = rate
    cases = []
    for basis in ("rows", "columns"):
        tree = tree_of(name, basis)
        cols = basis == "columns"
        codes = EN.orders_cyclic(tree.J)
        for i, T in enumerate(LENGTHS):
            for B in (1, 3):
                mean = mean_of(tree.J, 40 + i) if (i + B) % 2 else None
                degrees = bool((i + B + cols) % 2)
                v = AN.rotation_tracks(tree.J, T, 100 * i + B + (7 if cols else 0), B=B, columns=cols, mean=mean)
                m64 = None if mean is None else mean.astype(np.float64)
                e64, R64, s64, (n1, n2) = EN.euler(v, codes, cols, None, m64, Lf, M, degrees, want=True)
                assert n1 >= 0.25 and n2 >= 0.25, (name, rate, basis, T, B, n1, n2)
                e32 = EN.euler(v, codes, cols, None, mean, Lf, M, degrees, dtype=np.float32)
                cases.append(dict(what=f"{name} {basis} T={T} B={B} L/M={rate} mean={mean is not None} degrees={degrees}", tree=tree, v=v,
                                  mean=mean, codes=codes, degrees=degrees, e64=e64, R64=R64, s64=s64, e32=e32))
    return cases


def masks(c):
    """(angle-space joint-frames, joint-frames near the branch threshold) of a case, from float64."""
    b = c["e64"][..., 1]
    cosb = np.cos(np.radians(b) if c["degrees"] else b)
    gap = 1.0 - np.abs(c["s64"])
    return np.abs(cosb) >= 0.05, (gap >= 2.0 ** -21) & (gap <= 2.0 ** -19)


def errors(e, c):
    """(matrix-space error [B, T, J], angle-space error [B, T, J] in radians) of angles e against the case's float64."""
    period = 360.0 if c["degrees"] else 2 * np.pi
    em = np.abs(rebuilt(e, c["codes"], c["degrees"]) - c["R64"]).max(-1)
    ea = np.abs(mod_period(np.asarray(e, np.float64) - c["e64"], period)).max(-1)
    return em, (np.radians(ea) if c["degrees"] else ea)


def bounds_of(cases):
    """8 x E32 in both spaces, and the conditions of the docstring."""
    e_m = e_a = 0.0
    total = out = near = 0
    for c in cases:
        ok, band = masks(c)
        em, ea = errors(c["e32"], c)
        keep = ~band
        e_m = max(e_m, float(em[keep].max()))
        e_a = max(e_a, float(ea[ok & keep].max()) if (ok & keep).any() else 0.0)
        total, out, near = total + ok.size, out + int((~ok).sum()), near + int(band.sum())
    assert out <= 0.01 * total, ("the angle-space check leaves out too much", out, total)
    assert near <= 0.001 * total, ("too many joint-frames at the branch threshold", near, total)
    assert e_m > 0 and e_a > 0, (e_m, e_a)
    return 8 * e_m, 8 * e_a


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_euler_against_float64(name, rate):
    cases = accuracy_cases(name, rate)
    tol_m, tol_a = bounds_of(cases)
    _BOUNDS[name, rate] = (tol_m, tol_a)
    worst_m = worst_a = 0.0
    for c in cases:
        mt = None if c["mean"] is None else torch.from_numpy(c["mean"])
        g = SK.euler_from_rot6d(gpu(c["v"]), c["tree"], names_of(c["codes"]), mean=mt, fps=FPS[rate], degrees=c["degrees"])
        if FPS[rate] is not None:
            g, n_out = g
            assert n_out == [SN.out_frames(c["v"].shape[1], *rate)] * c["v"].shape[0]
        assert g.shape == c["e64"].shape and g.dtype == torch.float32 and g.is_cuda, c["what"]
        g = g.cpu().numpy()
        assert np.isfinite(g).all(), c["what"]
        ok, band = masks(c)
        em, ea = errors(g, c)
        worst_m, worst_a = max(worst_m, float(em[~band].max())), max(worst_a, float(ea[ok & ~band].max(initial=0.0)))
        assert (em[~band] <= tol_m).all(), (c["what"], "matrix space", float(em[~band].max()), "bound 8 E32 =", tol_m, "angle bound", tol_a)
        assert (ea[ok & ~band] <= tol_a).all(), (c["what"], "angle space (rad)", float(ea[ok & ~band].max()), "bound 8 E32 =", tol_a, "matrix bound", tol_m)
        lim = 90.0 if c["degrees"] else np.pi / 2
        assert (np.abs(g[..., 1]) <= np.float32(lim)).all(), c["what"]
    print(f"euler {name} L/M={rate}: matrix space worst {worst_m:.3e} (8 E32 = {tol_m:.3e}); angle space worst {worst_a:.3e} rad (8 E32 = {tol_a:.3e} rad)")


@pytest.mark.parametrize("name", NAMES)
def test_inverse_against_float64(name):
    worst = tol = 0.0
    runs = []
    for basis in ("rows", "columns"):
        tree = tree_of(name, basis)
        cols = basis == "columns"
        codes = EN.orders_cyclic(tree.J)
        for i, T in enumerate([1, 15, 16, 17, 35]):
            B = 1 + i % 3
            degrees = bool(i % 2)
            rng = np.random.default_rng(300 + i + 10 * cols)
            e = rng.uniform(-np.pi, np.pi, (B, T, tree.J, 3))
            e[..., 1] = rng.uniform(-np.pi / 2, np.pi / 2, (B, T, tree.J))
            e = (np.degrees(e) if degrees else e).astype(np.float32)
            mean = mean_of(tree.J, 60 + i) if i % 2 == 0 else None
            d64 = EN.rot6d(e.astype(np.float64), codes, cols, None, None if mean is None else mean.astype(np.float64), degrees)
            d32 = EN.rot6d(e, codes, cols, None, mean, degrees, dtype=np.float32)
            tol = max(tol, 8 * float(np.abs(d32.astype(np.float64) - d64).max()))
            runs.append((tree, codes, e, mean, degrees, d64))
    assert 0 < tol <= 1e-4, tol
    for tree, codes, e, mean, degrees, d64 in runs:
        got = SK.rot6d_from_euler(gpu(e), tree, names_of(codes), mean=None if mean is None else torch.from_numpy(mean), degrees=degrees)
        assert got.shape == d64.shape and got.dtype == torch.float32 and got.is_cuda
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - d64).max())
        worst = max(worst, err)
        assert err <= tol, (name, e.shape, degrees, err, "bound 8 E32 =", tol)
    print(f"inverse {name}: worst {worst:.3e} (8 E32 = {tol:.3e})")


@pytest.mark.parametrize("basis", ["rows", "columns"])
def test_round_trip_on_orthonormal_input(basis):
    tree = tree_of("upper47", basis)
    codes = EN.orders_cyclic(tree.J)
    v = AN.rotation_tracks(tree.J, 2 * TF + 3, 77, B=2, columns=basis == "columns")
    m = AN.matrices(v.astype(np.float64).reshape(2, -1, tree.J, 6), basis == "columns").reshape(2, -1, tree.J, 3, 3)
    if basis == "columns":
        m = np.swapaxes(m, -1, -2)
    x = np.ascontiguousarray(m[..., :2, :]).reshape(v.shape).astype(np.float32)       # orthonormal up to fp32 rounding
    e64 = EN.euler(x, codes, basis == "columns")
    back32 = EN.rot6d(EN.euler(x, codes, basis == "columns", dtype=np.float32), codes, basis == "columns", dtype=np.float32)
    tol = 8 * float(np.abs(back32.astype(np.float64) - x).max())
    assert 0 < tol <= 1e-4
    e = SK.euler_from_rot6d(gpu(x), tree, names_of(codes))
    back = SK.rot6d_from_euler(e, tree, names_of(codes)).cpu().numpy().astype(np.float64)
    assert np.abs(back - x).max() <= tol, (float(np.abs(back - x).max()), tol)
    assert e64.shape == tuple(e.shape)


# ---- special inputs ----------------------------------------------------------------------------------------------------------------------------
def test_lock_branch_identity_and_degenerate_groups():
    tree = tree_of("chain")
    J = tree.J
    tol_m = 8 * 2.0 ** -23                                                         # the matrix bound of exact inputs: a few fp32 roundings of 1
    for code, o in enumerate(EN.ORDERS):
        i, j, k, eps = EN.axes(code)
        for sign in (1, -1):
            for degrees in (True, False):
                # R with R[i][k] = eps sign: rows e_i -> sign eps e_k, the rest a signed permutation with det +1; exact in both precisions
                R = np.zeros((3, 3))
                R[i, k] = eps * sign
                R[j, j] = 1.0
                R[k, i] = -eps * sign
                assert abs(np.linalg.det(R) - 1.0) < 1e-15
                x = np.tile(R[:2].reshape(6), (1, 3, J)).astype(np.float32)
                e64, _R64, s64, _n = EN.euler(x, [code] * J, want=True, degrees=degrees)
                assert (s64 == sign).all()
                g = SK.euler_from_rot6d(gpu(x), tree, o, degrees=degrees).cpu().numpy()
                quarter = np.float32(90.0) if degrees else np.float32(np.pi / 2)
                assert (g[..., 2] == 0).all() and (g[..., 1] == sign * quarter).all(), (o, sign, degrees, g[0, 0])
                assert np.abs(rebuilt(g, [code] * J, degrees) - R.reshape(9)).max() <= tol_m, (o, sign)
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (2, TF + 1, J))
    for tr in (tree, tree_of("chain", "columns")):
        g = SK.euler_from_rot6d(gpu(ident), tr, names_of(EN.orders_cyclic(J))).cpu().numpy()
        assert (g == 0).all()
    bad = np.zeros((1, 4, 6 * J), np.float32)
    bad[0, 1] = np.tile(np.array([1, 2, 3, 2, 4, 6], np.float32), J)              # a1 parallel to a2
    bad[0, 2] = np.tile(np.array([0, 0, 0, 1, 0, 0], np.float32), J)
    bad[0, 3] = np.tile(np.array([1e-20, 0, 0, 0, 1e-20, 0], np.float32), J)
    g = SK.euler_from_rot6d(gpu(bad), tree, names_of(EN.orders_cyclic(J)))
    assert torch.isfinite(g).all()
    assert torch.isfinite(SK.rot6d_from_euler(g, tree, names_of(EN.orders_cyclic(J)))).all()


@pytest.mark.parametrize("rate", [(1, 1), (5, 3), (2, 3)])
def test_ragged_rows_and_draws(rate):
    tree = tree_of("star")
    J, T, U, R = tree.J, 2 * TF + 3, 4, 3
    codes = EN.orders_cyclic(J)
    frames = [T, TF + 1, 1, 0]
    v = AN.rotation_tracks(J, T, 5, B=U)
    full = np.repeat(v[:, None], R, 1).copy()
    full[:, 1:] += np.float32(0.01) * np.arange(1, R, dtype=np.float32)[None, :, None, None]
    dirty = full.copy()
    for u, n in enumerate(frames):
        dirty[u, :, n:] = np.nan                                                   # nothing behind a row's end is read
    g, n_out = SK.euler_from_rot6d(gpu(dirty), tree, names_of(codes), frames=frames, fps=FPS[rate])
    assert n_out == [SN.out_frames(n, *rate) for n in frames]
    g = g.cpu().numpy()
    assert np.isfinite(g).all() and g.shape == (U, R, SN.out_frames(T, *rate), J, 3)
    for u, n in enumerate(frames):
        assert (g[u, :, n_out[u]:] == 0).all()
        for r in range(R):
            if n:                                                                  # a row alone, cut to its own frames: the same bits
                alone = SK.euler_from_rot6d(gpu(full[u, r, :n]), tree, names_of(codes), fps=FPS[rate])
                alone = (alone[0] if FPS[rate] is not None else alone).cpu().numpy()
                assert np.array_equal(g[u, r, :n_out[u]], alone), (u, r)
    # the inverse: zeros behind a row's end, NaN there never read
    e = np.where(np.isnan(g), 0, g)
    e_dirty = g.copy()
    for u in range(U):
        e_dirty[u, :, n_out[u]:] = np.nan
    back = SK.rot6d_from_euler(gpu(e_dirty), tree, names_of(codes), frames=n_out).cpu().numpy()
    assert np.isfinite(back).all()
    for u in range(U):
        assert (back[u, :, n_out[u]:] == 0).all()
        if n_out[u]:
            assert np.array_equal(back[u, :, :n_out[u]], SK.rot6d_from_euler(gpu(e[u, :, :n_out[u]]), tree, names_of(codes)).cpu().numpy())


def test_refusals_by_name():
    tree = tree_of("chain")
    x = gpu(AN.rotation_tracks(tree.J, 4, 1))
    with pytest.raises(L.EgError, match="repeats an axis"):
        SK.euler_from_rot6d(x, tree, "XYX")
    with pytest.raises(L.EgError, match="need one of"):
        SK.euler_from_rot6d(x, tree, ["XYZ"] * (tree.J - 1) + ["xyw"])
    with pytest.raises(L.EgError, match="6J=30 columns"):
        SK.euler_from_rot6d(x[..., :24], tree, "XYZ")
    with pytest.raises(L.EgError, match="euler shape"):
        SK.rot6d_from_euler(x, tree, "XYZ")
    with pytest.raises(L.EgError, match="period="):
        SK.unwrap_angles(x, period=float("inf"))


# ---- unwrap ------------------------------------------------------------------------------------------------------------------------------------
def wrap32(walk, period):
    """A float64 walk wrapped into [-period / 2, period / 2) and rounded to fp32: what a principal-value kernel hands the filter."""
    return ((walk + period / 2) % period - period / 2).astype(np.float32)


def unwrap_series(T, C, seed, period):
    """Five full turns and back, random walks, and jumps placed on the first and on the last frame of a tile."""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.uniform(-0.45, 0.45, (T, C)) * period, axis=0)
    walk[:, 0] = np.linspace(0.0, 5.0 * period, T) + 0.01 * period
    p = wrap32(walk, period)
    if C > 2:
        p[:, 1] = np.float32(0.4 * period) * np.where(np.arange(T) % UT == 0, -1, 1)          # a jump into and out of the first frame of every tile
        p[:, 2] = np.float32(0.4 * period) * np.where(np.arange(T) % UT == UT - 1, -1, 1)     # ... of the last frame
    return p


@pytest.mark.parametrize("period", [360.0, 2 * np.pi])
@pytest.mark.parametrize("T", [1, 2, UT - 1, UT, UT + 1, 3 * UT + 1])
def test_unwrap_bit_for_bit(T, period):
    p = np.stack([unwrap_series(T, 141, 9 + b, period) for b in range(3)])
    ref = EN.unwrap(p, None, period)
    got = SK.unwrap_angles(gpu(p), period=period)
    assert got.dtype == torch.float32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (T, period)
    if T > 2:
        assert np.abs(np.diff(ref.astype(np.float64), axis=1)).max() <= 0.5 * period * (1 + 1e-6)
        assert ref[:, -1, 0].min() > 4.9 * period                                  # the five turns are there
    if T == 3 * UT + 1:                                                            # ragged rows, NaN behind their end, one draw axis, frames = 1 and 0
        frames = [T, UT + 1, 1, 0]
        q = np.stack([np.stack([unwrap_series(T, 7, 50 + 2 * u + r, period) for r in range(2)]) for u in range(4)])
        for u, n in enumerate(frames):
            q[u, :, n:] = np.nan
        ref = EN.unwrap(q.reshape(8, T, 7), [n for n in frames for _ in range(2)], period).reshape(q.shape)
        got = SK.unwrap_angles(gpu(q), frames=frames, period=period).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        for u, n in enumerate(frames):
            assert np.isfinite(got[u, :, :n]).all() and np.isnan(got[u, :, n:]).all()


@pytest.mark.parametrize("degrees", [True, False])
def test_euler_with_unwrap_equals_the_two_calls(degrees):
    tree = tree_of("upper47")
    codes = EN.orders_cyclic(tree.J)
    T, frames = 2 * UT + 5, [2 * UT + 5, UT + 3, 1]
    v = gpu(AN.rotation_tracks(tree.J, T, 123, B=3, cap_deg=179.0))
    for fps in (None, (15, 25)):
        one, n1 = SK.euler_from_rot6d(v, tree, names_of(codes), frames=frames, fps=fps, degrees=degrees, unwrap=True)
        e, n2 = SK.euler_from_rot6d(v, tree, names_of(codes), frames=frames, fps=fps, degrees=degrees)
        two = SK.unwrap_angles(e.reshape(3, e.shape[1], -1), frames=n2, period=360.0 if degrees else 2 * np.pi).reshape(e.shape)
        assert n1 == n2 and torch.equal(one, two)
        ref = EN.unwrap(e.cpu().numpy().reshape(3, e.shape[1], -1), n2, 360.0 if degrees else 2 * np.pi).reshape(e.shape)
        assert np.array_equal(one.cpu().numpy().view(np.uint32), ref.view(np.uint32))


# ---- the siblings ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [(1, 1), (5, 3)])
def test_agrees_with_the_local_quaternions(rate):
    """The rotation rebuilt from the Euler angles and rotations_from_rot6d's local quaternion of the same call: within the sum of the two
    tests' bounds (8 E32 of each against the shared float64 matrices), in matrix space."""
    name = "upper47"
    tree = tree_of(name)
    body = AN.BODIES[name]()
    codes = EN.orders_cyclic(tree.J)
    Lf, M = rate
    v = AN.rotation_tracks(tree.J, 2 * TF + 3, 31, B=2)
    e64, R64, s64, _n = EN.euler(v, codes, False, None, None, Lf, M, True, want=True)
    e32 = EN.euler(v, codes, False, None, None, Lf, M, True, dtype=np.float32)
    _j, q64 = AN.articulate(v, body, False, None, None, "local", Lf, M)
    _j, q32 = AN.articulate(v, body, False, None, None, "local", Lf, M, dtype=np.float32)
    tol_e = 8 * float(np.abs(rebuilt(e32, codes, True) - R64).max())
    tol_q = 8 * float(np.abs(AN.quat_matrix(q32.astype(np.float64)) - AN.quat_matrix(q64)).max())
    assert tol_e > 0 and tol_q > 0
    x = gpu(v)
    e = SK.euler_from_rot6d(x, tree, names_of(codes), fps=FPS[rate])
    q = SK.rotations_from_rot6d(x, tree, fps=FPS[rate])
    if FPS[rate] is not None:
        e, q = e[0], q[0]
    qn = q.cpu().numpy().astype(np.float64)
    qn = qn / np.linalg.norm(qn, axis=-1, keepdims=True)
    diff = float(np.abs(rebuilt(e.cpu().numpy(), codes, True) - AN.quat_matrix(qn)).max())
    assert diff <= tol_e + tol_q, (diff, tol_e, tol_q)


# ---- launch forms and graphs ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_the_eager_call():
    tree = tree_of("upper47")
    codes = names_of(EN.orders_cyclic(tree.J))
    B, T = 3, 2 * UT + 5
    x = gpu(AN.rotation_tracks(tree.J, T, 8, B=B))
    d_frames = torch.tensor([T, UT + 1, 7], dtype=torch.int32, device=dev())
    out = torch.empty(B, T, tree.J, 3, device=dev())
    ws = SK.unwrap_workspace(B, T, 3 * tree.J, dev())
    back = torch.empty(B, T, 6 * tree.J, device=dev())

    def run():
        SK.launch_euler(x, tree, codes, d_frames, out=out)
        SK.launch_unwrap(out.view(B, T, -1), d_frames, workspace=ws)
        SK.launch_rot6d_euler(out, tree, codes, d_frames, out=back)
    run()                                                                          # warm-up: the order table is uploaded here
    torch.cuda.synchronize()
    eager = (out.clone(), back.clone())
    out.zero_(); back.zero_()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(back, eager[1])
    one = SK.euler_from_rot6d(x, tree, codes, frames=[T, UT + 1, 7], unwrap=True)[0]
    assert torch.equal(one, eager[0])


# ---- callers -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["alone", "draws", "takes", "fps", "smooth", "all"])
def test_synthesize_with_euler_equals_the_function_on_its_track(case):
    """"all": joints, rotations and Euler channels of one call, recordings of unequal length at another frame rate, each bit for bit the
    public function on out["track"].  The body is the 47-joint tree: a call refuses a tree whose 6J is not the generator's pose_dim (282 for
    the one BEAT-shaped generator the suite builds), so the five-joint chain cannot go through synthesize."""
    model, vae = beat_models()
    tree = tree_of("upper47")
    orders = names_of(EN.orders_cyclic(tree.J))
    U, W = 2, 3
    g = beat_inputs(U, W, 120)
    mean = gpu(mean_of(tree.J, 81))
    lengths = [3 * HOP - 100, HOP + 700]                                                            # 3 and 2 windows
    audio = gpu(synth_audio(U, max(lengths), seed=80))
    zz = torch.from_numpy(hash_uniform("articulate/z", (U, 2, W, 32), -2.0, 2.0, 121))
    kw = dict(hop_samples=HOP, joints=tree, joints_mean=mean, euler=orders)
    fn, fps, unwrap = Hs.synthesize, None, False
    if case == "alone":
        kw.update(labels=g["label"][:, 0].contiguous(), z=g["z"], lengths=lengths, euler="ZXY")
        orders = "ZXY"
    elif case == "draws":
        audio = audio[:, :2 * HOP + NS].contiguous()
        kw.update(labels=g["label"], z=zz, draws=2, euler_unwrap=True)
        unwrap = True
    elif case == "takes":
        fn = Hs.synthesize_takes
        kw.update(labels=g["label"][:, 0].contiguous(), z=zz, draws=2, lengths=lengths, euler_unwrap=True, rotations=True)
        unwrap = True
    elif case in ("fps", "all"):
        kw.update(labels=g["label"][:, 0].contiguous(), z=g["z"], lengths=lengths, joints_fps=(15, 30), **(dict(rotations=True) if case == "all" else {}))
        fps = (15, 30)
    else:
        kw.update(labels=g["label"][:, 0].contiguous(), z=g["z"], lengths=lengths, smooth=(9, 3))
    out = fn((model, vae), audio, g["text"], g["seed_pose"], **kw)
    lead = (U, 2) if case in ("draws", "takes") else (U,)
    wp = out["windows_per"] if "windows_per" in out else [W] * U
    frames = [w * HB + PB for w in wp]
    poses = out["track_smooth"] if case == "smooth" else out["track"]
    we, n_out = SK.euler_from_rot6d(poses, tree, orders, frames=frames, mean=mean, fps=fps, unwrap=unwrap)
    assert out["joint_frames"] == n_out == [SK.out_frames(n, fps) for n in frames]
    assert tuple(out["euler"].shape) == lead + (SK.out_frames(poses.shape[-2], fps), 47, 3) == tuple(out["joints"].shape)
    assert torch.equal(out["euler"], we) and torch.isfinite(we).all() and we[0].any()
    assert ("rotations" in out) == (case in ("takes", "all"))
    if case == "all":
        wj, nj = SK.joints_from_rot6d(poses, tree, frames=frames, mean=mean, fps=fps)
        wq, nq = SK.rotations_from_rot6d(poses, tree, frames=frames, mean=mean, fps=fps)
        assert nj == nq == n_out and torch.equal(out["joints"], wj) and torch.equal(out["rotations"], wq) and wq[0].any()
    if case != "draws":
        assert wp == [3, 2] and not out["euler"][1, ..., n_out[1]:, :, :].any()
    if case == "alone":                                                                             # without euler=: the same, no "euler"
        del kw["euler"]
        plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **kw)
        assert set(out) == set(plain) | {"euler"} and torch.equal(plain["joints"], out["joints"]) and torch.equal(plain["track"], out["track"])


def test_callers_refuse_by_name():
    from skeleton_gpu_common import inputs, ted_models
    model, vae = ted_models()
    g = inputs(2, 2, 80)
    audio = gpu(synth_audio(2, 32000 + (124 - 1) * 512, seed=82))
    call = lambda **kw: Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], labels=g["label"], hop_samples=32000, z=g["z"], **kw)
    with pytest.raises(L.EgError, match="synthesize: euler= without joints=tree"):
        call(euler="ZXY")
    with pytest.raises(L.EgError, match="synthesize: euler= with joints=Skeleton: direction-vector bodies have no joint rotations"):
        call(euler="ZXY", joints=SK.ted_expressive())
    with pytest.raises(L.EgError, match="synthesize: euler_unwrap=True without euler=order"):
        call(euler_unwrap=True, joints=SK.ted_expressive())
    with pytest.raises(L.EgError, match="GestureStream: euler= with joints=Skeleton"):
        Hs.open_stream((model, vae), 2, g["seed_pose"], hop_samples=32000, joints=SK.ted_expressive(), euler="ZXY")
    bmodel, bvae = beat_models()
    tree = tree_of("upper47")
    b = beat_inputs(2, 2, 120)
    with pytest.raises(L.EgError, match="GestureStream: euler_unwrap=True is not supported"):
        Hs.open_stream((bmodel, bvae), 2, b["seed_pose"], hop_samples=HOP, joints=tree, euler="ZXY", euler_unwrap=True)
    with pytest.raises(L.EgError, match="GestureStream: joints_fps= is not supported"):
        Hs.open_stream((bmodel, bvae), 2, b["seed_pose"], hop_samples=HOP, joints=tree, euler="ZXY", joints_fps=(15, 30))
    with pytest.raises(L.EgError, match="GestureStream: smooth= together with joints= is not supported"):
        Hs.open_stream((bmodel, bvae), 2, b["seed_pose"], hop_samples=HOP, joints=tree, euler="ZXY", smooth=(9, 3))
    with pytest.raises(L.EgError, match="GestureStream: euler= without joints=tree"):
        Hs.open_stream((bmodel, bvae), 2, b["seed_pose"], hop_samples=HOP, euler="ZXY")
    with pytest.raises(L.EgError, match="GestureStream: euler: joint 0: order 'ZXZ' repeats an axis"):
        Hs.open_stream((bmodel, bvae), 2, b["seed_pose"], hop_samples=HOP, joints=tree, euler="ZXZ")
    with pytest.raises(L.EgError, match="euler=BvhFile needs a tree with joint names"):
        Hs.open_stream((bmodel, bvae), 2, b["seed_pose"], hop_samples=HOP, joints=tree, euler=BVH.parse("ROOT a { OFFSET 0 0 0 CHANNELS 3 Zrotation Xrotation Yrotation }"))


def test_stream_last_euler_the_tail_and_the_finished_track():
    model, vae = beat_models()
    tree = tree_of("upper47")
    orders = names_of(EN.orders_cyclic(tree.J))
    U = 2
    g = beat_inputs(U, 4, 120)
    mean = gpu(mean_of(tree.J, 85))
    T = 2 * HOP + NS - 9000
    audio = gpu(synth_audio(U, T, seed=80))
    padded = torch.zeros(U, 4 * HOP, device=dev())
    padded[:, :T] = audio
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=tree, joints_mean=mean, euler=orders)
    assert s.last_euler is None
    chunks, raw = [], []
    for k in range(1, 5):
        c = max(0, k - 2)
        rows, valid = s.push(padded[:, (k - 1) * HOP:k * HOP].contiguous(), g["text"][:, c], g["label"][:, c], g["z"][:, c], ends=T - 3 * HOP if k == 4 else None)
        assert (rows is None) == (s.last_euler is None) == (k == 1)
        if rows is not None:
            assert tuple(s.last_euler.shape) == (U, HB, 47, 3) and s.last_rotations is None
            assert torch.equal(s.last_euler, SK.launch_euler(rows.contiguous(), tree, orders, valid, 1, HB, mean)) and s.last_euler.any()
            assert valid.cpu().tolist() == [1, 1]
            chunks.append(s.last_euler)
            raw.append(rows)
    assert len(chunks) == 3
    te = s.tail_euler()
    assert torch.equal(te, SK.launch_euler(s.tail().contiguous(), tree, orders, None, 1, 1, mean)) and tuple(te.shape) == (U, PB, 47, 3)
    track = torch.cat(raw + [s.tail()], 1)                                          # a row's pushes followed by its tail: its finished track
    assert torch.equal(torch.cat(chunks + [te], 1), SK.euler_from_rot6d(track, tree, orders, mean=mean))
    # a row that is not valid in a step has zero angles
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=tree, euler="ZXY")
    short = gpu(synth_audio(U, HOP, seed=86))
    rows, valid = s.push(short, g["text"][:, 0], g["label"][:, 0], g["z"][:, 0], ends=[-1, 700])
    assert valid.cpu().tolist() == [0, 1] and not s.last_euler[0].any() and s.last_euler[1].any()
    s2 = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, joints=tree)
    with pytest.raises(L.EgError, match="tail_euler: the session was opened without euler"):
        s2.tail_euler()


def test_stream_graph_holds_one_launch_more():
    """The launch histogram of a session's first emitting push -- two warm-up runs and the capture of the step, or the one run of an eager
    session -- with joints=tree, without and with euler=: the same launches, plus one articulate_euler per run."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EG_LAUNCH_HIST="1", PYTHONPATH=os.pathsep.join([root, os.path.dirname(os.path.abspath(__file__))]))
    res = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--hist-child"], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    hist = json.loads(next(line for line in res.stdout.splitlines() if line.startswith("HIST "))[5:])
    for mode, runs in (("graph", 3), ("eager", 1)):
        without, with_ = hist[mode]
        assert without and "articulate_euler" not in without and without.get("articulate_forward") == runs
        assert with_ == dict(without, articulate_euler=runs), (mode, without, with_)


def _hist_child():
    def histogram(reset):
        lib = L.load()
        buf = C.create_string_buffer(int(lib.eg_launch_histogram(None, 0, 0)) + 64)
        lib.eg_launch_histogram(buf, len(buf), int(reset))
        return {k: int(n) for k, n in (line.rsplit(" ", 1) for line in buf.value.decode().splitlines())}

    model, vae = beat_models()
    tree = tree_of("upper47")
    U = 2
    g = beat_inputs(U, 2, 120)
    audio = gpu(synth_audio(U, 2 * HOP, seed=5))
    out = {}
    for mode, graph in (("graph", True), ("eager", False)):
        out[mode] = []
        for kw in (dict(joints=tree), dict(joints=tree, euler="ZXY")):
            s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, graph=graph, **kw)
            tree.table(dev())                                     # the tables' uploads are no launches of the library, but keep them out of the step
            if "euler" in kw:
                s._outs.to(dev())
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
