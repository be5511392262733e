"""SRGR and L1 diversity on the GPU (eg_srgr_tracks / eg_l1div_tracks through jointscore.srgr_of_joints / l1div_of_tracks / launch_srgr /
launch_l1div, harness.synthesize(srgr=, l1div=) and synthesize_takes) against the numpy restatement tests/jointscore_np.py -- hits bit for
bit, every float64 figure inside the bound stated there -- and against itself bit for bit: a row alone against the row in a batch, graph
replay against eager, a device count of 0, the callers against the functions."""
import numpy as np
import pytest
import torch

import jointscore_np as JN
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import jointscore as JS
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.synth import synth_audio
from skeleton_gpu_common import H_, HOP, N, P_, dev, inputs, ted_models

pytestmark = pytest.mark.gpu

TF = JS.TILE_FRAMES
LENGTHS = (1, TF - 1, TF, TF + 1, 2 * TF + 3)
SRGR_KEYS = ("srgr", "recall", "hits")
L1_KEYS = ("l1div", "l1_sum", "mean")


def ratio(err, bound):
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("J", [1, 43, 47, 64])
def test_srgr_hits_bit_for_bit_and_rates_within_the_bound(J):
    """Every T around the tile height; two recordings, the second two frames short (one where T allows no less) with NaN behind its end;
    weights of both signs, a third of them 0; offsets that put 40-50 % of the cells inside the threshold."""
    worst = 0.0
    for T in LENGTHS:
        rng = np.random.default_rng(100 * J + T)
        g = rng.standard_normal((2, T, J, 3)).astype(np.float32)
        r = (g + (rng.random((2, T, J, 3)) - 0.5) * 0.14).astype(np.float32)
        w = (rng.random((2, T)) - 0.4).astype(np.float32)
        w[:, ::3] = 0
        frames = [T, max(1, T - 2)]
        r[1, frames[1]:], g[1, frames[1]:], w[1, frames[1]:] = np.nan, np.nan, np.nan
        got = JS.srgr_of_joints(*(torch.from_numpy(a).to(dev()) for a in (r, g, w)), frames=frames)
        assert all(got[k].is_cuda for k in SRGR_KEYS) and got["srgr"].dtype == torch.float64 and got["hits"].dtype == torch.int32
        assert tuple(got["srgr"].shape) == (2,) and tuple(got["hits"].shape) == (2, J) and got["frames"].tolist() == frames
        hits, want, bound, recall = JN.srgr(r, g, w, frames, 1, 0.1, JS.SCALE)
        assert np.array_equal(got["hits"].cpu().numpy(), hits), (J, T)
        assert np.array_equal(got["recall"].cpu().numpy(), recall), (J, T)
        err = np.abs(got["srgr"].cpu().numpy() - want)
        worst = max(worst, ratio(err, bound))
        assert (err <= bound).all() and (T * J < 1000 or 0.3 < recall[0] < 0.6), (J, T, err, bound)
        host = JS.srgr_of_joints(r, g, w, frames=frames)                                # the host path adds in the kernel's order
        assert np.array_equal(host["srgr"], got["srgr"].cpu().numpy()) and np.array_equal(host["hits"], hits)
    print(f"J={J}: worst srgr error / bound {worst:.3g}")


@pytest.mark.parametrize("D", [1, 3, 126, 129, 282, JS.MAX_COLS])
def test_l1_means_and_sums_within_the_bound(D):
    worst = [0.0, 0.0]
    for T in LENGTHS:
        rng = np.random.default_rng(100 * D + T)
        x = (rng.standard_normal((2, T, D)) * 0.3 + rng.standard_normal(D)).astype(np.float32)
        frames = [T, max(1, T - 2)]
        x[1, frames[1]:] = np.nan
        keep = x.copy()
        xd = torch.from_numpy(x).to(dev())
        got = JS.l1div_of_tracks(xd, frames=frames)
        assert all(got[k].is_cuda and got[k].dtype == torch.float64 for k in L1_KEYS) and tuple(got["mean"].shape) == (2, D)
        assert np.array_equal(xd.cpu().numpy(), keep, equal_nan=True)                 # the input is not written
        mean, mean_bound, s, s_bound = JN.l1div(x, frames)
        e_m, e_s = np.abs(got["mean"].cpu().numpy() - mean), np.abs(got["l1_sum"].cpu().numpy() - s)
        worst = [max(worst[0], ratio(e_m, mean_bound)), max(worst[1], ratio(e_s, s_bound))]
        assert (e_m <= mean_bound).all() and (e_s <= s_bound).all(), (D, T)
        assert np.array_equal(got["l1div"].cpu().numpy(), got["l1_sum"].cpu().numpy() / np.asarray(frames, np.float64))
        assert np.isfinite(got["mean"].cpu().numpy()).all() and (T == 1 or s[0] > 0)
    print(f"D={D}: worst mean error / bound {worst[0]:.3g}, worst l1_sum error / bound {worst[1]:.3g}")


def test_a_row_does_not_depend_on_the_batch_on_its_place_or_on_T():
    """[U, R, T, ...] with R = 3, unequal frames, NaN tails and non-contiguous input; then one take alone, as [T, J, 3], in another batch at
    another place and at a larger T: the same bits."""
    U, R, T, J = 3, 3, 2 * TF + 5, 43
    rng = np.random.default_rng(9)
    g = rng.standard_normal((U, T, J, 3)).astype(np.float32)
    r = (g[:, None] + (rng.random((U, R, T, J, 3)) - 0.5) * 0.14).astype(np.float32)
    w = (rng.random((U, T)) - 0.4).astype(np.float32)
    frames = [TF + 3, T, 7]
    for u, n in enumerate(frames):
        r[u, :, n:], g[u, n:], w[u, n:] = np.nan, np.nan, np.nan
    wide = torch.from_numpy(np.concatenate([r, r], -1)).to(dev())                       # [U, R, T, J, 6]: the joints are a strided view of it
    rd, gd, wd = wide[..., :3], torch.from_numpy(g).to(dev()), torch.from_numpy(w).to(dev())
    assert not rd.is_contiguous()
    got = JS.srgr_of_joints(rd, gd, wd, frames=frames)
    per = [n for n in frames for _ in range(R)]
    hits, want, bound, recall = JN.srgr(r.reshape(U * R, T, J, 3), g, w, per, R, 0.1, JS.SCALE)
    assert tuple(got["srgr"].shape) == (U, R) and np.array_equal(got["hits"].cpu().numpy().reshape(U * R, J), hits)
    assert (np.abs(got["srgr"].cpu().numpy().reshape(-1) - want) <= bound).all() and np.array_equal(got["recall"].cpu().numpy().reshape(-1), recall)
    flat = wide.reshape(U, R, T, J * 6)[..., : J * 3 + 1][..., 1:]                        # non-contiguous: columns 1 .. 3J of 6J
    l1 = JS.l1div_of_tracks(flat, frames=frames)
    x = flat.cpu().numpy()
    mean, mean_bound, s, s_bound = JN.l1div(x.reshape(U * R, T, J * 3), per)
    assert (np.abs(l1["mean"].cpu().numpy().reshape(U * R, -1) - mean) <= mean_bound).all()
    assert (np.abs(l1["l1_sum"].cpu().numpy().reshape(-1) - s) <= s_bound).all()
    # take (0, 2) alone, and as recording 2 of another batch at a larger T
    u, k, n = 0, 2, frames[0]
    alone = JS.srgr_of_joints(torch.from_numpy(r[u, k, :n]).to(dev()), gd[u, :n], wd[u, :n])
    alone_l1 = JS.l1div_of_tracks(torch.from_numpy(x[u, k, :n]).to(dev()))
    T2 = T + TF + 1
    r2, g2 = np.full((3, T2, J, 3), np.nan, np.float32), np.full((3, T2, J, 3), np.nan, np.float32)
    w2, x2 = np.full((3, T2), np.nan, np.float32), np.full((3, T2, J * 3), np.nan, np.float32)
    f2 = [5, T2, n]
    for i, m in enumerate(f2):
        g2[i, :m] = rng.standard_normal((m, J, 3))
        r2[i, :m] = g2[i, :m] + (rng.random((m, J, 3)) - 0.5) * 0.14
        w2[i, :m] = rng.random(m)
        x2[i, :m] = rng.standard_normal((m, J * 3))
    r2[2, :n], g2[2, :n], w2[2, :n], x2[2, :n] = r[u, k, :n], g[u, :n], w[u, :n], x[u, k, :n]
    moved = JS.srgr_of_joints(*(torch.from_numpy(a).to(dev()) for a in (r2, g2, w2)), frames=f2)
    moved_l1 = JS.l1div_of_tracks(torch.from_numpy(x2).to(dev()), frames=f2)
    for key in SRGR_KEYS:
        assert torch.equal(alone[key], got[key][u, k]) and torch.equal(moved[key][2], got[key][u, k]), key
    for key in L1_KEYS:
        assert torch.equal(alone_l1[key], l1[key][u, k]) and torch.equal(moved_l1[key][2], l1[key][u, k]), key
    assert float(got["srgr"][u, k]) != 0.0 and float(l1["l1_sum"][u, k]) > 0


def test_the_threshold_edge_and_a_device_count_of_zero():
    r = torch.tensor([[[0.0625, 0.03125, 0.0]]], device=dev())
    g = torch.zeros_like(r)
    miss = JS.srgr_of_joints(r, g, threshold=0.09375)
    hit = JS.srgr_of_joints(r, g, threshold=float(np.nextafter(0.09375, 1)))
    assert miss["hits"].tolist() == [0] and float(miss["srgr"]) == 0.0
    assert hit["hits"].tolist() == [1] and float(hit["recall"]) == 1.0 and float(hit["srgr"]) == 1 / 0.165
    nan = JS.srgr_of_joints(torch.full_like(r, float("nan")), g, threshold=1e9)
    assert nan["hits"].tolist() == [0]
    # row 1's device count is 0 behind a host count that passes: zeros, although its frames are all NaN; its neighbours as they are alone
    T, J = TF + 9, 47
    rng = np.random.default_rng(8)
    gd = torch.from_numpy(rng.standard_normal((3, T, J, 3)).astype(np.float32)).to(dev())
    rd = gd + (torch.rand(3, T, J, 3, device=dev()) - 0.5) * 0.14
    xd = rd.reshape(3, T, J * 3).contiguous()
    frames = [T, T - 2, TF]
    d_frames = torch.tensor(frames, dtype=torch.int32, device=dev())
    out = tuple(torch.full_like(t, 7) for t in JS.launch_srgr(rd, gd, None, frames, d_frames))
    out_l1 = tuple(torch.full_like(t, 7) for t in JS.launch_l1div(xd, frames, d_frames))
    JS.launch_srgr(rd, gd, None, frames, d_frames, out=out)
    JS.launch_l1div(xd, frames, d_frames, out=out_l1)
    first, first_l1 = [t.clone() for t in out], [t.clone() for t in out_l1]
    assert int(first[2].sum()) > 0 and float(first_l1[1].min()) > 0
    rd[1], gd[1], xd[1] = float("nan"), float("nan"), float("nan")
    low = torch.tensor([T, 0, TF], dtype=torch.int32, device=dev())
    JS.launch_srgr(rd, gd, None, frames, low, out=out)
    JS.launch_l1div(xd, frames, low, out=out_l1)
    assert not any(t[1].any() for t in out) and not any(t[1].any() for t in out_l1)
    for b in (0, 2):
        assert all(torch.equal(t[b], f[b]) for t, f in zip(out, first)) and all(torch.equal(t[b], f[b]) for t, f in zip(out_l1, first_l1))


def test_graph_replay_equals_the_eager_calls():
    """Both calls in one graph, replayed three times on fresh inputs: each replay is the eager call bit for bit (nothing is zeroed and nothing
    is left over from the replay before)."""
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    U, R, T, J = 2, 3, 2 * TF + 4, 43
    frames = [2 * TF + 4, TF - 1]
    rng = np.random.default_rng(77)
    rd, gd = torch.empty(U * R, T, J, 3, device=dev()), torch.empty(U, T, J, 3, device=dev())
    wd = torch.empty(U, T, device=dev())
    xd = rd.view(U * R, T, J * 3)

    def fresh():
        g = rng.standard_normal((U, T, J, 3)).astype(np.float32)
        gd.copy_(torch.from_numpy(g))
        rd.copy_(torch.from_numpy((np.repeat(g, R, 0) + (rng.random((U * R, T, J, 3)) - 0.5) * 0.14).astype(np.float32)))
        wd.copy_(torch.from_numpy((rng.random((U, T)) - 0.4).astype(np.float32)))

    fresh()
    d_frames = torch.tensor(frames, dtype=torch.int32, device=dev())
    lib = JS.L.load()
    ws_s = torch.empty(int(lib.eg_srgr_workspace_bytes(U * R, T, J)), dtype=torch.uint8, device=dev())
    ws_l = torch.empty(int(lib.eg_l1div_workspace_bytes(U * R, T, J * 3)), dtype=torch.uint8, device=dev())
    out_s = tuple(torch.empty_like(t) for t in JS.launch_srgr(rd, gd, wd, frames, d_frames, R, workspace=ws_s))      # the warm-up
    out_l = tuple(torch.empty_like(t) for t in JS.launch_l1div(xd, frames, d_frames, R, workspace=ws_l))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        JS.launch_srgr(rd, gd, wd, frames, d_frames, R, workspace=ws_s, out=out_s)
        JS.launch_l1div(xd, frames, d_frames, R, workspace=ws_l, out=out_l)
    for k in range(3):
        fresh()
        for t in out_s + out_l:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        eager = JS.launch_srgr(rd, gd, wd, frames, d_frames, R) + JS.launch_l1div(xd, frames, d_frames, R)
        assert all(torch.equal(a, b) for a, b in zip(out_s + out_l, eager)), k
        assert int(out_s[2].sum()) > 0 and float(out_l[1].min()) > 0
    # the draws axis: one count and one target per recording, shared by its rows
    each = [n for n in frames for _ in range(R)]
    rows = JS.launch_srgr(rd, gd.repeat_interleave(R, 0), wd.repeat_interleave(R, 0), each, torch.tensor(each, dtype=torch.int32, device=dev()))
    assert all(torch.equal(a, b) for a, b in zip(out_s, rows))


# ---- the callers ---------------------------------------------------------------------------------------------------------------------------
def same(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert (torch.equal(got[k], v) if isinstance(v, torch.Tensor) else np.array_equal(got[k], v)), k


def same_but(got, plain, extra):
    assert set(got) == set(plain) | extra
    for k, v in plain.items():
        assert torch.equal(got[k], v) if isinstance(v, torch.Tensor) else got[k] == v, k


def targets_near(joints, seed, takes=False):
    """SemanticTargets at the shape of a call's joints: the (first take's) joints moved by up to 7 cm per coordinate, weights in [0, 1)."""
    base = joints[:, 0] if takes else joints
    gen = torch.Generator().manual_seed(seed)
    move = ((torch.rand(base.shape, generator=gen) - 0.5) * 0.14).to(base.device)
    base = torch.nan_to_num(base)
    return JS.SemanticTargets(base + move, torch.rand(base.shape[:2], generator=gen).to(base.device), threshold=0.1)


def test_synthesize_srgr_and_l1div_rectangular_ragged_and_smoothed():
    model, vae = ted_models()
    sk = SK.ted_expressive()
    U, W = 2, 2
    g = inputs(U, W, 60)
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=61)).to(dev())
    kw = dict(labels=g["label"], hop_samples=HOP, z=g["z"], joints=sk)
    plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **kw)
    tg = targets_near(plain["joints"], 1)
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], srgr=tg, l1div=True, **kw)
    same_but(got, plain, {"srgr", "l1div"})
    same(got["srgr"], JS.srgr_of_joints(got["joints"], tg.joints, tg.semantic, got["joint_frames"], 0.1))
    same(got["l1div"], JS.l1div_of_tracks(got["joints"].flatten(-2), got["joint_frames"]))
    n = W * H_ + P_
    assert tuple(got["srgr"]["hits"].shape) == (U, sk.J) and got["srgr"]["frames"].tolist() == [n] * U and tuple(got["l1div"]["mean"].shape) == (U, 3 * sk.J)
    assert 0 < float(got["srgr"]["recall"].min()) and float(got["srgr"]["recall"].max()) < 1 and float(got["l1div"]["l1div"].min()) > 0
    only = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], l1div=True, **kw)
    same_but(only, plain, {"l1div"})
    # targets of another length are refused by name before the roll-out
    with pytest.raises(JS.L.EgError, match=f"synthesize: srgr=: the targets .* have T'={n - 1}, the call's joints have T'={n}"):
        Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], srgr=JS.SemanticTargets(tg.joints[:, :-1]), **kw)
    # smooth=(9, 3) at 30 fps: the figures describe the smoothed joints
    sm_plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], smooth=(9, 3), joints_fps=(15, 30), **kw)
    tg2 = targets_near(sm_plain["joints"], 2)
    sm = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], smooth=(9, 3), joints_fps=(15, 30), srgr=tg2, l1div=True, **kw)
    assert sm["joint_frames"] == [2 * n] * U and torch.equal(sm["joints"], sm_plain["joints"])
    same(sm["srgr"], JS.srgr_of_joints(sm["joints"], tg2.joints, tg2.semantic, sm["joint_frames"], 0.1))
    same(sm["l1div"], JS.l1div_of_tracks(sm["joints"].flatten(-2), sm["joint_frames"]))
    # lengths=: 2 and 1 windows
    lens = [2 * HOP - 7, HOP - 5]
    audio = torch.from_numpy(synth_audio(U, max(lens), seed=62)).to(dev())
    rkw = dict(labels=g["label"][:, 0].contiguous(), hop_samples=HOP, z=g["z"], joints=sk, lengths=lens)
    rg_plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **rkw)
    tg3 = targets_near(rg_plain["joints"], 3)
    rg = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], srgr=tg3, l1div=True, **rkw)
    assert rg["windows_per"] == [2, 1] and rg["srgr"]["frames"].tolist() == [2 * H_ + P_, H_ + P_]
    same(rg["srgr"], JS.srgr_of_joints(rg["joints"], tg3.joints, tg3.semantic, rg["joint_frames"], 0.1))
    same(rg["l1div"], JS.l1div_of_tracks(rg["joints"].flatten(-2), rg["joint_frames"]))


def test_synthesize_draws_and_takes_srgr_and_l1div():
    model, vae = ted_models()
    sk = SK.ted_expressive()
    U, W, Rd = 2, 2, 2
    g = inputs(U, W, 80)
    zz = torch.from_numpy(np.random.default_rng(83).standard_normal((U, Rd, W, 32)).astype(np.float32))
    lens = [2 * HOP - 7, HOP - 5]
    audio = torch.from_numpy(synth_audio(U, max(lens), seed=80)).to(dev())
    kw = dict(lengths=lens, draws=Rd, z=zz, hop_samples=HOP, joints=sk)
    plain = Hs.synthesize_takes((model, vae), audio, g["text"], g["seed_pose"], g["label"][:, 0].contiguous(), **kw)
    tg = targets_near(plain["joints"], 4, takes=True)
    got = Hs.synthesize_takes((model, vae), audio, g["text"], g["seed_pose"], g["label"][:, 0].contiguous(), srgr=tg, l1div=True, **kw)
    same_but(got, plain, {"srgr", "l1div"})
    assert got["windows_per"] == [2, 1] and tuple(got["srgr"]["srgr"].shape) == (U, Rd) and tuple(got["srgr"]["hits"].shape) == (U, Rd, sk.J)
    assert got["srgr"]["frames"].tolist() == [[2 * H_ + P_] * Rd, [H_ + P_] * Rd]
    same(got["srgr"], JS.srgr_of_joints(got["joints"], tg.joints, tg.semantic, got["joint_frames"], 0.1))
    same(got["l1div"], JS.l1div_of_tracks(got["joints"].flatten(-2), got["joint_frames"]))
    # take 0 is within 7 cm of the target everywhere; the rectangular draws= call
    assert float(got["srgr"]["recall"][:, 0].min()) > 0
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=82)).to(dev())
    dkw = dict(labels=g["label"], hop_samples=HOP, z=zz, draws=Rd, joints=sk)
    d_plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **dkw)
    tg2 = targets_near(d_plain["joints"], 5, takes=True)
    dr = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], srgr=tg2, l1div=True, **dkw)
    same_but(dr, d_plain, {"srgr", "l1div"})
    same(dr["srgr"], JS.srgr_of_joints(dr["joints"], tg2.joints, tg2.semantic, dr["joint_frames"], 0.1))
    same(dr["l1div"], JS.l1div_of_tracks(dr["joints"].flatten(-2), dr["joint_frames"]))
