"""The motion statistics on the GPU (eg_kin_stats through kinematics.kinematics_of_joints / launch_kinematics, harness.synthesize(kinematics=)
and synthesize_takes(kinematics=)) against the numpy restatement tests/kinematics_np.py -- histograms bit for bit, every mean inside the bound
stated there -- and against itself bit for bit: samples exactly on an edge, a row alone against the row in a batch, the same call twice, graph
replay against eager, a device count below 4, the callers against the function."""
import numpy as np
import pytest
import torch

import kinematics_np as KN
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import kinematics as KM
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.synth import synth_audio
from skeleton_gpu_common import H_, HOP, N, P_, dev, inputs, ted_models

pytestmark = pytest.mark.gpu

TF = KM.TILE_FRAMES
FPS = 15
KEYS = ("speed", "accel", "jerk", "speed_hist", "speed_over")


def figures(res):
    """The dict of kinematics_of_joints -> mean [rows, 3, J], hist [rows, J, B + 1] as numpy."""
    J = res["speed"].shape[-1]
    mean = torch.stack([res[k].reshape(-1, J) for k in ("speed", "accel", "jerk")], 1).cpu().numpy()
    hist = torch.cat([res["speed_hist"].reshape(-1, J, res["speed_hist"].shape[-1]), res["speed_over"].reshape(-1, J, 1)], 2).cpu().numpy()
    return mean, hist


def check(p, frames, edges, what):
    """One call on the device against the restatement: histograms equal, every mean inside the bound."""
    lead, (T, J) = p.shape[:-3], p.shape[-3:-1]
    R = lead[1] if len(lead) == 2 else 1
    got = KM.kinematics_of_joints(torch.from_numpy(p).to(dev()), FPS, frames=frames, edges=edges)
    B = len(edges) - 1
    assert all(got[k].is_cuda for k in KEYS) and got["jerk"].dtype == torch.float64 and got["speed_hist"].dtype == torch.int32, what
    assert tuple(got["speed"].shape) == lead + (J,) and tuple(got["speed_hist"].shape) == lead + (J, B) and tuple(got["speed_over"].shape) == lead + (J,)
    per_row = [n for n in (frames if frames is not None else [T]) for _ in range(R)]
    want, count, hist = KN.stats(p.reshape((-1,) + p.shape[-3:]), per_row, KN.edges2_of(edges, FPS), FPS)
    mean, h = figures(got)
    assert np.array_equal(h, hist), what
    assert np.array_equal(h.sum(-1), np.repeat(np.asarray(per_row)[:, None] - 1, J, 1)), what
    ok, ratio = KN.within(mean, want, count)
    print(f"{what}: worst mean error / bound {ratio:.3f}")
    assert ok and np.isfinite(mean).all(), (what, ratio)


@pytest.mark.parametrize("J", [1, 43, 47, 64])
def test_histogram_bit_for_bit_and_means_within_the_bound(J):
    """T = 4 (the shortest), one tile + 1 and two tiles + 3; frames = 4, TF, TF + 1, TF + 3 and T: the 3-frame halo ends on a tile boundary,
    one past it and at the last tile; one, three and 2 x 3 rows with NaN behind every row's end; 1, 40 and 256 bins; positions of 0.01, 1 and
    30 m, with edges that spread the samples of each over the bins."""
    case = 0
    for T in (4, TF + 1, 2 * TF + 3):
        pick = sorted({n for n in (4, TF, TF + 1, TF + 3, T) if n <= T})      # [4], [4, TF, TF + 1], [4, TF, TF + 1, TF + 3, T]
        for shape, frames in (((T, J, 3), None), ((3, T, J, 3), [pick[0], pick[len(pick) // 2], pick[-1]]),
                              ((2, 3, T, J, 3), [pick[-2] if len(pick) > 1 else pick[0], pick[min(1, len(pick) - 1)]])):
            B, scale = (1, 40, 256)[case % 3], (0.01, 1.0, 30.0)[(case // 3 + case) % 3]
            case += 1
            rng = np.random.default_rng(1000 * J + 10 * T + len(shape))
            p = (rng.standard_normal(shape) * scale).astype(np.float32)
            for u, n in enumerate(frames or []):
                p[u, ..., n:, :, :] = np.nan
            edges = np.linspace(0.0, 60.0 * scale, B + 1)
            check(p, frames, edges, f"J={J} {list(shape)} frames={frames} B={B} scale={scale}")
    assert case == 9


@pytest.mark.parametrize("T,J", [(2 * TF + 3, 1), (6, 43), (TF + 40, 2)])
def test_samples_exactly_on_an_edge_land_in_the_upper_bin(T, J):
    """The table is made of the restatement's own s2 values of the input: every sample sits exactly on an edge, and a kernel whose s2 differed
    in the last bit would put it one bin lower."""
    rng = np.random.default_rng(T + J)
    p = (rng.standard_normal((1, T, J, 3)) * 0.3).astype(np.float32)
    s2 = KN.s2_of(p[0], T, 1)
    table = np.concatenate([[0.0], np.unique(s2)])
    assert 2 <= len(table) <= 257 and table[1] > 0
    x = torch.from_numpy(p).to(dev())
    _mean, hist = KM.launch_kinematics(x, KM.SpeedBins(fps=FPS), edges2=torch.from_numpy(table).to(dev()))
    h = hist.cpu().numpy()[0]
    pos = np.searchsorted(table, s2, side="right") - 1
    assert np.array_equal(table[pos], s2)                                           # on its edge
    for j in range(J):
        assert np.array_equal(h[j], np.bincount(pos[:, j], minlength=len(table))), j
    assert not h[:, 0].any() and h.sum() == (T - 1) * J


def test_a_row_does_not_depend_on_the_batch_on_its_place_or_on_T():
    n, J = TF + 3, 43
    rng = np.random.default_rng(3)
    row = (rng.standard_normal((n, J, 3)) * 0.02).astype(np.float32)
    alone = KM.kinematics_of_joints(torch.from_numpy(row).to(dev()), FPS)
    assert float(alone["jerk"].min()) > 0 and int(alone["speed_hist"].sum()) + int(alone["speed_over"].sum()) == (n - 1) * J
    for place in (0, 2):
        T = 2 * TF + 5
        p = (rng.standard_normal((3, T, J, 3)) * 0.02).astype(np.float32)
        frames = [T, 4, T - 1]
        frames[place] = n
        p[place, :n] = row
        p[place, n:] = np.nan
        got = KM.kinematics_of_joints(torch.from_numpy(p).to(dev()), FPS, frames=frames)
        for k in KEYS:
            assert torch.equal(got[k][place], alone[k]), (place, k)
    one = KM.kinematics_of_joints(torch.from_numpy(row[None]).to(dev()), FPS, frames=[n])
    assert all(torch.equal(one[k][0], alone[k]) for k in KEYS)


def test_the_same_call_twice_and_a_device_count_below_four():
    """hist is zeroed inside the call: the same buffers, full of other values, give the same bits twice.  Then row 1's device count is 2 behind
    a host count that passes: its outputs are zeros although its frames are all NaN, and its neighbours' figures are those they have alone."""
    T, J = TF + 9, 47
    rng = np.random.default_rng(8)
    x = torch.from_numpy((rng.standard_normal((3, T, J, 3)) * 0.02).astype(np.float32)).to(dev())
    bins = KM.SpeedBins(fps=FPS)
    frames = [T, T - 2, TF]
    d_frames = torch.tensor(frames, dtype=torch.int32, device=dev())
    out = (torch.full((3, 3, J), 7.0, dtype=torch.float64, device=dev()), torch.full((3, J, 41), 7, dtype=torch.int32, device=dev()))
    KM.launch_kinematics(x, bins, frames, d_frames, out=out)
    first = [t.clone() for t in out]
    KM.launch_kinematics(x, bins, frames, d_frames, out=out)
    assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1])
    assert out[1].sum(-1).cpu().tolist() == [[n - 1] * J for n in frames]
    x[1] = float("nan")
    low = torch.tensor([T, 2, TF], dtype=torch.int32, device=dev())
    KM.launch_kinematics(x, bins, frames, low, out=out)
    assert not out[0][1].any() and not out[1][1].any()
    for b in (0, 2):
        assert torch.equal(out[0][b], first[0][b]) and torch.equal(out[1][b], first[1][b])


@pytest.mark.parametrize("unit,counts,zero", [(1, None, True), (4, 1, False), (4, 0, True)], ids=["count-3", "flags-of-4-one", "flags-of-4-none"])
def test_device_counts_that_differ_from_the_host_copy_meet_the_floor_of_four(unit, counts, zero):
    """The floor of the shared device count (csrc/rows.h) at its edge, with draws: U = 2 recordings of 2 draws, T = one tile + 5 frames (two
    tiles, the second ragged), J = 3.  The host counts pass ([T, T]); the device counts give recording 1 three frames (one below the floor:
    zeros), or in the stream's flag form (frame_unit = 4, [T / 4, 1 or 0]) four frames (the floor itself: the figures of four frames) or none
    (zeros).  Recording 0 has the bits of the call whose two copies agree; the NaN behind every device count reaches no output."""
    T, J, dev_ = TF + 5, 3, dev()
    d_counts = [T, 3] if counts is None else [T // 4, counts]
    n = [min(c * unit, T) for c in d_counts]
    rng = np.random.default_rng(40 + unit)
    p = (rng.standard_normal((4, T, J, 3)) * 0.02).astype(np.float32)
    for u in range(2):
        p[2 * u:2 * u + 2, n[u]:] = np.nan
    x = torch.from_numpy(p).to(dev_)
    bins = KM.SpeedBins(fps=FPS)
    out = (torch.full((4, 3, J), 7.0, dtype=torch.float64, device=dev_), torch.full((4, J, 41), 7, dtype=torch.int32, device=dev_))
    KM.launch_kinematics(x, bins, [T, T], torch.tensor(d_counts, dtype=torch.int32, device=dev_), 2, unit, out=out)
    mean, hist = out
    assert bool(torch.isfinite(mean).all())
    # the call whose host and device copies agree: recording 1 gets the floor's four frames so that the host check passes
    agree = [d_counts[0], max(d_counts[1], -(-4 // unit))]
    want_mean, want_hist = KM.launch_kinematics(x, bins, agree, torch.tensor(agree, dtype=torch.int32, device=dev_), 2, unit)
    assert torch.equal(mean[:2], want_mean[:2]) and torch.equal(hist[:2], want_hist[:2])
    assert hist[:2].sum(-1).cpu().tolist() == [[n[0] - 1] * J] * 2
    if zero:
        assert not mean[2:].any() and not hist[2:].any()
    else:
        assert torch.equal(mean[2:], want_mean[2:]) and torch.equal(hist[2:], want_hist[2:])
        assert hist[2:].sum(-1).cpu().tolist() == [[3] * J] * 2 and bool((mean[2:] > 0).all())


def test_graph_replay_equals_the_eager_call():
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    T, J, frames = 2 * TF + 4, 43, [2 * TF + 4, TF - 1, 4, 40, 2 * TF, TF + 2]
    rng = np.random.default_rng(77)
    new = lambda: torch.from_numpy((rng.standard_normal((6, T, J, 3)) * 0.02).astype(np.float32))
    x = new().to(dev())
    bins = KM.SpeedBins(fps=FPS)
    d_frames = torch.tensor(frames, dtype=torch.int32, device=dev())
    ws = torch.empty(int(KM.L.load().eg_kin_workspace_bytes(6, T, J, bins.bins)), dtype=torch.uint8, device=dev())
    out = tuple(torch.empty_like(t) for t in KM.launch_kinematics(x, bins, frames, d_frames, workspace=ws))     # the warm-up: the table is uploaded here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        KM.launch_kinematics(x, bins, frames, d_frames, workspace=ws, out=out)
    for k in range(2):
        x.copy_(new())
        out[0].fill_(float("nan"))
        out[1].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        mean, hist = KM.launch_kinematics(x, bins, frames, d_frames)
        assert torch.equal(out[0], mean) and torch.equal(out[1], hist), k
    # the draws axis: one count per recording, shared by its rows
    d2 = torch.tensor(frames[:3], dtype=torch.int32, device=dev())
    each = [n for n in frames[:3] for _ in range(2)]
    pairs = KM.launch_kinematics(x, bins, frames[:3], d2, draws=2)
    rows = KM.launch_kinematics(x, bins, each, torch.tensor(each, dtype=torch.int32, device=dev()))
    assert torch.equal(pairs[0], rows[0]) and torch.equal(pairs[1], rows[1])
    # a histogram of 4 x 64 x 257 counts (263 KB, and more than 64 KB of LDS per workgroup): zeroed on every one of three replays
    big = KM.SpeedBins(np.linspace(0, 2, 257), FPS)
    xb = torch.from_numpy((rng.standard_normal((4, TF + 1, 64, 3)) * 0.02).astype(np.float32)).to(dev())
    want = KM.launch_kinematics(xb, big)
    ws = torch.empty(int(KM.L.load().eg_kin_workspace_bytes(4, TF + 1, 64, 256)), dtype=torch.uint8, device=dev())
    out = tuple(torch.empty_like(t) for t in want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        KM.launch_kinematics(xb, big, workspace=ws, out=out)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]), k


# ---- the callers ---------------------------------------------------------------------------------------------------------------------------
def same(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert (torch.equal(got[k], v) if isinstance(v, torch.Tensor) else np.array_equal(got[k], v)), k


def same_but(got, plain, extra):
    assert set(got) == set(plain) | extra
    for k, v in plain.items():
        assert torch.equal(got[k], v) if isinstance(v, torch.Tensor) else got[k] == v, k


def test_synthesize_kinematics_rectangular_ragged_and_smoothed():
    model, vae = ted_models()
    sk = SK.ted_expressive()
    U, W = 2, 2
    g = inputs(U, W, 60)
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=61)).to(dev())
    kw = dict(labels=g["label"], hop_samples=HOP, z=g["z"], joints=sk)
    plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **kw)
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], kinematics=True, **kw)
    same_but(got, plain, {"kinematics"})
    kin = got["kinematics"]
    same(kin, KM.kinematics_of_joints(got["joints"], FPS, frames=got["joint_frames"]))
    n = W * H_ + P_
    assert got["joint_frames"] == [n] * U and tuple(kin["speed"].shape) == (U, sk.J) and tuple(kin["speed_hist"].shape) == (U, sk.J, 40)
    assert torch.equal(kin["speed_hist"].sum(-1) + kin["speed_over"], torch.full((U, sk.J), n - 1, dtype=torch.int32, device=dev()))
    # smooth=(9, 3): the figures describe the smoothed joints, whose mean jerk is below the raw joints' for every recording; at 30 fps with
    # other edges
    edges = np.linspace(0, 4, 21)
    sm = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], smooth=(9, 3), kinematics=edges, joints_fps=(15, 30), **kw)
    same(sm["kinematics"], KM.kinematics_of_joints(sm["joints"], 30, frames=sm["joint_frames"], edges=edges))
    assert sm["joint_frames"] == [2 * n] * U and tuple(sm["kinematics"]["speed_hist"].shape) == (U, sk.J, 20)
    smooth15 = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], smooth=(9, 3), kinematics=True, **kw)["kinematics"]
    raw, smooth = kin["jerk"].mean(-1).cpu().tolist(), smooth15["jerk"].mean(-1).cpu().tolist()
    print(f"mean jerk per recording: raw {raw}, smoothed {smooth}")
    assert all(s < r for s, r in zip(smooth, raw))
    # lengths=: 2 and 1 windows
    lens = [2 * HOP - 7, HOP - 5]
    audio = torch.from_numpy(synth_audio(U, max(lens), seed=62)).to(dev())
    rg = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], labels=g["label"][:, 0].contiguous(), hop_samples=HOP, z=g["z"], joints=sk,
                       lengths=lens, kinematics=KM.SpeedBins(fps=FPS))
    assert rg["windows_per"] == [2, 1] and rg["joint_frames"] == [2 * H_ + P_, H_ + P_]
    same(rg["kinematics"], KM.kinematics_of_joints(rg["joints"], FPS, frames=rg["joint_frames"]))
    assert (rg["kinematics"]["speed_hist"].sum(-1) + rg["kinematics"]["speed_over"])[:, 0].cpu().tolist() == [2 * H_ + P_ - 1, H_ + P_ - 1]


def test_synthesize_draws_and_takes_kinematics():
    model, vae = ted_models()
    sk = SK.ted_expressive()
    U, W, Rd = 2, 2, 2
    g = inputs(U, W, 80)
    zz = torch.from_numpy(np.random.default_rng(83).standard_normal((U, Rd, W, 32)).astype(np.float32))
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=82)).to(dev())
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], labels=g["label"], hop_samples=HOP, z=zz, draws=Rd, joints=sk, kinematics=True)
    assert tuple(got["kinematics"]["jerk"].shape) == (U, Rd, sk.J) and tuple(got["kinematics"]["speed_hist"].shape) == (U, Rd, sk.J, 40)
    same(got["kinematics"], KM.kinematics_of_joints(got["joints"], FPS, frames=got["joint_frames"]))
    lens = [2 * HOP - 7, HOP - 5]
    audio = torch.from_numpy(synth_audio(U, max(lens), seed=80)).to(dev())
    kw = dict(lengths=lens, draws=Rd, z=zz, hop_samples=HOP, joints=sk)
    plain = Hs.synthesize_takes((model, vae), audio, g["text"], g["seed_pose"], g["label"][:, 0].contiguous(), **kw)
    got = Hs.synthesize_takes((model, vae), audio, g["text"], g["seed_pose"], g["label"][:, 0].contiguous(), kinematics=True, **kw)
    same_but(got, plain, {"kinematics"})
    assert got["windows_per"] == [2, 1] and tuple(got["kinematics"]["speed"].shape) == (U, Rd, sk.J)
    same(got["kinematics"], KM.kinematics_of_joints(got["joints"], FPS, frames=got["joint_frames"]))
    counts = (got["kinematics"]["speed_hist"].sum(-1) + got["kinematics"]["speed_over"])[:, :, 0].cpu().tolist()
    assert counts == [[2 * H_ + P_ - 1] * Rd, [H_ + P_ - 1] * Rd]
