"""Motion-clip features of whole tracks on the GPU (csrc/motionfeat.hip through emotiongestures_amd.motionfeat, takes.take_diversity,
harness.synthesize_takes and EmbeddingSpaceEvaluator.push_tracks): (1) bit for bit against the per-layer chain on host-cut windows, (2) every
element against the float64 tower within an a-priori bound, (3) the reference's golden latents, (4) the take diversity against the numpy
restatement, (5) the evaluator on tracks against the evaluator on clips, (6) graph capture, (7) end to end from raw audio.

The base case straddles the kernel's run: recording 2 has 34 + 2 * RUN_FRAMES + 3 poses, so at every stride its takes span several runs, a
partial last run and (with the tail) a window on no stride grid; recordings 0 and 1 have one window, and one window plus the tail."""
import os

import numpy as np
import pytest
import torch

import motionfeat_np as MN
import rollout_np as RN
import takes_np as T
from conftest import build_mirror
from emotiongestures_amd import motionfeat as MF
from emotiongestures_amd import takes
from emotiongestures_amd.model.motion_ae import MotionAE, _conv, _conv_pack
from emotiongestures_amd.synth import hash_uniform, hash_unit, load_synth_weights, synth_audio
from small_ops_f64 import compare_sliced

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(__file__)
U_, R_, D_ = 3, 2, 126
FRAMES = [34, 35, 34 + 2 * MF.RUN_FRAMES + 3]
TMAX = max(FRAMES) + 5
STRIDES = [1, 2, 17, 34, 40]
RTOL = 1e-9                                     # tests/test_gpu_takes.py: the fp64 distance against its restatement
_AE, _TRACK = {}, {}


def ae_for(latent):
    if latent not in _AE:
        _AE[latent] = load_synth_weights(MotionAE(D_, latent), 41).eval().to(DEV)
    return _AE[latent]


def track(seed=5):
    """(numpy [U, R, Tmax, D] with NaN behind every row's end, the same on the device)."""
    if seed not in _TRACK:
        host = MN.nan_track(U_, R_, TMAX, D_, FRAMES, seed)
        _TRACK[seed] = (host, torch.from_numpy(host).to(DEV))
    return _TRACK[seed]


def chain_rows(ae, windows):
    """PoseEncoderConv.net layer by layer through motion_ae._conv on windows [n, 34, D], flattened: the existing per-layer route."""
    net = ae.encoder.net
    x = windows.transpose(1, 2).contiguous()
    for blk in (net[0], net[1], net[2]):
        x = _conv(x, blk[0], blk[1], stride=blk[0].stride, padding=blk[0].padding, leaky=True)
    return _conv(x, net[3]).flatten(1).contiguous()


# ---- 1: bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latent", [32, 128])
@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("stride", STRIDES)
def test_rows_and_features_equal_the_chain_on_host_cut_windows_bit_for_bit(stride, tail, latent):
    ae = ae_for(latent)
    host, trk = track()
    windows = torch.from_numpy(MN.cut_windows(host, FRAMES, stride, tail)).to(DEV)
    N = windows.shape[0]
    with torch.no_grad():
        want_rows = chain_rows(ae, windows)
        want_feat = ae.encoder(windows)
    rows, plan = MF.window_rows(ae, trk, FRAMES, stride=stride, tail=tail)
    feat, plan_f = MF.window_features(ae, trk, FRAMES, stride=stride, tail=tail)
    torch.cuda.synchronize()
    assert plan is plan_f and N == R_ * plan.total and tuple(rows.shape) == (N, 384) and tuple(feat.shape) == (N, latent)
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(feat).all())
    assert torch.equal(rows, want_rows)
    assert torch.equal(feat, want_feat)
    # ranges that split runs: a row does not depend on the range it was computed in
    for c0, c1 in {(1, N - 1) if N > 2 else (0, N), (N // 3, N // 3 + max(1, N // 4)), (N - 1, N)}:
        part, _ = MF.window_rows(ae, trk, FRAMES, stride=stride, tail=tail, clips=(c0, c1))
        torch.cuda.synchronize()
        assert torch.equal(part, rows[c0:c1]), (c0, c1)
    # a three-dimensional track is one take per recording
    one, plan1 = MF.window_rows(ae, trk[:, 1].contiguous(), FRAMES, stride=stride, tail=tail)
    u, r, _s = MF.clip_index(plan, R_)
    torch.cuda.synchronize()
    assert plan1.total * 1 == one.shape[0] and torch.equal(one, rows[torch.from_numpy(r == 1).to(DEV)])


@pytest.mark.parametrize("stride", [3, 12, 13, 29, 30, 31, 32, 33, 35])
def test_strides_on_both_sides_of_every_change_of_path(stride):
    """The kernel changes form with the stride: the dense conv3 / conv4 up to stride 12 (full runs of 8 windows; 13 is per window), one shared
    span of conv2 positions below 30, of conv1 positions below 32, of poses below 34, windows staged apart from 34 on."""
    ae = ae_for(32)
    host, trk = track()
    windows = torch.from_numpy(MN.cut_windows(host, FRAMES, stride, True)).to(DEV)
    with torch.no_grad():
        want = chain_rows(ae, windows)
    rows, _plan = MF.window_rows(ae, trk, FRAMES, stride=stride)
    torch.cuda.synchronize()
    assert torch.equal(rows, want)


def test_pose_widths_up_to_the_maximum_and_chunked_features():
    """D = 128 (16-byte rows, the widest the LDS plan holds) and D = 5; window_features in ranges of 7 clips equals the encoder run in those ranges."""
    frames = [70, 34]
    for D in (128, 5):
        ae = load_synth_weights(MotionAE(D, 32), 43).eval().to(DEV)
        host = MN.nan_track(2, 2, 72, D, frames, 9)
        trk = torch.from_numpy(host).to(DEV)
        windows = torch.from_numpy(MN.cut_windows(host, frames, 3, True)).to(DEV)
        rows, _plan = MF.window_rows(ae, trk, frames, stride=3)
        feat, _plan = MF.window_features(ae, trk, frames, stride=3, chunk_clips=7)
        with torch.no_grad():
            want = torch.cat([ae.encoder(windows[c0:c0 + 7]) for c0 in range(0, windows.shape[0], 7)])
            assert torch.equal(rows, chain_rows(ae, windows)), D
        torch.cuda.synchronize()
        assert torch.equal(feat, want), D


# ---- 2: float64, independent of the existing kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("stride", STRIDES)
def test_rows_lie_within_the_a_priori_bound_of_the_float64_tower(stride, tail):
    ae = ae_for(32)
    host, trk = track()
    net = ae.encoder.net
    weights = [tuple(t.cpu() for t in _conv_pack(blk[0], DEV, blk[1])) for blk in (net[0], net[1], net[2])]
    weights.append(tuple(t.cpu() for t in _conv_pack(net[3], DEV)))
    ref, bound = MN.tower_f64(torch.from_numpy(MN.cut_windows(host, FRAMES, stride, tail)), weights)
    rows, _plan = MF.window_rows(ae, trk, FRAMES, stride=stride, tail=tail)
    torch.cuda.synchronize()
    got = rows.cpu().view(-1, 32, 12)
    whole, sl, el = compare_sliced(got, ref, bound, f"motion rows stride {stride} tail {tail}", axes=("clip", "channel", "position"))
    print(f"stride {stride} tail {tail}: whole {whole:.3g}, worst slice {sl:.3g}, worst element {el:.3g} of the bound; bound / |ref| rms "
          f"{float(bound.norm() / ref.norm()):.3g}")


# ---- 3: the reference's golden --------------------------------------------------------------------------------------------------------
def test_three_golden_clips_as_one_track():
    G = np.load(os.path.join(HERE, "golden", "motion_ae.npz"))
    clips = ((hash_unit("ae.in", 3 * 34 * 126, 1) * 2 - 1) * 0.8).astype(np.float32).reshape(3, 34, 126)      # tests/test_motion_ae.py: poses
    feat, plan = MF.window_features(ae_for(128), torch.from_numpy(clips.reshape(1, 1, 102, 126)).to(DEV), stride=34)
    torch.cuda.synchronize()
    assert plan.counts.tolist() == [3] and tuple(feat.shape) == (3, 128)
    err = np.linalg.norm(feat.cpu().numpy() - G["z"]) / np.linalg.norm(G["z"])
    print("relative norm against the golden latents", err)
    assert err < 2e-5


# ---- 4: take diversity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [None, 1])
def test_take_diversity_equals_the_float64_restatement_on_the_features(span):
    ae = ae_for(32)
    _host, trk = track()
    feat, plan = MF.window_features(ae, trk, FRAMES, stride=17)
    out = takes.take_diversity(ae, trk, FRAMES, span=span, stride=17)
    torch.cuda.synchronize()
    want_d, want_v = T.take_distance_np(feat.cpu().numpy(), plan.counts.tolist(), R_, span=span)
    dist, div = out["distance"].cpu().numpy(), out["diversity"].cpu().numpy()
    assert dist.shape == (U_, R_, R_) and dist.dtype == np.float64 and (want_d[:, 0, 1] > 0).all()
    np.testing.assert_allclose(dist, want_d, rtol=RTOL, atol=0)
    np.testing.assert_allclose(div, want_v, rtol=RTOL, atol=0)


# ---- 5: the evaluator -----------------------------------------------------------------------------------------------------------------
def test_evaluator_push_tracks_equals_push_samples_on_the_same_clips():
    from types import SimpleNamespace
    from emotiongestures_amd.model.embedding_space_evaluator import EmbeddingSpaceEvaluator
    args = SimpleNamespace(n_pre_poses=4, n_poses=34, pose_dim=126, wordembed_dim=300)
    ckpt = {"pose_dim": 126, "latent_dim": 128, "motion_ae": ae_for(128).state_dict()}
    by_clip, by_track = EmbeddingSpaceEvaluator(args, ckpt, None, DEV), EmbeddingSpaceEvaluator(args, ckpt, None, DEV)
    real = torch.from_numpy(hash_uniform("motionfeat/real", (4, 34, 126), -0.8, 0.8, 3)).to(DEV)
    gen = (real * 0.9 + 0.1 * torch.from_numpy(hash_uniform("motionfeat/gen", (4, 34, 126), -0.8, 0.8, 4)).to(DEV)).contiguous()
    by_clip.push_samples(None, None, gen, real)
    plan = by_track.push_tracks(gen.reshape(1, 136, 126), real.reshape(1, 136, 126), stride=34)
    assert plan.counts.tolist() == [4] and by_track.get_no_of_samples() == 1
    assert np.array_equal(by_track.real_feat_list[0], by_clip.real_feat_list[0])
    assert np.array_equal(by_track.generated_feat_list[0], by_clip.generated_feat_list[0])
    assert by_track.recon_err_diff == [] and by_track.cos_err_diff == [] and len(by_clip.recon_err_diff) == 1
    np.testing.assert_equal(by_track.get_scores(), by_clip.get_scores())


# ---- 6: capture -----------------------------------------------------------------------------------------------------------------------
def test_one_range_of_rows_and_out_net_captures_into_a_graph():
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    ae = ae_for(32)
    contents = [torch.from_numpy(MN.nan_track(U_, R_, TMAX, D_, FRAMES, 20 + i)).to(DEV) for i in range(3)]
    trk = contents[0].clone()
    c0, c1 = 5, 37                                                              # the tail window of recording 1 and part of recording 2: splits a run
    rows = torch.empty(c1 - c0, 384, device=DEV)
    _r, plan = MF.window_rows(ae, trk, FRAMES, stride=17, clips=(c0, c1), out=rows)      # eager warm-up: packs, table, LDS opt-in
    MF.out_net(ae, rows)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
        MF.window_rows(ae, trk, FRAMES, stride=17, clips=(c0, c1), out=rows)
        feat = MF.out_net(ae, rows)
    for new in contents[1:]:
        trk.copy_(new)
        rows.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want_rows, _p = MF.window_rows(ae, new, FRAMES, stride=17, clips=(c0, c1))
        want = MF.out_net(ae, want_rows)
        torch.cuda.synchronize()
        assert torch.equal(rows, want_rows) and torch.equal(feat, want)
    assert plan.total == 1 + 2 + 18


# ---- 7: end to end --------------------------------------------------------------------------------------------------------------------
def test_harness_synthesize_takes_with_a_motion_ae_end_to_end():
    from emotiongestures_amd import harness as H
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    F_, P_, HOP = 34, 4, 32000
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision="bf16x3").to(DEV)
    vae = load_synth_weights(MLP_Reconstruct_v3(frames=F_), 7).eval().to(DEV)
    ae = ae_for(32)
    U, Rd, lengths, wp = 2, 2, [2 * HOP + 5000, HOP + 700], (3, 2)
    audio = torch.from_numpy(synth_audio(U, max(lengths), seed=430)).to(DEV)
    inp = RN.rollout_inputs(U, max(wp), F_, D_, P_, seed=430)
    text, seed_pose = torch.from_numpy(inp["text"]).to(DEV), torch.from_numpy(inp["seed_pose"]).to(DEV)
    labels = torch.from_numpy(inp["label"]).to(DEV)
    z = torch.from_numpy(hash_uniform("motionfeat/z", (U, Rd, max(wp), 32), -2.0, 2.0, 430))
    kw = dict(lengths=lengths, draws=Rd, z=z, hop_samples=HOP)
    plain = H.synthesize_takes((model, vae), audio, text, seed_pose, labels, **kw)
    out = H.synthesize_takes((model, vae), audio, text, seed_pose, labels, diversity=ae, **kw)
    torch.cuda.synchronize()
    assert set(out) == set(plain) | {"take_distance", "take_diversity"} and torch.equal(out["track"], plain["track"])
    frames = [w * (F_ - P_) + P_ for w in wp]
    assert out["windows_per"] == list(wp) and frames == [94, 64]
    d = out["take_distance"].cpu().numpy()
    assert d.shape == (2, 2, 2) and d.dtype == np.float64 and tuple(out["take_diversity"].shape) == (2,)
    assert np.array_equal(d, d.transpose(0, 2, 1)) and not d[:, np.eye(2, dtype=bool)].any() and (d[:, 0, 1] > 0).all()
    want = takes.take_diversity(ae, out["track"], frames, span=1, stride=34)
    torch.cuda.synchronize()
    assert torch.equal(out["take_distance"], want["distance"]) and torch.equal(out["take_diversity"], want["diversity"])
    half = H.synthesize_takes((model, vae), audio, text, seed_pose, labels, diversity=ae, diversity_stride=17, **kw)
    want = takes.take_diversity(ae, out["track"], frames, span=1, stride=17)
    torch.cuda.synchronize()
    assert torch.equal(half["take_distance"], want["distance"]) and not torch.equal(half["take_distance"], out["take_distance"])
