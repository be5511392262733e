"""Beat-alignment score on the GPU (eg_beat_align: beat_stft_kernel + beat_align_kernel) against the test-side numpy restatement of
the audio half (tests/beat_np.py), the reference's own pose beat sets (tests/golden/beat_align.npz) and the host calculate_align; the
per-clip drop-in loop of the eval script and harness.evaluate(beat=True)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, build_mirror

sys.path.insert(0, GOLDEN)
from make_golden_beat import full_pose  # noqa: E402

import beat_np  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 1e-4


def noise_bursts(b, n, seed):
    """Seeded BEAT-like audio: noise whose level jumps every 512..4096 samples (onsets at the jumps), some stretches silent."""
    rng = np.random.default_rng(seed)
    out = np.zeros((b, n), np.float32)
    for i in range(b):
        env = np.zeros(n, np.float32)
        p = 0
        while p < n:
            L = int(rng.integers(512, 4096))
            env[p:p + L] = 0.0 if rng.random() < 0.25 else rng.uniform(0.01, 1.0)
            p += L
        out[i] = rng.standard_normal(n).astype(np.float32) * env
    return out


def click_train(n, period, first):
    y = np.zeros(n, np.float32)
    y[first::period] = 1.0
    return y


def random_poses(b, f, d, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((b, f, d)).astype(np.float32) * np.float32(0.05), axis=1, dtype=np.float32)


def _beats(audio, pose=None, **kw):
    from emotiongestures_amd.beat import _run, beat_alignment
    a = torch.from_numpy(audio).to(DEV)
    if pose is None:
        _, bt = _run(a, None, 15, 0, 1, 0.3, 2, True)
        sc = None
    else:
        sc, bt = beat_alignment(a, torch.from_numpy(pose).to(DEV), want_beats=True, **kw)
        sc = sc.cpu().numpy()
    torch.cuda.synchronize()
    return sc, {k: (None if v is None else v.cpu().numpy()) for k, v in bt.items()}


def _sets(c):
    return np.repeat(np.arange(c.shape[-1]), c.astype(np.int64))


def _check_audio(audio, bt, exact, tag):
    """oenv / rms within rel-L2 1e-5 of the restatement; beat decisions equal, or (exact=False) differing only where the restatement's
    decision margin is below MARGIN.  Returns the recorded flips."""
    flips = []
    for i, y in enumerate(audio):
        r = beat_np.load_audio(y)
        T = r["oenv"].size
        for k in ("oenv", "rms"):
            ref, got = r[k].astype(np.float64), bt[k][i].astype(np.float64)
            assert np.linalg.norm(got - ref) <= 1e-5 * max(np.linalg.norm(ref), 1e-30), (tag, i, k, np.linalg.norm(got - ref) / np.linalg.norm(ref))
        got_raw = np.flatnonzero(bt["audio_beats"][i, 0])
        assert bt["n_audio_beats"][i] == got_raw.size
        if exact:
            assert np.array_equal(got_raw, r["raw"]), (tag, i)
            assert np.array_equal(bt["audio_beats"][i, 1], beat_np.counts(r["bt"], T)), (tag, i)
            assert np.array_equal(bt["audio_beats"][i, 2], beat_np.counts(r["bt_rms"], T)), (tag, i)
            continue
        fragile = np.flatnonzero(r["peak_margin"] < MARGIN)
        for n in np.flatnonzero(beat_np.counts(got_raw, T) != beat_np.counts(r["raw"], T)):
            near = fragile[np.abs(fragile - n) <= 2]
            assert near.size, f"{tag} clip {i}: onset flip at frame {n} without a decision margin < {MARGIN} near it"
            flips.append((tag, i, "raw", int(n), float(r["peak_margin"][near].min())))
        # backtracks of the GPU's own onsets: against the restatement's minima, except where a minimum decision is within MARGIN
        for a, (flag, mm) in enumerate(zip(r["min_flag"], r["min_margin"]), start=1):
            ref_bt = beat_np.backtrack(got_raw, flag)
            got_bt = _sets(bt["audio_beats"][i, a])
            for e, g, f in zip(got_raw, got_bt, ref_bt):
                if g != f:
                    lo = min(g, f)
                    assert (mm[lo:e + 1] < MARGIN).any(), f"{tag} clip {i}: backtrack {a} of onset {e}: {g} vs {f}"
                    flips.append((tag, i, f"bt{a}", int(e), float(mm[lo:e + 1].min())))
    for fl in flips:
        print("beat decision flip (restatement margin < 1e-4):", fl)
    return flips


def test_audio_half_matches_restatement_on_beat_noise():
    audio = noise_bursts(64, 64000, 1)
    _, bt = _beats(audio)
    assert bt["oenv"].shape == (64, 126) and (bt["n_audio_beats"] > 0).all()
    flips = _check_audio(audio, bt, exact=False, tag="beat64")
    assert len(flips) <= 8


def test_audio_half_on_long_and_odd_length_clips():
    for n, b, seed in ((160000, 4, 2), (48123, 3, 3)):
        audio = noise_bursts(b, n, seed)
        _, bt = _beats(audio)
        assert bt["oenv"].shape == (b, 1 + n // 512)
        _check_audio(audio, bt, exact=False, tag=f"n{n}")


def test_audio_beats_exact_on_click_train():
    audio = np.stack([click_train(64000, 4000, 1500), click_train(64000, 5333, 700), click_train(64000, 3000, 2100)])
    _, bt = _beats(audio)
    assert (bt["n_audio_beats"] >= 10).all()
    _check_audio(audio, bt, exact=True, tag="clicks")


def test_pose_beats_bitwise_equal_reference_golden():
    from emotiongestures_amd.beat import alignment
    z = np.load(os.path.join(GOLDEN, "beat_align.npz"))
    pose = full_pose(z["joints"])
    audio = noise_bursts(pose.shape[0], 64000, 4)
    al = alignment(0.3, 2)
    for key in sorted({tuple(int(v) for v in m) for m in z["meta"]}):
        idx = np.flatnonzero((z["meta"] == np.array(key)).all(1))
        t0, t1, fps = key
        sc, bt = _beats(audio[idx], pose[idx], fps=fps, t_start=t0, t_end=t1)
        assert np.array_equal(bt["pose_beats"], z["pose_beats"][idx]), key
        for j, i in enumerate(idx):             # scores against the host calculate_align on the same beat sets
            ons = [_sets(bt["audio_beats"][j, a]) for a in range(3)]
            ref = al.calculate_align(*ons, *al.load_pose(pose[i], t0, t1, fps, True), fps)
            assert abs(sc[j] - ref) <= 1e-12, (key, i, sc[j], ref)


@pytest.mark.parametrize("B", [1, 7, 64, 256])
def test_batched_scores_match_host_calculate_align_and_are_deterministic(B):
    from emotiongestures_amd.beat import alignment, beat_alignment
    audio = noise_bursts(B, 64000, 10 + B)
    pose = random_poses(B, 60, 282, 20 + B)
    sc, bt = _beats(audio, pose)
    al = alignment(0.3, 2)
    for i in range(B):
        sets = al.load_pose(pose[i], 0, 4, 15, True)
        assert all(np.array_equal(s[0], np.flatnonzero(bt["pose_beats"][i, q])) for q, s in enumerate(sets)), i
        ref = al.calculate_align(*[_sets(bt["audio_beats"][i, a]) for a in range(3)], *sets, 15)
        assert abs(sc[i] - ref) <= 1e-12, (i, sc[i], ref)
    a, p = torch.from_numpy(audio).to(DEV), torch.from_numpy(pose).to(DEV)
    s1, s2 = beat_alignment(a, p), beat_alignment(a, p)
    assert torch.equal(s1, s2) and np.array_equal(s1.cpu().numpy(), sc)


def test_silent_clip_is_nan_and_leaves_neighbours_alone():
    from emotiongestures_amd.beat import beat_alignment
    audio = noise_bursts(3, 64000, 30)
    audio[1] = 0.0
    pose = random_poses(3, 60, 282, 31)
    sc, bt = _beats(audio, pose)
    assert np.isnan(sc[1]) and bt["n_audio_beats"][1] == 0 and not bt["audio_beats"][1].any()
    for i in (0, 2):
        solo = beat_alignment(torch.from_numpy(audio[i:i + 1]).to(DEV), torch.from_numpy(pose[i:i + 1]).to(DEV)).cpu().numpy()
        assert solo[0] == sc[i] and np.isfinite(sc[i])


_LOOP = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import emotiongestures_amd as E
E.install_aliases(beat_score=True)
from model.Beat_score_v2 import alignment
in_audio = torch.from_numpy(np.load(sys.argv[2]))
pred_pose_np = np.load(sys.argv[3])
test_batch_size, motion_resampling_framerate, n_poses = in_audio.shape[0], 15, pred_pose_np.shape[1]
# test_emotion_gesture_diversity_iterative.py:185-190, 241-248, 258
alignmenter = alignment(0.3, 2)
t_start = 0
t_end = int(n_poses / motion_resampling_framerate)
BL_score = 0.
for batch_idx in range(test_batch_size):
    audio = in_audio[batch_idx, :]
    onset_raw, onset_bt, onset_bt_rms = alignmenter.load_audio(audio.cpu().numpy().reshape(-1), t_start, True)
    beat_right_arm, beat_right_shoulder, beat_right_fore_arm, beat_right_wrist, beat_left_arm, beat_left_shoulder, beat_left_fore_arm, beat_left_wrist = alignmenter.load_pose(pred_pose_np[batch_idx, :, :], t_start, t_end, motion_resampling_framerate, True)
    BL_score += alignmenter.calculate_align(onset_raw, onset_bt, onset_bt_rms, beat_right_arm, beat_right_shoulder, beat_right_fore_arm, beat_right_wrist, beat_left_arm, beat_left_shoulder, beat_left_fore_arm, beat_left_wrist, motion_resampling_framerate)
avf_BL_score = BL_score / (1 * test_batch_size)
assert alignmenter.oenv.shape == (126,) and alignmenter.rms.shape == (1, 126) and alignmenter.S is None
assert np.allclose(alignmenter.times, np.arange(126) * 512 / 22050)
print(repr(avf_BL_score))
'''


def test_reference_drop_in_loop_matches_batched_mean(tmp_path):
    from emotiongestures_amd.beat import beat_alignment
    audio = noise_bursts(8, 64000, 40)
    pose = random_poses(8, 60, 282, 41)
    np.save(tmp_path / "audio.npy", audio)
    np.save(tmp_path / "pose.npy", pose)
    (tmp_path / "loop.py").write_text(_LOOP)
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py"), ROOT, str(tmp_path / "audio.npy"), str(tmp_path / "pose.npy")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    loop = float(r.stdout.strip().splitlines()[-1])
    batched = float(beat_alignment(torch.from_numpy(audio).to(DEV), torch.from_numpy(pose).to(DEV)).mean())
    assert abs(loop - batched) <= 1e-12, (loop, batched)


def test_harness_evaluate_beat_opt_in():
    from emotiongestures_amd import harness as H
    from emotiongestures_amd.beat import beat_alignment
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.model.FGD import MLP_Reconstruct
    from emotiongestures_amd.skeleton_classifer.Models import Transformer as Skel
    from emotiongestures_amd.synth import hash_uniform, load_synth_weights, synth_inputs
    F, D, P = 60, 282, 10
    gen = build_mirror("spatial", F, D, P, 10, seed=31).to(DEV)
    vae = load_synth_weights(MLP_Reconstruct_v3(), 31).eval().to(DEV)
    fgd = load_synth_weights(MLP_Reconstruct(), 31).eval().to(DEV)
    skel = load_synth_weights(Skel(class_dim=8, pose_dim=282, d_word_vec=512, d_model=512, d_inner=2048, n_layers=3, n_head=8, d_k=64,
                                   d_v=64, n_position=60), 31).eval().to(DEV)
    batches, zs = [], []
    for i in range(2):
        inp = synth_inputs(3, F, D, P, seed=40 + i)
        pose = torch.from_numpy(hash_uniform(f"h/pose{i}", (3, F, D), -0.5, 0.5, 40 + i))
        batches.append({"spec": torch.from_numpy(inp["spec"]), "text": torch.from_numpy(inp["text"]), "pose_seq": pose,
                        "label": torch.from_numpy(inp["label"]), "audio": torch.from_numpy(noise_bursts(3, 64000, 50 + i))})
        zs.append(torch.from_numpy(inp["z"]))
    np.random.seed(99)
    plain = H.evaluate(gen, vae, fgd, skel, batches, P, device=DEV, z_list=zs)
    np.random.seed(99)
    with_beat = H.evaluate(gen, vae, fgd, skel, batches, P, device=DEV, z_list=zs, beat=True)
    assert "beat" not in plain and set(with_beat) == set(plain) | {"beat"}
    for k, v in plain.items():
        assert with_beat[k] == v or (np.isnan(v) and np.isnan(with_beat[k])), k
    scores = []
    with torch.no_grad():
        for bt, z in zip(batches, zs):
            sampled = vae.sample(bt["label"].to(DEV), z=z)
            pose = gen(bt["spec"].to(DEV), bt["text"].to(DEV), bt["pose_seq"][:, :P].contiguous().to(DEV), sampled)[0]
            scores.append(beat_alignment(bt["audio"].to(DEV), pose).cpu().numpy())
    assert abs(with_beat["beat"] - float(np.mean(np.concatenate(scores)))) <= 1e-12
    silent = [dict(batches[0], audio=torch.zeros(3, 64000))]
    with pytest.raises(ValueError, match="batch 0 clip 0"):
        H.evaluate(gen, vae, fgd, skel, silent, P, device=DEV, z_list=zs[:1], beat=True)
