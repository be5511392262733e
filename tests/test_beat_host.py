"""Beat-alignment score, host side (CPU): the drop-in alignment's load_pose / calculate_align against the reference's own
model/Beat_score_v2.py (tests/golden/beat_align.npz from tests/golden/make_golden_beat.py), the opt-in model.Beat_score_v2 alias, and the
test-side numpy restatement of the audio half (tests/beat_np.py) against independent implementations of its pieces."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
from make_golden_beat import full_pose  # noqa: E402

import beat_np  # noqa: E402


def _golden():
    z = np.load(os.path.join(GOLDEN, "beat_align.npz"))
    return z, full_pose(z["joints"])


def _sets_from_counts(c):
    return np.repeat(np.arange(c.shape[-1]), c.astype(np.int64))


def test_load_pose_reproduces_reference_beat_sets():
    from emotiongestures_amd.beat import alignment
    z, pose = _golden()
    al = alignment(0.3, 2)
    for i in range(pose.shape[0]):
        t0, t1, fps = (int(v) for v in z["meta"][i])
        sets = al.load_pose(pose[i], t0, t1, fps, True)
        assert len(sets) == 8 and all(isinstance(s, tuple) and len(s) == 1 for s in sets)
        for q, s in enumerate(sets):
            assert np.array_equal(s[0], np.flatnonzero(z["pose_beats"][i, q])), (i, q)


def test_calculate_align_reproduces_reference_scores():
    from emotiongestures_amd.beat import alignment
    z, pose = _golden()
    al = alignment(0.3, 2)
    for i in range(pose.shape[0]):
        t0, t1, fps = (int(v) for v in z["meta"][i])
        ons = [_sets_from_counts(z["onsets"][i, a]) for a in range(3)]
        got = al.calculate_align(*ons, *al.load_pose(pose[i], t0, t1, fps, True), fps)
        assert abs(got - z["score"][i]) <= 1e-12, (i, got, z["score"][i])
    assert z["score"][-1] == 0.0                         # the still clip: no pose beat -> every GAHR term is exp(-inf) = 0


def test_host_error_cases_match_reference():
    from emotiongestures_amd.beat import alignment
    z, pose = _golden()
    assert z["errors"].tolist() == [1, 1]               # the reference raised IndexError (D=126) and ZeroDivisionError (no onsets)
    al = alignment(0.3, 2)
    with pytest.raises(ValueError):
        al.load_pose(pose[0][:, :126], 0, 4, 15, True)
    e = np.array([], np.int64)
    with pytest.raises(ZeroDivisionError):
        al.calculate_align(e, e, e, *al.load_pose(pose[0], 0, 4, 15, True), 15)


def test_unimplemented_methods_still_refuse():
    from emotiongestures_amd import beat
    al = beat.alignment(0.3, 2)
    with pytest.raises(NotImplementedError):
        al.audio_beat_vis(None, None, None)
    with pytest.raises(NotImplementedError):
        beat.L1div()
    with pytest.raises(NotImplementedError):
        beat.SRGR()


def test_batched_path_has_no_cpu_fallback():
    from emotiongestures_amd.beat import beat_alignment
    with pytest.raises(RuntimeError):
        beat_alignment(torch.zeros(1, 16000), torch.zeros(1, 60, 282))


def _child(code):
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_install_aliases_default_still_refuses_beat_score():
    _child("import emotiongestures_amd as E; E.install_aliases()\n"
           "from model.Beat_score_v2 import alignment\n"
           "from emotiongestures_amd.model import Beat_score_v2 as stub\n"
           "assert alignment is stub.alignment\n"
           "try:\n"
           "    alignment(0.3, 2).load_pose(None, 0, 4, 15, True)\n"
           "    raise SystemExit('load_pose did not refuse')\n"
           "except NotImplementedError:\n"
           "    pass\n"
           "print('ok')\n")


def test_install_aliases_beat_score_resolves_the_metric():
    _child("import emotiongestures_amd as E; E.install_aliases(beat_score=True)\n"
           "from model.Beat_score_v2 import alignment\n"
           "from emotiongestures_amd import beat\n"
           "assert alignment is beat.alignment\n"
           "import numpy as np\n"
           "al = alignment(0.3, 2)\n"
           "pose = np.cumsum(np.random.default_rng(0).standard_normal((60, 282)).astype(np.float32), 0)\n"
           "s = al.calculate_align(np.array([10]), np.array([8]), np.array([9]), *al.load_pose(pose, 0, 4, 15, True), 15)\n"
           "assert 0.0 < s <= 1.0\n"
           "print('ok')\n")


# ---- the numpy restatement of the audio half against independent implementations of its pieces ----------------------------------------
def test_restatement_filterbank_matches_transformers_slaney():
    tau = pytest.importorskip("transformers.audio_utils")
    from oracle import emogest_oracle as O
    ours = O.mel_filterbank(16000, 2048, 128).astype(np.float64)
    theirs = tau.mel_filter_bank(num_frequency_bins=1025, num_mel_filters=128, min_frequency=0.0, max_frequency=8000.0,
                                 sampling_rate=16000, norm="slaney", mel_scale="slaney").T
    assert ours.shape == theirs.shape == (128, 1025)
    assert np.abs(ours - theirs).max() <= 1e-6 * np.abs(theirs).max()


def test_restatement_power_spectrum_matches_torch_stft():
    y = np.random.default_rng(5).standard_normal(48123).astype(np.float32)
    P = beat_np.stft_power(y)
    X = torch.stft(torch.from_numpy(y).double(), n_fft=2048, hop_length=512, window=torch.hann_window(2048, periodic=True, dtype=torch.float64),
                   center=True, pad_mode="constant", return_complex=True)
    ref = (X.abs() ** 2).numpy()
    assert P.shape == ref.shape == (1025, 1 + 48123 // 512)
    assert np.abs(P - ref).max() <= 1e-6 * ref.max()          # the restatement uses the kernel's fp32 Hann table (oracle.hann_periodic)


def test_restatement_picks_on_a_hand_made_envelope():
    """peak_pick / backtrack on a small envelope whose answer is worked out by hand: peaks need x[n] >= x[n-1] and x[n] >= mean(x[n-4:n+5])
    + 0.07, the frame after an accepted peak is skipped, each onset backtracks to the last local minimum at or before it."""
    oenv = np.array([0, 0, 0, 0.2, 1.0, 1.0, 0.1, 0.05, 0.6, 0.2, 0.0, 0.0, 0.6, 0.1, 0.0, 0.0], np.float32)
    x = beat_np.normalise(oenv)
    raw, _ = beat_np.peak_pick(x)
    assert raw.tolist() == [4, 8, 12]                    # 5 is skipped (wait), 8 beats its window mean by > 0.07
    flag, _ = beat_np.minima(oenv)
    assert np.flatnonzero(flag).tolist() == [0, 2, 7, 11]
    assert beat_np.backtrack(raw, flag).tolist() == [2, 7, 11]


def test_restatement_matches_librosa_where_installed():
    librosa = pytest.importorskip("librosa", reason="librosa is not installed on this image: the restatement is unpinned against it here")
    y = np.random.default_rng(9).standard_normal(64000).astype(np.float32) * np.repeat(np.random.default_rng(10).random(125) > 0.6, 512)[:64000]
    r = beat_np.load_audio(y)
    oenv = librosa.onset.onset_strength(y=y, sr=16000)
    assert np.linalg.norm(oenv - r["oenv"]) <= 1e-5 * np.linalg.norm(oenv)
    raw = librosa.onset.onset_detect(onset_envelope=oenv, backtrack=False)
    assert np.array_equal(raw, r["raw"])
    assert np.array_equal(librosa.onset.onset_backtrack(raw, oenv), r["bt"])
