#!/usr/bin/env python3
"""Generate tests/golden/beat_align.npz from the reference's own model/Beat_score_v2.py (alignment.load_pose / calculate_align).

Build container only:   python tests/golden/make_golden_beat.py

Imported in place from /root/reference with the empty stand-ins of make_golden_training_types._stubs, plus
`librosa.frames_to_time = frames * 512 / 22050` (librosa's defaults: the only librosa function the pose / score half calls).
The audio half (load_audio) needs librosa proper and is not covered here.

Stored:
  joints [N, 60, 48] fp32: pose columns 18:42 ++ 150:174 (the only ones load_pose reads): seeded random walks with exactly repeated
      frames (zero-velocity plateaus), so that argrelextrema's strict '<' meets ties.  The [N, 60, 282] pose the reference ran on is
      full_pose(joints): the other columns hold a fixed filler, so that reading a wrong column shows;
  meta [N, 3] = (t_start, t_end, fps) per clip (some slice the right side);
  pose_beats [N, 8, 59] uint8: the 8 index sets of load_pose (return order; right-side indices relative to the slice);
  onsets [N, 3, 126] uint8: seeded (onset_raw, onset_bt, onset_bt_rms) frame sets as multiplicities (backtracked sets repeat frames);
  score [N] fp64: calculate_align(onsets, load_pose(pose), fps) of the reference;
  errors [2]: 1 if load_pose raised IndexError on a D = 126 pose, 1 if calculate_align raised ZeroDivisionError on empty onsets.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = "/root/reference"
N, F, D, T = 12, 60, 282, 126


def full_pose(joints):
    """[N, F, 48] joint columns -> [N, F, 282] pose; every other column = a fixed filler pattern."""
    n, f, _ = joints.shape
    pose = np.broadcast_to((np.arange(f * D).reshape(f, D) % 97).astype(np.float32) * np.float32(0.37), (n, f, D)).copy()
    pose[:, :, 18:42] = joints[:, :, :24]
    pose[:, :, 150:174] = joints[:, :, 24:]
    return pose


def poses(rng):
    out = np.zeros((N, F, 48), np.float32)
    for i in range(N):
        steps = rng.standard_normal((F, 48)).astype(np.float32) * np.float32(0.05 * (1 + i % 3))
        p = np.cumsum(steps, axis=0, dtype=np.float32)
        # exactly repeated frames: a zero-velocity plateau, and an isolated repeat
        a = int(rng.integers(5, 40))
        p[a + 1:a + 4] = p[a]
        b = int(rng.integers(45, 58))
        p[b + 1] = p[b]
        if i % 4 == 1:                   # a still clip segment on every joint group at once
            p[20:26] = p[20]
        if i % 4 == 2:                   # frames identical two apart (equal velocity magnitudes around a frame)
            p[30] = p[28]
        out[i] = p
    out[N - 1] = out[N - 1, :1]          # one fully still clip: no pose beat at all (GAHR 0 terms)
    return out


def onset_sets(rng):
    """Seeded ascending frame lists in the shape onset_detect / onset_backtrack produce: raw onsets at least 2 apart, backtracked
    sets mapped to minima <= each onset (duplicates where two onsets share one)."""
    res = []
    for i in range(N):
        n = int(rng.integers(1, 30))
        raw = np.unique(rng.integers(3, T, size=n) // 2 * 2)
        bt = np.maximum(raw - rng.integers(0, 6, size=raw.size), 0)
        bt = np.maximum.accumulate(bt)
        if raw.size > 2:
            bt[1] = bt[0]                # a shared minimum
        bt_rms = np.maximum.accumulate(np.maximum(raw - rng.integers(0, 4, size=raw.size), 0))
        res.append((raw.astype(np.int64), bt.astype(np.int64), bt_rms.astype(np.int64)))
    return res


def main():
    from make_golden_training_types import _stubs
    _stubs()
    sys.modules["librosa"].frames_to_time = lambda frames, sr=22050, hop_length=512, n_fft=None: \
        (np.asanyarray(frames) * hop_length).astype(int) / float(sr)
    sys.path.insert(0, REF)
    sys.modules.pop("model", None)
    from model.Beat_score_v2 import alignment

    rng = np.random.default_rng(20261016)
    joints = poses(rng)
    pose = full_pose(joints)
    meta = np.array([[0, 4, 15]] * N, np.int64)
    meta[3] = (1, 3, 15)                 # right-side curves sliced [15:45]
    meta[7] = (0, 2, 15)                 # [0:30]
    meta[9] = (2, 4, 15)                 # [30:60] -> clipped to the 59 velocities
    ons = onset_sets(rng)
    al = alignment(0.3, 2)
    pose_beats = np.zeros((N, 8, F - 1), np.uint8)
    onsets = np.zeros((N, 3, T), np.uint8)
    score = np.zeros(N, np.float64)
    for i in range(N):
        t0, t1, fps = (int(v) for v in meta[i])
        sets = al.load_pose(pose[i], t0, t1, fps, True)
        assert len(sets) == 8
        for q, s in enumerate(sets):
            pose_beats[i, q, s[0]] = 1
        for a in range(3):
            np.add.at(onsets[i, a], ons[i][a], 1)
        score[i] = al.calculate_align(*ons[i], *sets, fps)
        print(i, [len(s[0]) for s in sets], [len(o) for o in ons[i]], score[i])
    errors = np.zeros(2, np.int64)
    try:
        al.load_pose(pose[0][:, :126], 0, 4, 15, True)
    except IndexError:
        errors[0] = 1
    try:
        e = np.array([], np.int64)
        al.calculate_align(e, e, e, *al.load_pose(pose[0], 0, 4, 15, True), 15)
    except ZeroDivisionError:
        errors[1] = 1
    assert errors.all(), errors
    np.savez_compressed(os.path.join(HERE, "beat_align.npz"), joints=joints, meta=meta, pose_beats=pose_beats, onsets=onsets, score=score,
                        errors=errors)


if __name__ == "__main__":
    main()
