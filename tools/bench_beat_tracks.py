#!/usr/bin/env python3
"""Beat-alignment score of whole recordings (beat.beat_alignment_tracks / eg_beat_align_tracks) timed as one hipGraph per call, device
events after warm-up, every timed window sized to at least --window-s seconds of replays.

Against what the clip call can do: U = 8 recordings of 30 s with R = 1 and R = 8 draws; the baseline is `beat_alignment` at batch 8 and at
batch 64 with the audio repeated 8 times (the only way the clip call scores those shapes).  New call and baselines alternate inside one
process for --rounds rounds; the baseline's min-max over the rounds is the run-to-run spread reported beside each ratio.
Where no baseline exists: (U, seconds, R) = (8, 60, 8), (1, 600, 1) and 64 recordings of 10-90 s with 4 draws: ms per call and us per
scored track.  Prints one JSON line.

Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_beat_tracks.py --eager-case ten_min

    python tools/bench_beat_tracks.py [--rounds 5] [--window-s 0.4] [--out profiles/beat_tracks_bench_line.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import alternate, graph_of, summary, write_line  # noqa: E402
SR, FPS = 16000, 15


def make(lengths, R, seed):
    """Noise whose level jumps every 512..4096 samples (onsets at the jumps), cumulative-sum poses; -> audio [U, max], track [U, R, Tmax, 282]."""
    rng = np.random.default_rng(seed)
    U, stride = len(lengths), max(lengths)
    audio = np.zeros((U, stride), np.float32)
    for u, n in enumerate(lengths):
        env = np.repeat(rng.uniform(0.0, 1.0, n // 2048 + 1) * (rng.random(n // 2048 + 1) > 0.25), 2048)[:n]
        audio[u, :n] = (rng.standard_normal(n) * env).astype(np.float32)
    frames = [n * FPS // SR for n in lengths]
    track = np.cumsum(rng.standard_normal((U, R, max(frames), 282)).astype(np.float32) * np.float32(0.05), axis=2, dtype=np.float32)
    return audio, track, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--eager-case", default=None, choices=["ten_min", "u8_60s_r8", "ragged64_r4", "u8_30s_r8"],
                    help="run that case eagerly --eager-iters times and exit (for a rocprofv3 kernel trace)")
    ap.add_argument("--eager-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd.beat import beat_alignment, beat_alignment_tracks
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(x).to(dev)
    rng = np.random.default_rng(64)
    cases = {"u8_30s_r8": ([30 * SR] * 8, 8), "u8_60s_r8": ([60 * SR] * 8, 8), "ten_min": ([600 * SR], 1),
             "ragged64_r4": ([int(v) for v in rng.integers(10 * SR, 90 * SR, 64)], 4)}
    if a.eager_case:
        lengths, R = cases[a.eager_case]
        audio, track, frames = make(lengths, R, 1)
        au, tr = up(audio), up(track)
        for _ in range(a.eager_iters):
            s = beat_alignment_tracks(au, tr, lengths=lengths, frames=frames)
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "finite": int(torch.isfinite(s).sum())}))
        return

    res = {"metric": "beat_alignment_tracks", "unit": "one hipGraph per call, device events", "rounds": a.rounds, "window_s": a.window_s,
           "pose": "282 columns, 15 fps, sigma 0.3, order 2"}
    # ---- against the clip call: 8 recordings of 30 s (T = 938 onset frames, 450 poses)
    lengths = [30 * SR] * 8
    for R in (1, 8):
        audio, track, frames = make(lengths, R, 10 + R)
        au, tr = up(audio), up(track)
        au_rep = au[:, None, :].expand(8, R, au.shape[1]).reshape(8 * R, -1).contiguous()
        po_rep = tr.reshape(8 * R, tr.shape[2], 282).contiguous()
        g_new, s_new = graph_of(lambda: beat_alignment_tracks(au, tr, lengths=lengths, frames=frames))
        g_old, s_old = graph_of(lambda: beat_alignment(au_rep, po_rep))
        g_old2, _ = graph_of(lambda: beat_alignment(au_rep, po_rep))                       # the baseline again: its own spread
        same = bool(torch.equal(s_new.reshape(-1).view(torch.int64), s_old.view(torch.int64)))
        t, reps = alternate({"tracks": g_new, "clip": g_old, "clip_again": g_old2}, a.rounds, a.window_s, min_reps=20, probe=10)
        base = t["clip"] + t["clip_again"]
        res[f"u8_30s_r{R}"] = {"tracks": summary(t["tracks"]), f"clip_batch{8 * R}": summary(base),
                               "clip_spread_pct": round(100 * (max(base) - min(base)) / statistics.median(base), 2),
                               "clip_over_tracks": round(statistics.median(base) / statistics.median(t["tracks"]), 3),
                               "us_per_track": round(1000 * statistics.median(t["tracks"]) / (8 * R), 3), "scores_bitwise_equal": same,
                               "replays_per_window": reps["tracks"]}
    # ---- where no baseline exists
    for name in ("u8_60s_r8", "ten_min", "ragged64_r4"):
        lengths, R = cases[name]
        audio, track, frames = make(lengths, R, 20 + len(lengths))
        au, tr = up(audio), up(track)
        g_new, s = graph_of(lambda: beat_alignment_tracks(au, tr, lengths=lengths, frames=frames))
        t, reps = alternate({"tracks": g_new}, a.rounds, a.window_s, min_reps=20, probe=10)
        res[name] = {"recordings": len(lengths), "draws": R, "seconds": [round(min(lengths) / SR, 1), round(max(lengths) / SR, 1)],
                     "onset_frames": int(sum(1 + n // 512 for n in lengths)), **summary(t["tracks"]),
                     "us_per_track": round(1000 * statistics.median(t["tracks"]) / (len(lengths) * R), 3),
                     "finite": int(torch.isfinite(s).sum()), "replays_per_window": reps["tracks"]}
    res["device"] = torch.cuda.get_device_name(dev)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
