#!/usr/bin/env python3
"""Beat-alignment score timing: the batched GPU path (eg_beat_align, two kernels) at B = 64 and 256 BEAT clips (64 000 samples of 16 kHz
audio, 60 x 282 poses), device events after warm-up; and, for comparison, the per-clip drop-in loop of the eval script
(alignment.load_audio + load_pose + calculate_align, test_emotion_gesture_diversity_iterative.py:241-248) on a few clips.
Prints one JSON line.  Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_beat.py` separately.

    python tools/bench_beat.py [--iters 200] [--loop-clips 16] [--out profiles/beat_bench_line.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(b, seed):
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.uniform(0.0, 1.0, (b, 126)) * (rng.random((b, 126)) > 0.3), 512, axis=1)[:, :64000]
    audio = (rng.standard_normal((b, 64000)) * env).astype(np.float32)
    pose = np.cumsum(rng.standard_normal((b, 60, 282)).astype(np.float32) * np.float32(0.05), axis=1, dtype=np.float32)
    return audio, pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop-clips", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd.beat import alignment, beat_alignment
    dev = torch.device("cuda:0")
    res = {"metric": "beat_alignment", "clip": "64000 samples @16 kHz, pose 60x282, fps 15, sigma 0.3, order 2"}
    for B in (64, 256):
        audio, pose = inputs(B, B)
        au, po = torch.from_numpy(audio).to(dev), torch.from_numpy(pose).to(dev)
        for _ in range(a.warmup):
            beat_alignment(au, po)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            s = beat_alignment(au, po)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        res[f"batched_ms_B{B}"] = round(ms, 4)
        res[f"batched_us_per_clip_B{B}"] = round(1000 * ms / B, 3)
        res[f"finite_B{B}"] = int(torch.isfinite(s).sum())
    audio, pose = inputs(a.loop_clips, 7)
    al = alignment(0.3, 2)
    al.load_audio(audio[0], 0, True)            # warm-up (tables, allocator)
    t0 = time.perf_counter()
    for i in range(a.loop_clips):
        o = al.load_audio(audio[i], 0, True)
        al.calculate_align(*o, *al.load_pose(pose[i], 0, 4, 15, True), 15)
    res["dropin_loop_ms_per_clip"] = round(1000 * (time.perf_counter() - t0) / a.loop_clips, 3)
    res["dropin_loop_ms_B64_est"] = round(64 * res["dropin_loop_ms_per_clip"], 2)
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
