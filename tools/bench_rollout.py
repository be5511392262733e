#!/usr/bin/env python3
"""Long-form synthesis timing: (a) Transformer.synthesize (eg_generator_forward_rollout: everything the prior does not reach once at batch
U*W, then W dependent decoder steps of U clips) against (b) what the library offered before it: a loop of W forward() calls at batch U with
the hand-off and the cross-fade done by torch ops on the device.  Both are captured as ONE hipGraph each and replayed; TED shapes (34 frames,
prior 4, 15 fps), bf16x3.  After a warm-up of every shape the two alternate, `--rounds` timed windows each of `--iters` replays between device
events, every window ending in a device synchronise; the median window is reported.  Launch counts are the library's own (eg_launch_count
while the graph is captured); the torch ops of (b) are not in them.  Prints one JSON line.  Kernel statistics: run one shape under
`rocprofv3 --kernel-trace --stats -- python tools/bench_rollout.py --shapes 64x8` separately.

    python tools/bench_rollout.py [--shapes 1x30,8x30,64x8] [--iters 10] [--rounds 5] [--out profiles/rollout_bench_line.json]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import capture, window_ms, write_line  # noqa: E402

F_, D_, P_, FPS = 34, 126, 4, 15
H_ = F_ - P_


def inputs(U, W, dev, seed=3):
    from emotiongestures_amd.synth import hash_uniform, synth_inputs
    inp = synth_inputs(U * W, F_, D_, P_, seed=seed)
    r = lambda a: torch.from_numpy(a.reshape((U, W) + a.shape[1:])).to(dev)
    return {"spec": r(inp["spec"]), "text": r(inp["text"]), "seed_pose": r(inp["pre_pose"])[:, 0].contiguous(),
            "sampled": torch.from_numpy(hash_uniform("bench/sampled", (U, W, F_, 512), -1.0, 1.0, seed)).to(dev)}


def loop(model, g, alpha):
    U, W = g["spec"].shape[:2]
    track = torch.empty(U, W * H_ + P_, D_, device=g["spec"].device)
    prior = g["seed_pose"]
    for w in range(W):
        pose = model(g["spec"][:, w], g["text"][:, w], prior, g["sampled"][:, w])[0]
        if w == 0:
            track[:, :F_] = pose
        else:
            track[:, w * H_: w * H_ + P_] = (1 - alpha) * prior + alpha * pose[:, :P_]
            track[:, w * H_ + P_: w * H_ + F_] = pose[:, P_:]
        prior = pose[:, H_:].contiguous()
    return track


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x30,8x30,64x8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.builders import build_mirror
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = L.load()
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision=a.precision).to(dev)
    alpha = (torch.arange(1, P_ + 1, dtype=torch.float32, device=dev) / (P_ + 1))[None, :, None]
    res = {"metric": "rollout", "precision": a.precision, "frames": F_, "prior_frames": P_, "fps": FPS, "iters": a.iters, "rounds": a.rounds,
           "shapes": []}
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    legs = []
    for U, W in shapes:                         # capture (and thereby warm up) every shape before anything is timed
        g = inputs(U, W, dev)
        ga, oa, la = capture(lambda: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"])["track"], lib)
        gb, ob, lb = capture(lambda: loop(model, g, alpha), lib)
        for _ in range(a.warmup):
            ga.replay()
            gb.replay()
        torch.cuda.synchronize()
        legs.append((U, W, g, ga, oa, la, gb, ob, lb))
    for U, W, g, ga, oa, la, gb, ob, lb in legs:
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(window_ms(ga, a.iters))
            tb.append(window_ms(gb, a.iters))
        seconds = U * (W * H_ + P_) / FPS
        ma, mb = statistics.median(ta), statistics.median(tb)
        diff = float(((oa - ob).flatten(1).norm(dim=1) / ob.flatten(1).norm(dim=1)).max())
        res["shapes"].append({
            "U": U, "W": W, "audio_seconds": round(seconds, 2),
            "rollout_ms": round(ma, 3), "rollout_ms_min_max": [round(min(ta), 3), round(max(ta), 3)],
            "rollout_ms_per_audio_second": round(ma / seconds, 4), "rollout_launches_per_window": round(la / W, 1),
            "loop_ms": round(mb, 3), "loop_ms_min_max": [round(min(tb), 3), round(max(tb), 3)],
            "loop_ms_per_audio_second": round(mb / seconds, 4), "loop_library_launches_per_window": round(lb / W, 1),
            "speedup": round(mb / ma, 3), "track_rel_l2_rollout_vs_loop": diff, "track_bitwise": bool(torch.equal(oa, ob))})
    res["device"] = torch.cuda.get_device_name(dev)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
