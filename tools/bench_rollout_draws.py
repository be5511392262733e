#!/usr/bin/env python3
"""Diverse roll-out timing: (a) Transformer.synthesize(draws=R) (eg_generator_forward_rollout_draws: the audio tower once per window, fusion /
encoder / K|V per (window, draw), W decoder steps at batch U*R) against (b) what the library offered before it for the same result:
synthesize on the recordings replicated R times (U*R recordings, the tower R times per window).  Both are captured as ONE hipGraph each and
replayed; TED shapes (34 frames, prior 4, 15 fps), bf16x3.  After a warm-up of every shape the two alternate, `--rounds` timed windows each
of `--iters` replays between device events, every window ending in a device synchronise; the median window is reported.  Launch counts are
the library's own (eg_launch_count while the graph is captured).  Prints one JSON line.  Kernel statistics: run one shape under
`rocprofv3 --kernel-trace --stats -- python tools/bench_rollout_draws.py --shapes 1x30x32` separately.

    python tools/bench_rollout_draws.py [--shapes 1x30x8,8x8x8,8x30x4,1x30x32] [--iters 5] [--rounds 5] [--out profiles/rollout_draws_bench_line.json]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import capture, window_ms, write_line  # noqa: E402

F_, D_, P_, FPS = 34, 126, 4, 15
H_ = F_ - P_


def inputs(U, W, R, dev, seed=3):
    from emotiongestures_amd.synth import hash_uniform, synth_inputs
    inp = synth_inputs(U * W, F_, D_, P_, seed=seed)
    r = lambda a: torch.from_numpy(a.reshape((U, W) + a.shape[1:])).to(dev)
    return {"spec": r(inp["spec"]), "text": r(inp["text"]), "seed_pose": r(inp["pre_pose"])[:, 0].contiguous(),
            "sampled": torch.from_numpy(hash_uniform("bench/sampled_draws", (U, R, W, F_, 512), -1.0, 1.0, seed)).to(dev)}


def replicate(g):
    U, R = g["sampled"].shape[:2]
    rep = lambda x: x[:, None].expand((U, R) + tuple(x.shape[1:])).reshape((U * R,) + tuple(x.shape[1:])).contiguous()
    return {"spec": rep(g["spec"]), "text": rep(g["text"]), "seed_pose": rep(g["seed_pose"]),
            "sampled": g["sampled"].reshape((U * R,) + tuple(g["sampled"].shape[2:]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x30x8,8x8x8,8x30x4,1x30x32", help="UxWxR, comma separated")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.builders import build_mirror
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_draws.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = L.load()
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision=a.precision).to(dev)
    eng = model.engine()
    res = {"metric": "rollout_draws", "precision": a.precision, "frames": F_, "prior_frames": P_, "fps": FPS, "iters": a.iters,
           "rounds": a.rounds, "shapes": []}
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    legs = []
    for U, W, R in shapes:                      # capture (and thereby warm up) every shape before anything is timed
        g = inputs(U, W, R, dev)
        h = replicate(g)
        ga, oa, la = capture(lambda: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=R)["track"], lib)
        gb, ob, lb = capture(lambda: model.synthesize(h["spec"], h["text"], h["seed_pose"], h["sampled"])["track"], lib)
        for _ in range(a.warmup):
            ga.replay()
            gb.replay()
        torch.cuda.synchronize()
        legs.append((U, W, R, g, h, ga, oa, la, gb, ob, lb))
    for U, W, R, g, h, ga, oa, la, gb, ob, lb in legs:
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(window_ms(ga, a.iters))
            tb.append(window_ms(gb, a.iters))
        seconds = U * R * (W * H_ + P_) / FPS
        ma, mb = statistics.median(ta), statistics.median(tb)
        ob = ob.view(oa.shape)
        res["shapes"].append({
            "U": U, "W": W, "R": R, "track_seconds": round(seconds, 2),
            "draws_ms": round(ma, 3), "draws_ms_min_max": [round(min(ta), 3), round(max(ta), 3)],
            "draws_ms_per_track_second": round(ma / seconds, 4), "draws_launches": la,
            "draws_workspace_bytes": int(lib.eg_generator_rollout_draws_workspace_bytes(eng._h, U, W, R)),
            "replicated_ms": round(mb, 3), "replicated_ms_min_max": [round(min(tb), 3), round(max(tb), 3)],
            "replicated_ms_per_track_second": round(mb / seconds, 4), "replicated_launches": lb,
            "replicated_workspace_bytes": int(lib.eg_generator_rollout_workspace_bytes(eng._h, U * R, W)),
            "speedup": round(mb / ma, 3), "flop_estimate_ratio": round((7.75 + 1.5 * R) / (9.25 * R), 3),
            "track_bitwise": bool(torch.equal(oa, ob))})
    res["device"] = torch.cuda.get_device_name(dev)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
