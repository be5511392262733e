#!/usr/bin/env python3
"""The delayed output stage of a stream (GestureStream(render=): render.StreamRender) timed inside the steady-state step of a session: one
replayed hipGraph per contender, the contenders of a shape alternating, `--rounds` timed windows each of `--iters` replays between device events;
the median is reported with min and max.

Per shape four sessions on the same generator, audio and rows:
  plain    no output stage
  raw      the existing stage on the rows just emitted: joints= and rotations= (TED), joints=tree, rotations=True, euler= (BEAT)
  smooth   smooth=(9, 3) alone: the smoother's two launches
  render   render=(the raw stage's outputs, smooth=(9, 3), fps=(15, 30)): the smoother's two launches, the delay line's two, the output
           launches on a window of H + 1 frames that make 2 H output frames
The figure is the time the stage adds to a push, render - plain, held against what its parts add in the same run, (raw - plain) +
(smooth - plain): `added_over_parts`.  The stage makes twice the output frames of the raw stage and two launches more, so a ratio above 1 is
expected; nothing is gated.  TED shapes (34 frames, prior 4, 126 columns) at 1 / 8 / 64 rows and the BEAT shape (60 frames, prior 10, 282
columns, a 47-joint tree) at 8 rows.  Launch counts are the library's own over one eager step.  Prints one JSON line.

    python tools/bench_stream_render.py [--shapes 1,8,64] [--beat-rows 8] [--iters 100] [--rounds 5] [--out profiles/stream_render_bench_line.json]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import window_ms, write_line  # noqa: E402
from tools.bench_articulate import synthetic_tree  # noqa: E402

FPS, RENDER_FPS, FILTER = 15, 30, (9, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,8,64")
    ap.add_argument("--beat-rows", type=int, default=8)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd import skeleton as SK
    from emotiongestures_amd.builders import build_mirror
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.engine import MelFrontEnd
    from emotiongestures_amd.streaming import GestureStream
    from emotiongestures_amd.synth import load_synth_weights, synth_audio, synth_inputs
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_render.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = L.load()
    mel = MelFrontEnd(dev)
    ted = SK.ted_expressive()
    rest = np.random.default_rng(5).standard_normal((ted.K, 3))
    tree = synthetic_tree(SK)
    bodies = {"ted": dict(geom=(34, 126, 4), hop=32000, raw=dict(joints=ted, rotations=rest), render=dict(joints=ted, rotations=rest)),
              "beat": dict(geom=(60, 282, 10), hop=53333, raw=dict(joints=tree, rotations=True, euler="ZXY"),
                           render=dict(joints=tree, rotations=True, euler="ZXY"))}
    res = {"metric": "stream_render", "unit": "ms per steady-state push, device events, one graph replayed", "fps": [FPS, RENDER_FPS], "filter": list(FILTER),
           "iters": a.iters, "rounds": a.rounds, "shapes": []}
    cases = [("ted", int(u)) for u in a.shapes.split(",")] + [("beat", a.beat_rows)]
    legs = []
    for name, U in cases:                                       # open, warm up and capture every session before anything is timed
        b = bodies[name]
        F_, D_, P_ = b["geom"]
        hop = b["hop"]
        if "model" not in b:
            b["model"] = build_mirror("spatial", F_, D_, P_, P_, seed=7, precision="bf16x3").to(dev)
            b["vae"] = load_synth_weights(MLP_Reconstruct_v3(frames=F_), 7).eval().to(dev)
        model, vae = b["model"], b["vae"]
        inp = synth_inputs(U, F_, D_, P_, seed=3)
        g = {k: torch.from_numpy(inp[k]).to(dev) for k in ("text", "pre_pose", "label", "z")}
        audio = torch.from_numpy(synth_audio(U, 4 * hop, seed=3)).to(dev)
        kinds = {"plain": {}, "raw": b["raw"], "smooth": dict(smooth=FILTER), "render": dict(render=dict(b["render"], smooth=FILTER, fps=(FPS, RENDER_FPS)))}
        sess, counts = {}, {}
        for kind, kw in kinds.items():
            s = GestureStream((model, vae, mel), U, g["pre_pose"], hop_samples=hop, graph=True, **kw)
            e = GestureStream((model, vae, mel), U, g["pre_pose"], hop_samples=hop, graph=False, **kw)
            for k in range(3):                                  # the lag, window 0 (captures), one steady step
                for t in (s, e):
                    t.push(audio[:, k * hop:(k + 1) * hop].contiguous(), g["text"], g["label"], g["z"])
            n0 = lib.eg_launch_count()
            e.push(audio[:, 3 * hop:].contiguous(), g["text"], g["label"], g["z"])
            torch.cuda.synchronize()
            counts[kind] = lib.eg_launch_count() - n0
            sess[kind] = s
            for _ in range(3):
                s.replay()
        torch.cuda.synchronize()
        legs.append((name, U, sess, counts))
    for name, U, sess, counts in legs:
        t = {k: [] for k in sess}
        for _ in range(a.rounds):
            for k, s in sess.items():
                t[k].append(window_ms(s.replay, a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        parts = (med["raw"] - med["plain"]) + (med["smooth"] - med["plain"])
        added = med["render"] - med["plain"]
        rd = sess["render"]
        res["shapes"].append(dict(
            body=name, U=U, render_delay_frames=rd.render_delay, render_delay_ms=round(1e3 * rd.render_delay / FPS, 1), render_frames=rd.render_frames,
            **{f"{k}_step_ms": round(med[k], 4) for k in med}, **{f"{k}_step_ms_min_max": [round(min(t[k]), 4), round(max(t[k]), 4)] for k in t},
            launches_per_step=counts, added_by_render_ms=round(added, 4), added_by_raw_ms=round(med["raw"] - med["plain"], 4),
            added_by_smooth_ms=round(med["smooth"] - med["plain"], 4), added_over_parts=round(added / parts, 3) if parts > 0 else None,
            plain_band_ms=round(max(t["plain"]) - min(t["plain"]), 4)))
    res["device"] = torch.cuda.get_device_name(dev)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
