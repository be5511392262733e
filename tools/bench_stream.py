#!/usr/bin/env python3
"""Streaming synthesis timing: (a) the steady-state step of a GestureStream (push -> mel -> CVAE sample -> generator -> hand-off, ONE replayed
hipGraph) against (b) a ClipPipeline(lanes=1) step at the same batch (mel -> CVAE sample -> forward as one graph: what the library offers for
one window without ring, hand-off or state), same process, TED shapes (34 frames, prior 4, 15 fps, hop 32 000 samples, window 62 976), bf16x3.
After a warm-up of every shape the two alternate, `--rounds` timed windows each of `--iters` replays between device events, every window
ending in a device synchronise; median and min/max are reported.  The stream step adds its push and hand-off launches to identical generator
work, so it is expected to equal the pipeline step: `stream_minus_pipeline_ms` is held against the pipeline step's own min-max band plus the
added kernels' durations (`--added-us`, from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_stream.py --shapes 1` run).
Reported, not gated: step time over the hop duration (real-time factor) and (c) the eager loop a user writes without the session --
harness.synthesize(windows=1) per chunk with the audio window, the prior and the cross-fade kept by torch ops (wall clock, synchronised per
step).  Launch counts are the library's own (eg_launch_count over one eager step).  Prints one JSON line.

    python tools/bench_stream.py [--shapes 1,8,64] [--iters 100] [--rounds 5] [--added-us 13,14,30] [--out profiles/stream_bench_line.json]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import window_ms, write_line  # noqa: E402

F_, D_, P_, FPS = 34, 126, 4, 15
H_ = F_ - P_
HOP, N = 32000, (124 - 1) * 512


def launches(lib, fn):
    n0 = lib.eg_launch_count()
    fn()
    torch.cuda.synchronize()
    return lib.eg_launch_count() - n0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,8,64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--added-us", default="0", help="summed duration of the stream's own kernels per step from a kernel trace: one value, or one per shape")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd.builders import build_mirror
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.engine import MelFrontEnd
    from emotiongestures_amd.pipeline import ClipPipeline
    from emotiongestures_amd.streaming import GestureStream
    from emotiongestures_amd.synth import load_synth_weights, synth_audio, synth_inputs
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = L.load()
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision=a.precision).to(dev)
    vae = load_synth_weights(MLP_Reconstruct_v3(frames=F_), 7).eval().to(dev)
    mel = MelFrontEnd(dev)
    alpha = (torch.arange(1, P_ + 1, dtype=torch.float32, device=dev) / (P_ + 1))[None, :, None]
    res = {"metric": "stream", "precision": a.precision, "frames": F_, "prior_frames": P_, "fps": FPS, "hop_samples": HOP, "n_samples": N,
           "iters": a.iters, "rounds": a.rounds, "shapes": []}
    shapes = [int(s) for s in a.shapes.split(",")]
    added = [float(v) for v in a.added_us.split(",")]
    added = dict(zip(shapes, added * len(shapes) if len(added) == 1 else added))
    legs = []
    for U in shapes:                                            # capture (and thereby warm up) every shape before anything is timed
        inp = synth_inputs(U, F_, D_, P_, seed=3)
        g = {k: torch.from_numpy(inp[k]).to(dev) for k in ("text", "pre_pose", "label", "z")}
        audio = torch.from_numpy(synth_audio(U, 4 * HOP, seed=3)).to(dev)
        sess = GestureStream((model, vae, mel), U, g["pre_pose"], hop_samples=HOP, graph=True)
        eager = GestureStream((model, vae, mel), U, g["pre_pose"], hop_samples=HOP, graph=False)
        for k in range(3):                                      # the lag, window 0 (captures), one steady step
            for s in (sess, eager):
                s.push(audio[:, k * HOP: (k + 1) * HOP].contiguous(), g["text"], g["label"], g["z"])
        stream_launches = launches(lib, lambda: eager.push(audio[:, 3 * HOP:].contiguous(), g["text"], g["label"], g["z"]))
        pipe = ClipPipeline((model, vae, mel), {"audio": audio[:, :N].contiguous(), "text": g["text"], "pre_pose": g["pre_pose"], "label": g["label"],
                                                "z": g["z"]}, dev, lanes=1)
        pipe_launches = launches(lib, lambda: pipe._step(pipe.lanes[0]))
        ra, rb = (lambda s=sess: s.replay()), (lambda p=pipe: p.lanes[0].graph.replay())

        def loop_step(state={"prior": g["pre_pose"], "ring": torch.zeros(U, 2 * HOP, device=dev), "w": 0}, audio=audio, g=g):
            """What a user writes today: audio ring, window cut, prior and cross-fade on the host side of the library."""
            state["ring"] = torch.cat([state["ring"][:, HOP:], audio[:, :HOP]], 1)
            out = Hs.synthesize((model, vae), state["ring"][:, :N].contiguous(), g["text"][:, None], state["prior"], labels=g["label"], hop_samples=HOP,
                                z=g["z"][:, None], windows=1, mel=mel)["track"]
            rows = out[:, :H_].clone()
            if state["w"] > 0:
                rows[:, :P_] = (1 - alpha) * state["prior"] + alpha * out[:, :P_]
            state["prior"], state["w"] = out[:, H_:].contiguous(), state["w"] + 1
            return rows
        loop_launches = launches(lib, loop_step)
        for _ in range(a.warmup):
            ra(); rb(); loop_step()
        torch.cuda.synchronize()
        legs.append((U, ra, rb, loop_step, stream_launches, pipe_launches, loop_launches, sess, pipe))
    for U, ra, rb, loop_step, sl, pl, ll, _sess, _pipe in legs:
        ta, tb, tc = [], [], []
        for _ in range(a.rounds):
            ta.append(window_ms(ra, a.iters))
            tb.append(window_ms(rb, a.iters))
            t0 = time.perf_counter()
            for _i in range(a.iters):
                loop_step()
                torch.cuda.synchronize()
            tc.append(1e3 * (time.perf_counter() - t0) / a.iters)
        ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
        band = (max(tb) - min(tb)) + added[U] / 1e3
        res["shapes"].append({
            "U": U, "stream_step_ms": round(ma, 4), "stream_step_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
            "pipeline_step_ms": round(mb, 4), "pipeline_step_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
            "stream_minus_pipeline_ms": round(ma - mb, 4), "added_kernels_us": added[U], "band_ms": round(band, 4), "within_band": bool(ma - mb <= band),
            "real_time_factor": round(ma / (1e3 * HOP / 16000), 6), "stream_launches_per_step": sl, "pipeline_launches_per_step": pl,
            "eager_loop_ms": round(mc, 4), "eager_loop_ms_min_max": [round(min(tc), 4), round(max(tc), 4)], "eager_loop_library_launches_per_step": ll,
            "speedup_over_eager_loop": round(mc / ma, 3)})
    res["device"] = torch.cuda.get_device_name(dev)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
