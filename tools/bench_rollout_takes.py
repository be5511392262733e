#!/usr/bin/env python3
"""Takes roll-out timing: Transformer.synthesize_takes (eg_generator_forward_rollout_takes: R sampled tracks for recordings of unequal
length, the audio tower once per window) against what the library offered before it for the same tracks:
  (a) replicated: the ragged synthesize(windows_per=) on the recordings repeated R times -- the definition;
  (b) per_length: one rectangular synthesize(draws=R) per distinct window count, all of them in one graph (the sum);
  (c) padded:     one rectangular synthesize(draws=R) with every recording padded to the longest (tracks past a recording's end are waste).
Every contender is captured as ONE hipGraph and replayed; TED shapes (34 frames, prior 4, 15 fps), bf16x3.  After a warm-up of every shape the
contenders alternate, `--rounds` timed windows each of `--iters` replays between device events, every window ending in a device
synchronise; the median window and the spread (min, max) are reported.  Launch counts are the library's own (eg_launch_count while the graph
is captured).  Prints one JSON line.

    python tools/bench_rollout_takes.py [--shapes 64:4-30x4,8:8-30x8] [--iters 3] [--rounds 5] [--out profiles/rollout_takes_bench_line.json]

A shape is U:Wmin-WmaxxR: U recordings with window counts spread over [Wmin, Wmax] (a fixed stride walk, the same vector every run), R takes.
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


def window_counts(U, lo, hi):
    """U counts spread over [lo, hi]: a walk by a stride coprime to the span, so every run times the same vector."""
    span = hi - lo + 1
    stride = next(s for s in (37, 19, 11, 7, 5, 3, 2, 1) if np.gcd(s, span) == 1)
    return tuple(lo + (u * stride) % span for u in range(U))


def inputs(wp, R, dev, seed=3):
    """Padded [U, Wmax, ...] inputs with sampled [U, R, Wmax, F, 512] on the device."""
    from emotiongestures_amd.synth import hash_uniform, synth_inputs
    U, Wmax = len(wp), max(wp)
    inp = synth_inputs(U * Wmax, F_, D_, P_, seed=seed)
    r = lambda a: torch.from_numpy(a.reshape((U, Wmax) + a.shape[1:])).to(dev)
    return {"spec": r(inp["spec"]), "text": r(inp["text"]), "seed_pose": r(inp["pre_pose"])[:, 0].contiguous(),
            "sampled": torch.from_numpy(hash_uniform("bench/sampled_takes", (U, R, Wmax, F_, 512), -1.0, 1.0, seed)).to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64:4-30x4,8:8-30x8", help="U:Wmin-WmaxxR, comma separated")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.builders import build_mirror
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_takes.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = L.load()
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision=a.precision).to(dev)
    eng = model.engine()
    res = {"metric": "rollout_takes", "precision": a.precision, "frames": F_, "prior_frames": P_, "fps": FPS, "iters": a.iters,
           "rounds": a.rounds, "shapes": []}
    legs = []
    for shape in a.shapes.split(","):           # capture (and thereby warm up) every shape before anything is timed
        head, R = shape.split("x")
        U, span = head.split(":")
        lo, hi = span.split("-")
        U, R, lo, hi = int(U), int(R), int(lo), int(hi)
        wp = window_counts(U, lo, hi)
        N, Wmax = sum(wp), max(wp)
        g = inputs(wp, R, dev)
        with torch.no_grad():                   # packed once, outside the graphs: every contender gets its inputs in the form it takes
            spec, text = eng.pack_ragged(g["spec"], wp, "spec"), eng.pack_ragged(g["text"], wp, "text")
            wpr = tuple(w for w in wp for _ in range(R))
            sampled = eng.pack_ragged(g["sampled"].reshape((U * R, Wmax) + tuple(g["sampled"].shape[3:])), wpr, "sampled")
            rep = lambda x: x[:, None].expand((U, R) + tuple(x.shape[1:])).reshape((U * R,) + tuple(x.shape[1:])).contiguous()
            rspec, rtext = eng.pack_ragged(rep(g["spec"]), wpr, "spec"), eng.pack_ragged(rep(g["text"]), wpr, "text")
            rseed = rep(g["seed_pose"])
            groups = []
            for W in sorted(set(wp)):
                idx = torch.as_tensor([u for u in range(U) if wp[u] == W], device=dev)
                groups.append((W, g["spec"][idx][:, :W].contiguous(), g["text"][idx][:, :W].contiguous(), g["seed_pose"][idx].contiguous(),
                               g["sampled"][idx][:, :, :W].contiguous()))
        takes = lambda: model.synthesize_takes(spec, text, g["seed_pose"], sampled, windows_per=wp, draws=R)["track"]
        replicated = lambda: model.synthesize(rspec, rtext, rseed, sampled, windows_per=wpr)["track"]
        per_length = lambda: [model.synthesize(s, t, p, e, draws=R)["track"] for _W, s, t, p, e in groups]
        padded = lambda: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=R)["track"]
        graphs, outs, launches = {}, {}, {}
        for name, fn in (("takes", takes), ("replicated", replicated), ("per_length", per_length), ("padded", padded)):
            graphs[name], outs[name], launches[name] = capture(fn, lib)
            for _ in range(a.warmup):
                graphs[name].replay()
        torch.cuda.synchronize()
        ws = {"takes": int(lib.eg_generator_rollout_takes_workspace_bytes(eng._h, U, N, R)),
              "replicated": int(lib.eg_generator_rollout_ragged_workspace_bytes(eng._h, U * R, N * R)),
              "per_length": max(int(lib.eg_generator_rollout_draws_workspace_bytes(eng._h, int(s.shape[0]), W, R)) for W, s, *_ in groups),
              "padded": int(lib.eg_generator_rollout_draws_workspace_bytes(eng._h, U, Wmax, R))}
        keep = (g, spec, text, sampled, rspec, rtext, rseed, groups)       # the graphs read these buffers at every replay
        legs.append((U, R, wp, graphs, outs, launches, ws, len(groups), keep))
    for U, R, wp, graphs, outs, launches, ws, n_groups, _keep in legs:
        N, Wmax = sum(wp), max(wp)
        t = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, gr in graphs.items():
                t[k].append(window_ms(gr, a.iters))
        seconds = R * sum(w * H_ + P_ for w in wp) / FPS
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"U": U, "R": R, "windows_min": min(wp), "windows_max": Wmax, "total_windows": N, "distinct_lengths": n_groups,
               "track_seconds": round(seconds, 2)}
        for k in graphs:
            row[k + "_ms"] = round(med[k], 3)
            row[k + "_ms_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
            row[k + "_launches"] = launches[k]
            row[k + "_workspace_bytes"] = ws[k]
        row["takes_ms_per_track_second"] = round(med["takes"] / seconds, 4)
        for k in ("replicated", "per_length", "padded"):
            row["speedup_vs_" + k] = round(med[k] / med["takes"], 3)
        # per window: tower side 7.75, per (window, draw) 1.5 (the estimate profiles/rollout_draws_bench_line.json uses)
        row["flop_estimate_ratio_vs_replicated"] = round((7.75 + 1.5 * R) / (9.25 * R), 3)
        row["flop_estimate_ratio_vs_padded"] = round(N / (U * Wmax), 3)
        row["track_bitwise_vs_replicated"] = bool(torch.equal(outs["takes"], outs["replicated"].view(outs["takes"].shape)))
        res["shapes"].append(row)
    res["device"] = torch.cuda.get_device_name(dev)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
