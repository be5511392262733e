#!/usr/bin/env python3
"""Ragged roll-out timing: U recordings with their own window counts W_u synthesised by (r) ONE ragged call (Transformer.synthesize with
windows_per: phase A at batch N = sum W_u, Wmax steps at the shrinking batch U_s) against the two things a user could do before it:
(a) the rectangular roll-out on inputs padded to Wmax (phase A at batch U*Wmax, every step at batch U; the padded windows are wasted work),
(b) one rectangular roll-out per distinct length (small batches, one workspace per length).  Every contender is captured as ONE hipGraph and
replayed; TED shapes (34 frames, prior 4, 15 fps), bf16x3.  After a warm-up of everything the contenders alternate, `--rounds` timed windows
each of `--iters` replays between device events, every window ending in a device synchronise; the median window is reported.  Launch counts
are the library's own (eg_launch_count while the graph is captured).  The length vectors are fixed functions of synth.hash_unit:
  spread:   U = 32, W_u spread over 1 .. 30            one_long: U = 8, one recording of 30 windows among recordings of 1 .. 3
Prints one JSON line.

    python tools/bench_rollout_ragged.py [--cases spread,one_long] [--iters 10] [--rounds 5] [--out profiles/rollout_ragged_bench_line.json]
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

from tools.bench_rollout import F_, D_, P_, FPS, H_, capture, window_ms  # noqa: E402


def vectors():
    from emotiongestures_amd.synth import hash_unit
    spread = [1 + int(v * 30) for v in hash_unit("bench/ragged/spread", 32, 3)]
    spread[0], spread[1] = 30, 1                                   # both ends of the range are present whatever the hash gives
    short = [1 + int(v * 3) for v in hash_unit("bench/ragged/short", 8, 3)]
    short[5] = 30
    return {"spread": [min(30, w) for w in spread], "one_long": [min(30, w) for w in short]}


def inputs(wp, dev, seed=3):
    """Padded [U, Wmax, ...] inputs and their packed [N, ...] form."""
    from emotiongestures_amd.synth import hash_uniform, synth_inputs
    U, Wmax = len(wp), max(wp)
    inp = synth_inputs(U * Wmax, F_, D_, P_, seed=seed)
    r = lambda a: torch.from_numpy(a.reshape((U, Wmax) + a.shape[1:])).to(dev)
    pad = {"spec": r(inp["spec"]), "text": r(inp["text"]),
           "sampled": torch.from_numpy(hash_uniform("bench/sampled", (U, Wmax, F_, 512), -1.0, 1.0, seed)).to(dev)}
    packed = {k: torch.cat([v[u, :w] for u, w in enumerate(wp)]).contiguous() for k, v in pad.items()}
    return pad, packed, r(inp["pre_pose"])[:, 0].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="spread,one_long")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.builders import build_mirror
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_ragged.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = L.load()
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision=a.precision).to(dev)
    res = {"metric": "rollout_ragged", "precision": a.precision, "frames": F_, "prior_frames": P_, "fps": FPS, "iters": a.iters,
           "rounds": a.rounds, "cases": []}
    all_vectors = vectors()
    legs = []
    for name in a.cases.split(","):             # capture (and thereby warm up) every contender before anything is timed
        wp = all_vectors[name]
        pad, packed, seed_pose = inputs(wp, dev)
        groups = {}                              # (b): recordings grouped by window count, one rectangular call per group
        for u, w in enumerate(wp):
            groups.setdefault(w, []).append(u)
        grouped = [(w, pad["spec"][us, :w].contiguous(), pad["text"][us, :w].contiguous(), seed_pose[us].contiguous(),
                    pad["sampled"][us, :w].contiguous()) for w, us in sorted(groups.items())]
        gr, o_r, lr = capture(lambda: model.synthesize(packed["spec"], packed["text"], seed_pose, packed["sampled"], windows_per=wp)["track"], lib)
        ga, o_a, la = capture(lambda: model.synthesize(pad["spec"], pad["text"], seed_pose, pad["sampled"])["track"], lib)
        gb, o_b, lb = capture(lambda: [model.synthesize(s, t, p, e)["track"] for _w, s, t, p, e in grouped], lib)
        for _ in range(a.warmup):
            for g in (gr, ga, gb):
                g.replay()
        torch.cuda.synchronize()
        # the graphs read the inputs where they lie: keep them alive (the next case's capture empties the allocator's cache)
        legs.append((name, wp, groups, (gr, o_r, lr), (ga, o_a, la), (gb, o_b, lb), (pad, packed, seed_pose, grouped)))
    for name, wp, groups, (gr, o_r, lr), (ga, o_a, la), (gb, o_b, lb), _inputs in legs:
        tr, ta, tb = [], [], []
        for _ in range(a.rounds):
            tr.append(window_ms(gr, a.iters))
            ta.append(window_ms(ga, a.iters))
            tb.append(window_ms(gb, a.iters))
        U, N, Wmax = len(wp), sum(wp), max(wp)
        mr, ma, mb = statistics.median(tr), statistics.median(ta), statistics.median(tb)
        # the three agree on every real row: (a)'s rows of recording u up to its own end, (b)'s group tracks
        same_a = all(torch.equal(o_r[u, : w * H_ + P_], o_a[u, : w * H_ + P_]) for u, w in enumerate(wp))
        same_b = all(torch.equal(o_r[us, : w * H_ + P_], o_b[i]) for i, (w, us) in enumerate(sorted(groups.items())))
        seconds = sum(w * H_ + P_ for w in wp) / FPS
        res["cases"].append({
            "case": name, "windows_per": wp, "U": U, "N": N, "Wmax": Wmax, "fill": round(N / (U * Wmax), 3), "distinct_lengths": len(groups),
            "audio_seconds": round(seconds, 2),
            "ragged_ms": round(mr, 3), "ragged_ms_min_max": [round(min(tr), 3), round(max(tr), 3)], "ragged_launches": lr,
            "padded_ms": round(ma, 3), "padded_ms_min_max": [round(min(ta), 3), round(max(ta), 3)], "padded_launches": la,
            "per_length_ms": round(mb, 3), "per_length_ms_min_max": [round(min(tb), 3), round(max(tb), 3)], "per_length_launches": lb,
            "speedup_vs_padded": round(ma / mr, 3), "speedup_vs_per_length": round(mb / mr, 3),
            "tracks_bitwise_vs_padded": bool(same_a), "tracks_bitwise_vs_per_length": bool(same_b)})
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
