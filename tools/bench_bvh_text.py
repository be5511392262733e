#!/usr/bin/env python3
"""BVH text of whole takes (bvh.BvhFile.format_tracks: eg_bvh_text_measure, eg_bvh_text_write) timed on bench_euler.py's four track shapes
and 47-joint body (144 channels) -- 8 recordings x 30 s x 8 takes, 1 x 10 min x 32 takes, 64 ragged recordings of 12-89 s x 4 takes at 15 fps
and at 30 fps.  The input is the Euler channels on the device, as ``out["euler"]`` of a synthesis call holds them.  Contenders, per round and in
turn:
  host     the way without this stage: ``BvhFile.format`` of every take, each with its own device -> host copy (host clock);
  device   ``format_tracks`` on the device tensor -- table upload, buffers, measure, the copy of the sizes, write -- and one copy of the body
           to pinned host memory (host clock, synchronised at both ends);
  floor    a device copy of as many bytes as the text has (device events, a replayed graph).
Beside them, from device events: the measure launches, the write launch and the device -> pinned copy on their own, and ``copy_share``, the
copy's part of ``device``.  No time is fixed in advance: the ratios are reported as measured.

    python tools/bench_bvh_text.py [--rounds 5] [--window-s 0.4] [--out profiles/bvh_text_bench_line.json]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import graph_of, summary, window_ms, write_line  # noqa: E402
from tools.bench_articulate import synthetic_tree  # noqa: E402
from tools.bench_euler import bvh_of  # noqa: E402
from tools.bench_skeleton import FPS, frames_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--cases", default="u8_30s_x8,ten_min_x32,ragged64_x4,ragged64_x4_30fps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import bvh as BVH
    from emotiongestures_amd import skeleton as SK
    dev = torch.device("cuda:0")
    tree = synthetic_tree(SK)
    J = tree.J
    orders = [SK.ORDERS[(4 + j) % 6] if j % 5 == 0 else "ZXY" for j in range(J)]
    f = BVH.parse(bvh_of(tree, orders))
    rng = np.random.default_rng(64)
    ragged = [frames_of(s) for s in rng.uniform(12, 89, 64)]
    cases = {"u8_30s_x8": ([frames_of(30)] * 8, 8, 1), "ten_min_x32": ([frames_of(600)], 32, 1), "ragged64_x4": (ragged, 4, 1),
             "ragged64_x4_30fps": (ragged, 4, 2)}
    res = {"metric": "bvh_text", "unit": "ms; host and device: host clock, synchronised; floor, measure, write, copy: device events", "rounds": a.rounds,
           "window_s": a.window_s, "joints": J, "channels": f.channels, "tile_frames": BVH.TEXT_TILE_FRAMES, "device": torch.cuda.get_device_name(dev)}

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for name in a.cases.split(","):
        frames, R, up = cases[name]
        frames = [n * up for n in frames]
        U, T = len(frames), max(frames)
        g = torch.Generator(device=dev).manual_seed(U)
        x = (torch.rand((U, R, T, J, 3), generator=g, device=dev) * 360.0 - 180.0).contiguous()
        ft = 1.0 / (FPS * up)
        fr = None if min(frames) == max(frames) else frames
        bt = f.format_tracks(x, fr, frame_time=ft)
        total = int(bt.offsets[-1])
        pinned = torch.empty(total, dtype=torch.uint8).pin_memory()
        assert bt.text(U - 1, R - 1) == f.format(x[U - 1, R - 1, :frames[-1]], frame_time=ft)

        def host():
            return sum(len(f.format(x[u, r, :n], frame_time=ft)) for u, n in enumerate(frames) for r in range(R))

        def device():
            pinned.copy_(f.format_tracks(x, fr, frame_time=ft).body)
            return total
        k = BVH.TextKernels(f.text_table(), x.view(U * R, T, J, 3), fr, None if fr is None else torch.tensor(fr, dtype=torch.int32, device=dev), R)
        text = torch.empty(total, dtype=torch.uint8, device=dev)
        src = torch.empty(total, dtype=torch.uint8, device=dev)
        graphs = {"floor": graph_of(lambda: text.copy_(src))[0], "measure": graph_of(k.measure)[0], "write": graph_of(lambda: k.write(text))[0]}
        reps = {n: max(5, int(a.window_s * 1000.0 / max(window_ms(gr, 3), 1e-3)) + 1) for n, gr in graphs.items()}
        t = {n: [] for n in ("host", "device", "floor", "measure", "write", "copy")}
        device()                                                                       # warm-up
        for _ in range(a.rounds):
            ms, chars = clock(host)
            t["host"].append(ms)
            t["device"].append(statistics.median(clock(device)[0] for _ in range(3)))
            for n, gr in graphs.items():
                t[n].append(window_ms(gr, reps[n]))
            t["copy"].append(window_ms(lambda: pinned.copy_(text, non_blocking=True), 5))
        med = {n: statistics.median(v) for n, v in t.items()}
        entry = {"recordings": U, "takes": R, "fps": FPS * up, "frames": [min(frames), max(frames)], "frames_out": R * sum(frames), "bytes": total,
                 "characters_host": chars, "launches": {"measure": 3, "write": 1}}
        assert chars == total + sum(len(bt.head(u, r)) for u in range(U) for r in range(R))
        for n, v in t.items():
            entry[n] = summary(v)
        entry["host_over_device"] = round(med["host"] / med["device"], 1)
        entry["device_over_floor"] = round(med["device"] / med["floor"], 1)
        entry["kernels_over_floor"] = round((med["measure"] + med["write"]) / med["floor"], 1)
        entry["copy_share"] = round(med["copy"] / med["device"], 2)
        entry["write_GBps"] = round(total / (med["write"] * 1e-3) / 1e9, 1)
        entry["copy_GBps"] = round(total / (med["copy"] * 1e-3) / 1e9, 1)
        entry["device_ahead"] = bool(max(t["device"]) < min(t["host"]))
        res[name] = entry
        del x, bt, k, text, src, graphs, pinned
        torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
