#!/usr/bin/env python3
"""Motion statistics (kinematics.launch_kinematics: eg_kin_stats) timed on the joints of whole tracks with the TED geometry (43 joints, 30 new
poses per 2 s window + 4) -- bench_skeleton.py's four shapes: 8 recordings x 30 s x 8 takes, 1 x 10 min x 32 takes, 64 ragged recordings of
12-89 s x 4 takes at the native rate and at 15 -> 30 fps (twice the frames).  The joints are random walks (steps of about 1 cm), the bins the
default 40.  One captured graph per contender, device events after warm-up, alternating rounds: every timed window is sized to at least
--window-s seconds of replays, --rounds windows per figure: median, min and max.

Beside every case:
  composition  the same definition from torch ops on the same GPU, on the padded rectangle with masks: diff three times, square and sum in
               float64, sqrt, masked mean, bucketize + scatter_add for the histogram;
  floor        a device copy that moves the same bytes: (bytes in + bytes out) / 2 read and written;
  host         copy the joints to the host and run the numpy definition there (kinematics_of_joints on an array; host clock from the device
               tensor to the numpy result).
The expectation the result is held against: the kernel reads the joints once and writes almost nothing, the composition makes at least six
passes, so the kernel should sit within a small multiple of the floor and ahead of the composition at every shape ("rule_holds": the slowest
window of the kernel beats the fastest window of the composition).  Whatever is measured is written down.
Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_kinematics.py --eager-case ten_min_x32

    python tools/bench_kinematics.py [--rounds 5] [--window-s 0.4] [--out profiles/kinematics_bench_line.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import alternate, graph_of, summary, write_line  # noqa: E402
H, P, FPS, J = 30, 4, 15, 43


def frames_of(seconds):
    return -(-int(seconds * 16000) // 32000) * H + P


def composition(x, n, edges2, fps):
    """x [rows, T, J, 3] fp32, n [rows] int64 valid frames -> (mean [rows, 3, J] float64, hist [rows, J, E] int32), on the padded rectangle."""
    rows, T, Jn, _ = x.shape
    E = edges2.numel()
    d, means, hist = x, [], None
    for k in (1, 2, 3):
        d = torch.diff(d, dim=1)
        s2 = d.double().square().sum(-1)                                                   # [rows, T - k, J]
        valid = torch.arange(T - k, device=x.device)[None, :, None] < (n - k)[:, None, None]
        means.append(torch.where(valid, s2.sqrt(), 0.0).sum(1) * float(fps) ** k / (n - k)[:, None])
        if k == 1:
            pos = (torch.bucketize(s2, edges2, right=True) - 1).transpose(1, 2)            # [rows, J, T - 1]
            hist = torch.zeros(rows, Jn, E, dtype=torch.int32, device=x.device)
            hist.scatter_add_(2, pos, valid.transpose(1, 2).expand(rows, Jn, T - 1).to(torch.int32))
    return torch.stack(means, 1), hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--cases", default="u8_30s_x8,ten_min_x32,ragged64_x4,ragged64_x4_30fps")
    ap.add_argument("--eager-case", default=None, help="run that case eagerly --eager-iters times and exit (for a rocprofv3 kernel trace)")
    ap.add_argument("--eager-iters", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import kinematics as KM
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(64)
    ragged = [frames_of(s) for s in rng.uniform(12, 89, 64)]
    # name -> (frames per recording, takes, output frames per source frame)
    cases = {"u8_30s_x8": ([frames_of(30)] * 8, 8, 1), "ten_min_x32": ([frames_of(600)], 32, 1), "ragged64_x4": (ragged, 4, 1),
             "ragged64_x4_30fps": (ragged, 4, 2)}
    res = {"metric": "kinematics_stats", "unit": "device events, graphs replayed; host: wall clock from the device tensor to the numpy result",
           "rounds": a.rounds, "window_s": a.window_s, "tile_frames": KM.TILE_FRAMES, "joints": J, "bins": 40,
           "device": torch.cuda.get_device_name(dev)}
    holds = True
    with torch.no_grad():
        for name in [a.eager_case] if a.eager_case else a.cases.split(","):
            frames, R, up = cases[name]
            frames = [n * up for n in frames]
            fps = FPS * up
            rows, T = len(frames) * R, max(frames)
            g = torch.Generator(device=dev).manual_seed(len(frames))
            x = torch.cumsum(torch.randn(rows, T, J, 3, generator=g, device=dev) * (0.01 / up), 1)
            n_rows = torch.tensor(frames, device=dev).repeat_interleave(R)
            x = (x * (torch.arange(T, device=dev)[None, :] < n_rows[:, None])[:, :, None, None]).contiguous()
            bins = KM.SpeedBins(fps=fps)
            d_frames = torch.tensor(frames, dtype=torch.int32, device=dev)
            ws = torch.empty(int(KM.L.load().eg_kin_workspace_bytes(rows, T, J, bins.bins)), dtype=torch.uint8, device=dev)
            out = (torch.empty(rows, 3, J, dtype=torch.float64, device=dev), torch.empty(rows, J, bins.bins + 1, dtype=torch.int32, device=dev))
            table = bins.table(dev)
            if a.eager_case:
                for _ in range(a.eager_iters):
                    KM.launch_kinematics(x, bins, frames, d_frames, R, workspace=ws, out=out)
                torch.cuda.synchronize()
                print(json.dumps({"eager_case": name, "iters": a.eager_iters, "finite": bool(torch.isfinite(out[0]).all())}))
                return
            g_new, _ = graph_of(lambda: KM.launch_kinematics(x, bins, frames, d_frames, R, workspace=ws, out=out))
            g_old, y_old = graph_of(lambda: composition(x, n_rows, table, fps), warmup=2)
            nbytes = 4 * R * sum(frames) * J * 3 + 8 * out[0].numel() + 4 * out[1].numel()
            buf = torch.empty(max(1, nbytes // 8), dtype=torch.float32, device=dev)
            dst = torch.empty_like(buf)
            g_floor, _ = graph_of(lambda: dst.copy_(buf))
            g_new.replay()
            torch.cuda.synchronize()
            entry = {"recordings": len(frames), "takes": R, "fps": fps, "frames": [min(frames), max(frames)], "frames_in": R * sum(frames),
                     "bytes": nbytes, "workspace_bytes": ws.numel(), "launches": 3,
                     "hist_equals_composition": bool(torch.equal(out[1], y_old[1])),
                     "max_rel_diff_of_means_vs_composition": float(((out[0] - y_old[0]).abs() / y_old[0].abs().clamp_min(1e-300)).max())}
            t, reps = alternate({"graph": g_new, "composition": g_old, "floor": g_floor}, a.rounds, a.window_s)
            for k, v in t.items():
                entry[k] = summary(v)
            sec = statistics.median(t["graph"]) * 1e-3
            entry["GBps"] = round(nbytes / sec / 1e9, 1)
            entry["graph_over_floor"] = round(statistics.median(t["graph"]) / statistics.median(t["floor"]), 2)
            entry["composition_over_graph"] = round(statistics.median(t["composition"]) / statistics.median(t["graph"]), 2)
            entry["rule_holds"] = bool(max(t["graph"]) < min(t["composition"]))
            holds &= entry["rule_holds"]
            if not a.no_host:
                xs = x.view(len(frames), R, T, J, 3)
                host = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    y = KM.kinematics_of_joints(xs.cpu().numpy(), fps, frames=frames)
                    host.append((time.perf_counter() - t0) * 1e3)
                entry["host_copy_plus_numpy"] = summary(host)
                entry["host_over_graph"] = round(statistics.median(host) / statistics.median(t["graph"]), 1)
                full = np.concatenate([y["speed_hist"], y["speed_over"][..., None]], -1).reshape(rows, J, -1)
                entry["hist_equals_host"] = bool(np.array_equal(out[1].cpu().numpy(), full))
            entry["replays_per_window"] = reps["graph"]
            res[name] = entry
            del x, out, buf, dst, ws, g_new, g_old, g_floor, y_old
            torch.cuda.empty_cache()
    res["rule_holds_everywhere"] = holds
    write_line(res, a.out)


if __name__ == "__main__":
    main()
