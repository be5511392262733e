#!/usr/bin/env python3
"""Skeleton output (skeleton.joints_from_tracks: eg_skeleton_joints) timed on whole tracks with the TED geometry (42 bones, 30 new poses per 2 s
window + 4) -- 8 recordings x 30 s x 8 takes, 1 x 10 min x 32 takes, 64 ragged recordings of 12-89 s x 4 takes at the native rate and resampled
15 -> 30 fps -- and on one stream step (30 poses per row) for 1, 8 and 64 rows; the data set's mean is added, as the reference's video writer
does.  One captured graph per contender, device events after warm-up, alternating rounds: every timed window is sized to at least --window-s
seconds of replays, --rounds windows per figure: median, min and max.

Beside every case:
  composition  torch on the same GPU: the reference's loop over the 42 bones (joint[child] = joint[parent] + length * vec[bone], indexed
               writes into a zero tensor), torch.lerp between gathered frames for the rate change (on the padded rectangle);
  floor        a device copy that moves the same bytes: (bytes in + bytes out) / 2 read and written;
  host         the reference's way: copy the track to the host, run the bone loop in float64 numpy (and the linear interpolation) there
               (host clock from the device tensor to the numpy result).
The project's rule against the composition: the slowest window of the kernel beats the fastest window of the composition at every shape
("rule_holds").  The ratio to the floor is reported, not gated.
Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_skeleton.py --eager-case ten_min_x32

    python tools/bench_skeleton.py [--rounds 5] [--window-s 0.4] [--out profiles/skeleton_bench_line.json]
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
H, P, FPS = 30, 4, 15


def frames_of(seconds):
    return -(-int(seconds * 16000) // 32000) * H + P


def composition(x, sk, mean, ratio):
    """x [B, T, 3K] -> [B, T_out, J, 3]: the bone loop as indexed writes, then lerp between gathered frames."""
    B, T, _D = x.shape
    v = (x + mean).view(B, T, sk.K, 3)
    p = torch.zeros(B, T, sk.J, 3, device=x.device)
    for k, (a, b, l) in enumerate(sk.dir_vec_pairs):
        p[:, :, b] = p[:, :, a] + l * v[:, :, k]
    Lf, M = ratio
    if Lf == M:
        return p
    k = torch.arange(-(-T * Lf // M), device=x.device)
    lo = torch.clamp(k * M // Lf, max=T - 2)
    f = ((k * M - lo * Lf).float() / Lf)[None, :, None, None]
    return torch.lerp(p[:, lo], p[:, lo + 1], f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--cases", default="u8_30s_x8,ten_min_x32,ragged64_x4,ragged64_x4_30fps,step_1,step_8,step_64")
    ap.add_argument("--eager-case", default=None, help="run that case eagerly --eager-iters times and exit (for a rocprofv3 kernel trace)")
    ap.add_argument("--eager-iters", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import skeleton as SK
    dev = torch.device("cuda:0")
    sk = SK.ted_expressive()
    rng = np.random.default_rng(64)
    ragged = [frames_of(s) for s in rng.uniform(12, 89, 64)]
    # name -> (frames per recording, takes, (L, M), a stream step?)
    cases = {"u8_30s_x8": ([frames_of(30)] * 8, 8, (1, 1), False), "ten_min_x32": ([frames_of(600)], 32, (1, 1), False),
             "ragged64_x4": (ragged, 4, (1, 1), False), "ragged64_x4_30fps": (ragged, 4, (2, 1), False),
             "step_1": ([H], 1, (1, 1), True), "step_8": ([H] * 8, 1, (1, 1), True), "step_64": ([H] * 64, 1, (1, 1), True)}
    mean = (torch.randn(sk.pose_dim, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)

    def make(frames, R):
        g = torch.Generator(device=dev).manual_seed(len(frames))
        x = torch.randn(len(frames) * R, max(frames), sk.pose_dim, generator=g, device=dev)
        live = torch.arange(max(frames), device=dev)[None, :] < torch.tensor(frames, device=dev).repeat_interleave(R)[:, None]
        return (x * live[:, :, None]).contiguous()

    def setup(name):
        frames, R, ratio, step = cases[name]
        x = make(frames, R)
        d_frames = torch.ones(len(frames), dtype=torch.int32, device=dev) if step else torch.tensor(frames, dtype=torch.int32, device=dev)
        unit = H if step else 1                                       # a stream step passes its 0 / 1 valid flags
        t_out = -(-x.shape[1] * ratio[0] // ratio[1])
        out = torch.empty(x.shape[0], t_out, sk.J, 3, device=dev)
        run = lambda: SK.launch_joints(x, sk, d_frames, R, unit, mean, False, ratio, out=out)
        return frames, R, ratio, x, out, run

    if a.eager_case:
        _f, _R, _r, _x, out, run = setup(a.eager_case)
        for _ in range(a.eager_iters):
            run()
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "finite": bool(torch.isfinite(out).all())}))
        return

    res = {"metric": "skeleton_joints", "unit": "device events, graphs replayed; host: wall clock from the device tensor to the numpy result",
           "rounds": a.rounds, "window_s": a.window_s, "tile_frames": SK.TILE_FRAMES, "device": torch.cuda.get_device_name(dev)}
    holds = True
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R, ratio, x, out, run = setup(name)
            g_new, _ = graph_of(run)
            g_old, y_old = graph_of(lambda: composition(x, sk, mean, ratio), warmup=2)
            n_out = [-(-n * ratio[0] // ratio[1]) for n in frames]
            nbytes = 4 * (R * sum(frames) * sk.pose_dim + out.numel())
            buf = torch.empty(max(1, nbytes // 8), dtype=torch.float32, device=dev)
            dst = torch.empty_like(buf)
            g_floor, _ = graph_of(lambda: dst.copy_(buf))
            g_new.replay()
            torch.cuda.synchronize()
            full = [u for u, n in enumerate(frames) if n == max(frames)]      # the composition works on the padded rectangle
            rows = [u * R + r for u in full for r in range(R)]
            entry = {"recordings": len(frames), "takes": R, "L": ratio[0], "M": ratio[1], "frames": [min(frames), max(frames)],
                     "frames_in": R * sum(frames), "frames_out": R * sum(n_out), "bytes": nbytes, "launches": 1,
                     "max_abs_diff_vs_composition": float((out[rows] - y_old[rows]).abs().max())}
            t, reps = alternate({"graph": g_new, "composition": g_old, "floor": g_floor}, a.rounds, a.window_s)
            for k, v in t.items():
                entry[k] = summary(v)
            sec = statistics.median(t["graph"]) * 1e-3
            entry["GBps"] = round(nbytes / sec / 1e9, 1)
            entry["ns_per_output_frame"] = round(1e9 * sec / (R * sum(n_out)), 4)
            entry["graph_over_floor"] = round(statistics.median(t["graph"]) / statistics.median(t["floor"]), 2)
            entry["composition_over_graph"] = round(statistics.median(t["composition"]) / statistics.median(t["graph"]), 2)
            entry["rule_holds"] = bool(max(t["graph"]) < min(t["composition"]))
            holds &= entry["rule_holds"]
            if not a.no_host:
                fr = None if min(frames) == max(frames) else frames
                fps = None if ratio == (1, 1) else (FPS, FPS * ratio[0] // ratio[1])
                xs = x.view(len(frames), R, x.shape[1], sk.pose_dim)
                mh = mean.cpu().numpy()
                host = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    y = SK.joints_from_tracks(xs.cpu().numpy(), sk, frames=fr, mean=mh, fps=fps)
                    host.append((time.perf_counter() - t0) * 1e3)
                y = y[0] if isinstance(y, tuple) else y
                entry["host_copy_plus_numpy"] = summary(host)
                entry["host_over_graph"] = round(statistics.median(host) / statistics.median(t["graph"]), 1)
                entry["max_abs_diff_vs_host"] = float(np.abs(out.cpu().numpy().reshape(y.shape) - y).max())
            entry["replays_per_window"] = reps["graph"]
            res[name] = entry
            del x, out, buf, dst, g_new, g_old, g_floor, y_old
            torch.cuda.empty_cache()
    res["rule_holds_everywhere"] = holds
    write_line(res, a.out)


if __name__ == "__main__":
    main()
