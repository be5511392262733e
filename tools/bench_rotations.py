#!/usr/bin/env python3
"""Rotation output (skeleton.rotations_from_tracks: eg_skeleton_rotations) timed on bench_skeleton.py's shapes with the TED geometry (42 bones)
-- 8 recordings x 30 s x 8 takes, 1 x 10 min x 32 takes, 64 ragged recordings of 12-89 s x 4 takes at the native rate and resampled 15 -> 30 fps
-- and on one stream step (30 poses per row) for 1, 8 and 64 rows; local rotations against a random rest pose, bone vectors scattered around it, the
data set's mean added.  One captured graph per contender, device events after warm-up, alternating rounds (tools/_timing.py).

Beside every case:
  composition  the same definition from torch ops on the same GPU: a loop over the 42 bones of batched quaternion products (torch.lerp between
               gathered frames of the vectors for the rate change, on the padded rectangle);
  floor        a device copy that moves the same bytes: (bytes in + bytes out) / 2 read and written;
  host         copy the track to the host and run the float64 numpy definition there (host clock from the device tensor to the numpy result).
No time is fixed in advance: the ratios are reported.
Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_rotations.py --eager-case ten_min_x32

    python tools/bench_rotations.py [--rounds 5] [--window-s 0.4] [--out profiles/rotations_bench_line.json]
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
from tools.bench_skeleton import FPS, H, frames_of  # noqa: E402


def qmul(p, q):
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                        pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)


def qrot(q, v):
    u, w = q[..., 1:], q[..., :1]
    t = 2.0 * torch.linalg.cross(u, v)
    return v + w * t + torch.linalg.cross(u, t)


def arc(a, b, half):
    """a [3] unit, b [..., 3] -> [..., 4]; `half` [4]: the half turn of a."""
    c = (b * a).sum(-1, keepdim=True)
    q = torch.cat([1.0 + c, torch.linalg.cross(a.expand_as(b), b)], -1)
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    return torch.where(c >= -1.0 + 1e-6, q, half)


def composition(x, pb, rest, halves, conj, mean, ratio):
    """x [B, T, 3K] -> local rotations [B, T_out, K, 4] from torch ops."""
    B, T, _D = x.shape
    K = len(pb)
    v = (x + mean).view(B, T, K, 3)
    Lf, M = ratio
    if Lf != M:
        k = torch.arange(-(-T * Lf // M), device=x.device)
        lo = torch.clamp(k * M // Lf, max=T - 2)
        f = ((k * M - lo * Lf).float() / Lf)[None, :, None, None]
        v = torch.lerp(v[:, lo], v[:, lo + 1], f)
    v = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    G, out = [None] * K, torch.empty(B, v.shape[1], K, 4, device=x.device)
    for k in range(K):
        if pb[k] < 0:
            G[k] = arc(rest[k], v[:, :, k], halves[k])
            out[:, :, k] = G[k]
        else:
            P = G[pb[k]]
            loc = arc(rest[k], qrot(P * conj, v[:, :, k]), halves[k])
            G[k] = qmul(P, loc)
            out[:, :, k] = loc
    return out


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
    cases = {"u8_30s_x8": ([frames_of(30)] * 8, 8, (1, 1), False), "ten_min_x32": ([frames_of(600)], 32, (1, 1), False),
             "ragged64_x4": (ragged, 4, (1, 1), False), "ragged64_x4_30fps": (ragged, 4, (2, 1), False),
             "step_1": ([H], 1, (1, 1), True), "step_8": ([H] * 8, 1, (1, 1), True), "step_64": ([H] * 64, 1, (1, 1), True)}
    mean = (torch.randn(sk.pose_dim, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    pose = sk.rest_pose(np.random.default_rng(2).standard_normal((sk.K, 3)))
    rest = torch.from_numpy(pose.unit32).to(dev)
    pb = sk.bone_parents.tolist()
    e = torch.eye(3, device=dev)[rest.abs().argmin(1)]
    n = torch.linalg.cross(rest, e)
    halves = torch.cat([torch.zeros(sk.K, 1, device=dev), n / n.norm(dim=1, keepdim=True)], 1)
    conj = torch.tensor([1.0, -1.0, -1.0, -1.0], device=dev)

    def make(frames, R):
        """Bone vectors around the rest pose (swings well below a half turn), times positive scales, minus the mean; zeros behind a row's end."""
        g = torch.Generator(device=dev).manual_seed(len(frames))
        shape = (len(frames) * R, max(frames), sk.K, 3)
        x = (rest + 0.4 * torch.randn(shape, generator=g, device=dev)) * (0.5 + torch.rand(shape[:3] + (1,), generator=g, device=dev))
        x = x.view(shape[0], shape[1], sk.pose_dim) - mean
        live = torch.arange(max(frames), device=dev)[None, :] < torch.tensor(frames, device=dev).repeat_interleave(R)[:, None]
        return (x * live[:, :, None]).contiguous()

    def setup(name):
        frames, R, ratio, step = cases[name]
        x = make(frames, R)
        d_frames = torch.ones(len(frames), dtype=torch.int32, device=dev) if step else torch.tensor(frames, dtype=torch.int32, device=dev)
        unit = H if step else 1                                       # a stream step passes its 0 / 1 valid flags
        t_out = -(-x.shape[1] * ratio[0] // ratio[1])
        out = torch.empty(x.shape[0], t_out, sk.K, 4, device=dev)
        run = lambda: SK.launch_rotations(x, sk, pose, d_frames, R, unit, mean, "local", ratio, out=out)
        return frames, R, ratio, x, out, run

    if a.eager_case:
        _f, _R, _r, _x, out, run = setup(a.eager_case)
        for _ in range(a.eager_iters):
            run()
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "finite": bool(torch.isfinite(out).all())}))
        return

    res = {"metric": "skeleton_rotations", "unit": "device events, graphs replayed; host: wall clock from the device tensor to the numpy result",
           "rounds": a.rounds, "window_s": a.window_s, "tile_frames": SK.TILE_FRAMES, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R, ratio, x, out, run = setup(name)
            g_new, _ = graph_of(run)
            g_old, y_old = graph_of(lambda: composition(x, pb, rest, halves, conj, mean, ratio), warmup=2)
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
            if not a.no_host:
                fr = None if min(frames) == max(frames) else frames
                fps = None if ratio == (1, 1) else (FPS, FPS * ratio[0] // ratio[1])
                xs = x.view(len(frames), R, x.shape[1], sk.pose_dim)
                mh = mean.cpu().numpy()
                host = []
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    y = SK.rotations_from_tracks(xs.cpu().numpy(), sk, pose, frames=fr, mean=mh, fps=fps)
                    host.append((time.perf_counter() - t0) * 1e3)
                y = y[0] if isinstance(y, tuple) else y
                entry["host_copy_plus_numpy"] = summary(host)
                entry["host_over_graph"] = round(statistics.median(host) / statistics.median(t["graph"]), 1)
                entry["max_abs_diff_vs_host"] = float(np.abs(out.cpu().numpy().reshape(y.shape) - y).max())
            entry["replays_per_window"] = reps["graph"]
            res[name] = entry
            del x, out, buf, dst, g_new, g_old, g_floor, y_old
            torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
