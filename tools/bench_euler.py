#!/usr/bin/env python3
"""Euler channels (skeleton.launch_euler / launch_unwrap / launch_rot6d_euler: eg_articulate_euler, eg_angle_unwrap,
eg_articulate_rot6d_euler) timed on bench_articulate.py's shapes and 47-joint body -- 8 recordings x 30 s x 8 takes, 1 x 10 min x 32 takes, 64
ragged recordings of 12-89 s x 4 takes at the native rate and resampled 15 -> 30 fps -- and on one stream step (50 poses per row) for 1, 8 and
64 rows.  Contenders: the Euler launch alone, the Euler launch with the unwrap launches, and the inverse.  One captured graph per contender,
device events after warm-up, alternating rounds (tools/_timing.py).

Beside every case:
  composition  the same definition from torch ops on the same GPU: Gram-Schmidt, gathers by order, atan2 (torch.lerp between gathered frames
               for the rate change, on the padded rectangle);
  floor        a device copy that moves the bytes of the Euler launch: (bytes in + bytes out) / 2 read and written;
  host         copy the track to the host and run the float64 numpy definition there (host clock from the device tensor to the numpy result).
And once, for the ten-minute take: the host writer's time, ``BvhFile.format`` of one take of 47 joints (host clock), so that a reader can judge
whether formatting the MOTION text on the device would be worth building.
No time is fixed in advance: the ratios are reported, and ``rule`` says whether the slowest window of the Euler launch beat the fastest window
of the composition.

    python tools/bench_euler.py [--rounds 5] [--window-s 0.4] [--out profiles/euler_bench_line.json]
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
from tools.bench_articulate import H, synthetic_tree  # noqa: E402
from tools.bench_skeleton import FPS, frames_of  # noqa: E402


def composition(x, idx, eps, mean, ratio):
    """x [B, T, 6J] -> euler [B, T_out, J, 3] in degrees from torch ops (basis rows); idx [J, 7]: the flat matrix entries ii, ij, ik, jk, kk,
    kj, jj of every joint's order; eps [J]."""
    B, T, _D = x.shape
    J = idx.shape[0]
    v = (x + mean).view(B, T, J, 6)
    Lf, M = ratio
    if Lf != M:
        k = torch.arange(-(-T * Lf // M), device=x.device)
        lo = torch.clamp(k * M // Lf, max=T - 2)
        f = ((k * M - lo * Lf).float() / Lf)[None, :, None, None]
        v = torch.lerp(v[:, lo], v[:, lo + 1], f)
    a1, a2 = v[..., :3], v[..., 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u2 / u2.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    R = torch.stack([b1, b2, torch.linalg.cross(b1, b2)], -2).flatten(-2)
    g = R.gather(-1, idx.expand(R.shape[:-1] + (7,)))
    ii, ij, ik, jk, kk, kj, jj = g.unbind(-1)
    s = eps * ik
    free = 1 - s.abs() >= 2.0 ** -20
    b = torch.atan2(s, torch.sqrt(ii * ii + ij * ij))
    a = torch.where(free, torch.atan2(-eps * jk, kk), torch.atan2(eps * kj, jj))
    c = torch.where(free, torch.atan2(-eps * ij, ii), torch.zeros_like(s))
    return torch.stack([a, b, c], -1) * (180.0 / np.pi)


def bvh_of(tree, orders):
    """A BVH hierarchy text for the synthetic body: joint j3 .. named by number, centimetres."""
    kids = {j: [c for c in range(tree.J) if tree.parents[c] == j] for j in range(tree.J)}

    def node(j, depth):
        pad = "\t" * depth
        ch = " ".join(f"{a}rotation" for a in orders[j])
        head = f"{pad}{'ROOT' if j == 0 else 'JOINT'} j{j}\n{pad}{{\n{pad}\tOFFSET " + " ".join("%.6f" % (100 * v) for v in tree.offsets[j]) + "\n"
        head += f"{pad}\tCHANNELS {'6 Xposition Yposition Zposition ' if j == 0 else '3 '}{ch}\n"
        body = "".join(node(c, depth + 1) for c in kids[j]) or f"{pad}\tEnd Site\n{pad}\t{{\n{pad}\t\tOFFSET 0.000000 1.000000 0.000000\n{pad}\t}}\n"
        return head + body + f"{pad}}}\n"
    return "HIERARCHY\n" + node(0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--cases", default="u8_30s_x8,ten_min_x32,ragged64_x4,ragged64_x4_30fps,step_1,step_8,step_64")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import bvh as BVH
    from emotiongestures_amd import skeleton as SK
    dev = torch.device("cuda:0")
    tree = synthetic_tree(SK)
    J = tree.J
    orders = [SK.ORDERS[(4 + j) % 6] if j % 5 == 0 else "ZXY" for j in range(J)]       # mostly ZXY as in BEAT's files, every fifth joint another
    codes = SK.order_codes(orders, J)
    rows7 = []
    for code in codes:
        i, j, k, _e = SK.order_axes(code)
        rows7.append([3 * i + i, 3 * i + j, 3 * i + k, 3 * j + k, 3 * k + k, 3 * k + j, 3 * j + j])
    idx = torch.tensor(rows7, device=dev)
    eps = torch.tensor([SK.order_axes(c)[3] for c in codes], device=dev)
    rng = np.random.default_rng(64)
    ragged = [frames_of(s) for s in rng.uniform(12, 89, 64)]
    cases = {"u8_30s_x8": ([frames_of(30)] * 8, 8, (1, 1), False), "ten_min_x32": ([frames_of(600)], 32, (1, 1), False),
             "ragged64_x4": (ragged, 4, (1, 1), False), "ragged64_x4_30fps": (ragged, 4, (2, 1), False),
             "step_1": ([H], 1, (1, 1), True), "step_8": ([H] * 8, 1, (1, 1), True), "step_64": ([H] * 64, 1, (1, 1), True)}
    mean = (torch.randn(tree.pose_dim, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)

    def make(frames, R):
        """6-D groups around the identity's two rows, well away from degenerate, minus the mean; zeros behind a row's end."""
        g = torch.Generator(device=dev).manual_seed(len(frames))
        shape = (len(frames) * R, max(frames), J, 6)
        base = torch.tensor([1.0, 0, 0, 0, 1.0, 0], device=dev)
        x = (base + 0.3 * torch.randn(shape, generator=g, device=dev)) * (0.5 + torch.rand(shape[:3] + (1,), generator=g, device=dev))
        x = x.view(shape[0], shape[1], tree.pose_dim) - mean
        live = torch.arange(max(frames), device=dev)[None, :] < torch.tensor(frames, device=dev).repeat_interleave(R)[:, None]
        return (x * live[:, :, None]).contiguous()

    res = {"metric": "articulate_euler", "unit": "device events, graphs replayed; host: wall clock from the device tensor to the numpy result",
           "rounds": a.rounds, "window_s": a.window_s, "joints": J, "tile_frames": SK.ARTICULATE_TILE_FRAMES,
           "unwrap_tile_frames": SK.UNWRAP_TILE_FRAMES, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R, ratio, step = cases[name]
            x = make(frames, R)
            B = x.shape[0]
            d_frames = torch.ones(len(frames), dtype=torch.int32, device=dev) if step else torch.tensor(frames, dtype=torch.int32, device=dev)
            unit = H if step else 1                                   # a stream step passes its 0 / 1 valid flags
            n_out = [-(-n * ratio[0] // ratio[1]) for n in frames]
            t_out = -(-x.shape[1] * ratio[0] // ratio[1])
            d_out = d_frames if step else torch.tensor(n_out, dtype=torch.int32, device=dev)
            oe, ou = torch.empty(B, t_out, J, 3, device=dev), torch.empty(B, t_out, J, 3, device=dev)
            back = torch.empty(B, t_out, tree.pose_dim, device=dev)
            ws = SK.unwrap_workspace(B, t_out, 3 * J, dev)

            def with_unwrap():
                SK.launch_euler(x, tree, orders, d_frames, R, unit, mean, ratio, out=ou)
                SK.launch_unwrap(ou.view(B, t_out, 3 * J), d_out, R, unit, 360.0, ws)
            runs = {"euler": lambda: SK.launch_euler(x, tree, orders, d_frames, R, unit, mean, ratio, out=oe), "euler_unwrap": with_unwrap,
                    "inverse": lambda: SK.launch_rot6d_euler(oe, tree, orders, d_out, R, unit, mean, out=back)}
            graphs = {k: graph_of(run)[0] for k, run in runs.items()}
            graphs["composition"], ye = graph_of(lambda: composition(x, idx, eps, mean, ratio), warmup=2)
            nbytes = 4 * (R * sum(frames) * tree.pose_dim + R * sum(n_out) * 3 * J)
            buf = torch.empty(max(1, nbytes // 8), dtype=torch.float32, device=dev)
            dst = torch.empty_like(buf)
            graphs["floor"] = graph_of(lambda: dst.copy_(buf))[0]
            graphs["euler"].replay()
            torch.cuda.synchronize()
            full = [u for u, n in enumerate(frames) if n == max(frames)]      # the composition works on the padded rectangle
            rows = [u * R + r for u in full for r in range(R)]
            dd = (oe[rows] - ye[rows] + 180.0) % 360.0 - 180.0
            entry = {"recordings": len(frames), "takes": R, "L": ratio[0], "M": ratio[1], "frames": [min(frames), max(frames)],
                     "frames_in": R * sum(frames), "frames_out": R * sum(n_out), "bytes": nbytes,
                     "launches": {"euler": 1, "euler_unwrap": 2 if t_out <= SK.UNWRAP_TILE_FRAMES else 4, "inverse": 1},
                     "max_abs_diff_vs_composition_deg": float(dd.abs().max())}
            t, reps = alternate(graphs, a.rounds, a.window_s)
            for k, v in t.items():
                entry[k] = summary(v)
            med = {k: statistics.median(v) for k, v in t.items()}
            sec = med["euler"] * 1e-3
            entry["GBps"] = round(nbytes / sec / 1e9, 1)
            entry["ns_per_output_frame"] = round(1e9 * sec / (R * sum(n_out)), 4)
            entry["euler_over_floor"] = round(med["euler"] / med["floor"], 2)
            entry["euler_unwrap_over_euler"] = round(med["euler_unwrap"] / med["euler"], 2)
            entry["inverse_over_floor"] = round(med["inverse"] / med["floor"], 2)
            entry["composition_over_euler"] = round(med["composition"] / med["euler"], 2)
            entry["rule"] = bool(max(t["euler"]) < min(t["composition"]))
            if not a.no_host:
                fr = None if min(frames) == max(frames) else frames
                fps = None if ratio == (1, 1) else (FPS, FPS * ratio[0] // ratio[1])
                xs = x.view(len(frames), R, x.shape[1], tree.pose_dim)
                mh = mean.cpu().numpy()
                host = []
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    he = SK.euler_from_rot6d(xs.cpu().numpy(), tree, orders, frames=fr, mean=mh, fps=fps)
                    host.append((time.perf_counter() - t0) * 1e3)
                he = he[0] if isinstance(he, tuple) else he
                entry["host_copy_plus_numpy"] = summary(host)
                entry["host_over_euler"] = round(statistics.median(host) / med["euler"], 1)
                dh = (oe.cpu().numpy().reshape(he.shape) - he + 180.0) % 360.0 - 180.0
                entry["max_abs_diff_vs_host_deg"] = float(np.abs(dh).max())
            if name == "ten_min_x32":                                 # the host writer on one take of the ten-minute recording
                f = BVH.parse(bvh_of(tree, orders))
                take = ou[0]
                wr = []
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    text = f.format(take, frame_time=1.0 / FPS)
                    wr.append((time.perf_counter() - t0) * 1e3)
                entry["bvh_format_one_take"] = dict(summary(wr), frames=int(take.shape[0]), channels=f.channels, characters=len(text))
                entry["bvh_format_over_euler_unwrap_of_32_takes"] = round(statistics.median(wr) / med["euler_unwrap"], 1)
            entry["replays_per_window"] = reps["euler"]
            res[name] = entry
            del x, oe, ou, back, buf, dst, graphs, ye
            torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
