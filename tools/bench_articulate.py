#!/usr/bin/env python3
"""Articulated-body output (skeleton.launch_articulate: eg_articulate_forward) timed on bench_skeleton.py's shapes with a 47-joint body and
pose_dim = 282 -- 8 recordings x 30 s x 8 takes, 1 x 10 min x 32 takes, 64 ragged recordings of 12-89 s x 4 takes at the native rate and
resampled 15 -> 30 fps -- and on one stream step (50 poses per row) for 1, 8 and 64 rows; joints only, local rotations only, and both from one
launch.  One captured graph per contender, device events after warm-up, alternating rounds (tools/_timing.py).

Beside every case:
  composition  the same definition from torch ops on the same GPU, joints and rotations: Gram-Schmidt, a loop over the 47 joints of batched
               3x3 products, matrix-to-quaternion (torch.lerp between gathered frames for the rate change, on the padded rectangle);
  floor        a device copy that moves the bytes of the launch with both outputs: (bytes in + bytes out) / 2 read and written;
  host         copy the track to the host and run the float64 numpy definition there, joints and rotations (host clock from the device
               tensor to the numpy results).
No time is fixed in advance: the ratios are reported, and ``rule`` says whether the slowest window of the kernel (both outputs) beat the
fastest window of the composition.
Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_articulate.py --eager-case ten_min_x32

    python tools/bench_articulate.py [--rounds 5] [--window-s 0.4] [--out profiles/articulate_bench_line.json]
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
from tools.bench_skeleton import FPS, frames_of  # noqa: E402

H = 50                                                            # the poses a BEAT-shaped stream step emits per row (60 - 10)


def synthetic_tree(SK, basis="rows"):
    """A 47-joint upper body: a spine chain of 9, two arms of 4 from the chest, five three-joint fingers per hand; offsets of 3-30 cm."""
    parents = [-1, 0, 1, 2, 3, 4, 5, 6, 7]
    for _side in range(2):
        parents.append(4)
        for _ in range(3):
            parents.append(len(parents) - 1)
        wrist = len(parents) - 1
        for _f in range(5):
            parents += [wrist, len(parents), len(parents) + 1]
    rng = np.random.default_rng(47)
    off = rng.standard_normal((47, 3))
    off = off / np.linalg.norm(off, axis=1, keepdims=True) * rng.uniform(0.03, 0.3, (47, 1))
    return SK.JointTree(parents, off, basis=basis)


def quat_of(m):
    """m [..., 3, 3] -> unit quaternions [..., 4], w >= 0: the branch of the first largest of (trace, m00, m11, m22)."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.flatten(-2).unbind(-1)
    tr = m00 + m11 + m22
    cand = torch.stack([torch.stack([1 + tr, m21 - m12, m02 - m20, m10 - m01], -1), torch.stack([m21 - m12, 1 + m00 - m11 - m22, m01 + m10, m02 + m20], -1),
                        torch.stack([m02 - m20, m01 + m10, 1 - m00 + m11 - m22, m12 + m21], -1),
                        torch.stack([m10 - m01, m02 + m20, m12 + m21, 1 - m00 - m11 + m22], -1)], -2)
    pick = torch.stack([tr, m00, m11, m22], -1).argmax(-1)
    q = cand.gather(-2, pick[..., None, None].expand(pick.shape + (1, 4))).squeeze(-2)
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.where(q[..., :1] < 0, -q, q)


def composition(x, parents, off, mean, ratio):
    """x [B, T, 6J] -> (joints [B, T_out, J, 3], local rotations [B, T_out, J, 4]) from torch ops (basis rows)."""
    B, T, _D = x.shape
    J = len(parents)
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
    R = torch.stack([b1, b2, torch.linalg.cross(b1, b2)], -2)
    G, p = [None] * J, [None] * J
    for j in range(J):
        a = parents[j]
        if a < 0:
            G[j], p[j] = R[:, :, j], off[j].expand(B, R.shape[1], 3)
        else:
            G[j] = G[a] @ R[:, :, j]
            p[j] = p[a] + G[a] @ off[j]
    return torch.stack(p, 2), quat_of(R)


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
    tree = synthetic_tree(SK)
    J = tree.J
    rng = np.random.default_rng(64)
    ragged = [frames_of(s) for s in rng.uniform(12, 89, 64)]
    cases = {"u8_30s_x8": ([frames_of(30)] * 8, 8, (1, 1), False), "ten_min_x32": ([frames_of(600)], 32, (1, 1), False),
             "ragged64_x4": (ragged, 4, (1, 1), False), "ragged64_x4_30fps": (ragged, 4, (2, 1), False),
             "step_1": ([H], 1, (1, 1), True), "step_8": ([H] * 8, 1, (1, 1), True), "step_64": ([H] * 64, 1, (1, 1), True)}
    mean = (torch.randn(tree.pose_dim, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    parents = tree.parents.tolist()
    off = torch.from_numpy(tree.offsets32).to(dev)

    def make(frames, R):
        """6-D groups around the identity's two rows, well away from degenerate, minus the mean; zeros behind a row's end."""
        g = torch.Generator(device=dev).manual_seed(len(frames))
        shape = (len(frames) * R, max(frames), J, 6)
        base = torch.tensor([1.0, 0, 0, 0, 1.0, 0], device=dev)
        x = (base + 0.3 * torch.randn(shape, generator=g, device=dev)) * (0.5 + torch.rand(shape[:3] + (1,), generator=g, device=dev))
        x = x.view(shape[0], shape[1], tree.pose_dim) - mean
        live = torch.arange(max(frames), device=dev)[None, :] < torch.tensor(frames, device=dev).repeat_interleave(R)[:, None]
        return (x * live[:, :, None]).contiguous()

    def setup(name):
        frames, R, ratio, step = cases[name]
        x = make(frames, R)
        d_frames = torch.ones(len(frames), dtype=torch.int32, device=dev) if step else torch.tensor(frames, dtype=torch.int32, device=dev)
        unit = H if step else 1                                       # a stream step passes its 0 / 1 valid flags
        t_out = -(-x.shape[1] * ratio[0] // ratio[1])
        oj, oq = torch.empty(x.shape[0], t_out, J, 3, device=dev), torch.empty(x.shape[0], t_out, J, 4, device=dev)
        runs = {"both": lambda: SK.launch_articulate(x, tree, d_frames, R, unit, mean, "local", ratio, out_joints=oj, out_rotations=oq),
                "joints": lambda: SK.launch_articulate(x, tree, d_frames, R, unit, mean, "local", ratio, out_joints=oj, rotations=False),
                "rotations": lambda: SK.launch_articulate(x, tree, d_frames, R, unit, mean, "local", ratio, out_rotations=oq, joints=False)}
        return frames, R, ratio, x, oj, oq, runs

    if a.eager_case:
        _f, _R, _r, _x, oj, oq, runs = setup(a.eager_case)
        for _ in range(a.eager_iters):
            runs["both"]()
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "finite": bool(torch.isfinite(oj).all() and torch.isfinite(oq).all())}))
        return

    res = {"metric": "articulate_forward", "unit": "device events, graphs replayed; host: wall clock from the device tensor to the numpy results",
           "rounds": a.rounds, "window_s": a.window_s, "joints": J, "tile_frames": SK.ARTICULATE_TILE_FRAMES, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R, ratio, x, oj, oq, runs = setup(name)
            graphs = {k: graph_of(run)[0] for k, run in runs.items()}
            graphs["composition"], (yj, yq) = graph_of(lambda: composition(x, parents, off, mean, ratio), warmup=2)
            n_out = [-(-n * ratio[0] // ratio[1]) for n in frames]
            nbytes = 4 * (R * sum(frames) * tree.pose_dim + R * sum(n_out) * 7 * J)
            buf = torch.empty(max(1, nbytes // 8), dtype=torch.float32, device=dev)
            dst = torch.empty_like(buf)
            graphs["floor"] = graph_of(lambda: dst.copy_(buf))[0]
            graphs["both"].replay()
            torch.cuda.synchronize()
            full = [u for u, n in enumerate(frames) if n == max(frames)]      # the composition works on the padded rectangle
            rows = [u * R + r for u in full for r in range(R)]
            entry = {"recordings": len(frames), "takes": R, "L": ratio[0], "M": ratio[1], "frames": [min(frames), max(frames)],
                     "frames_in": R * sum(frames), "frames_out": R * sum(n_out), "bytes": nbytes, "launches": 1,
                     "max_abs_diff_vs_composition": {"joints": float((oj[rows] - yj[rows]).abs().max()),
                                                     "rotations": float(torch.minimum((oq[rows] - yq[rows]).abs(), (oq[rows] + yq[rows]).abs()).max())}}
            t, reps = alternate(graphs, a.rounds, a.window_s)
            for k, v in t.items():
                entry[k] = summary(v)
            med = {k: statistics.median(v) for k, v in t.items()}
            sec = med["both"] * 1e-3
            entry["GBps"] = round(nbytes / sec / 1e9, 1)
            entry["ns_per_output_frame"] = round(1e9 * sec / (R * sum(n_out)), 4)
            entry["both_over_floor"] = round(med["both"] / med["floor"], 2)
            entry["both_over_joints_plus_rotations"] = round(med["both"] / (med["joints"] + med["rotations"]), 2)
            entry["composition_over_both"] = round(med["composition"] / med["both"], 2)
            entry["rule"] = bool(max(t["both"]) < min(t["composition"]))
            if not a.no_host:
                fr = None if min(frames) == max(frames) else frames
                fps = None if ratio == (1, 1) else (FPS, FPS * ratio[0] // ratio[1])
                xs = x.view(len(frames), R, x.shape[1], tree.pose_dim)
                mh = mean.cpu().numpy()
                host = []
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    xh = xs.cpu().numpy()
                    hj = SK.joints_from_rot6d(xh, tree, frames=fr, mean=mh, fps=fps)
                    hq = SK.rotations_from_rot6d(xh, tree, frames=fr, mean=mh, fps=fps)
                    host.append((time.perf_counter() - t0) * 1e3)
                hj, hq = (y[0] if isinstance(y, tuple) else y for y in (hj, hq))
                entry["host_copy_plus_numpy"] = summary(host)
                entry["host_over_both"] = round(statistics.median(host) / med["both"], 1)
                gq = oq.cpu().numpy().reshape(hq.shape)
                entry["max_abs_diff_vs_host"] = {"joints": float(np.abs(oj.cpu().numpy().reshape(hj.shape) - hj).max()),
                                                 "rotations": float(np.minimum(np.abs(gq - hq), np.abs(gq + hq)).max())}
            entry["replays_per_window"] = reps["both"]
            res[name] = entry
            del x, oj, oq, buf, dst, graphs, yj, yq
            torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
