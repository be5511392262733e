#!/usr/bin/env python3
"""Preview frames (preview.render_joints: eg_preview_raster) timed on whole takes of the 43-joint TED body (42 bones, radius 1.5, the default
orbit camera at 1.4 m across the picture), at 240 x 320 and at 120 x 160:

  u8_30s_x8        8 recordings x 30 s x 8 takes at 15 fps
  ragged64_x4      64 recordings of 14-88 s x 4 takes at 15 fps, and the same at 30 fps (ragged64_x4_30fps)
  ten_min_30fps    one ten-minute take at 30 fps

A shape whose pictures would not fit PreviewSpec's default max_bytes (8 GiB) is shrunk by dropping recordings from its end until it does; the
entry then says so ("shrunk_from_recordings").  One captured graph per contender, device events after warm-up, alternating rounds: every timed
window holds at least --window-s seconds of replays, --rounds windows per figure: median, min and max.

Contenders:
  graph        (a) the one launch;
  composition  (b) the same definition from torch ops on the same GPU, a loop over the bones on [N, H, W] tensors.  It runs on the first
               --composition-frames valid frames of the shape (its temporaries are ten fp32 tensors of N x H x W) and the time is scaled to
               the shape's valid frames: labelled "scaled"; elementwise passes over >= 10^7 pixels scale linearly;
  floor        (c) a device fill of the same output bytes;
  host         (d) the numpy definition (preview.render_joints on numpy input) on 16 frames, host clock, scaled to the shape: "scaled";
  matplotlib   (e) a 3-D matplotlib figure per frame as the reference draws it, 16 frames, scaled; only where matplotlib is importable.
The project's rule against the composition: the slowest window of the launch beats the fastest (scaled) window of the composition at every
shape ("rule_holds").  The ratio to the floor is reported, not gated.
Kernel statistics or counters, in a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/bench_preview.py --eager-case u8_30s_x8@240

    python tools/bench_preview.py [--rounds 5] [--window-s 0.3] [--out profiles/preview_bench_line.json]
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
H_NEW, PRIOR = 30, 4
SIZES = {"240": (240, 320), "120": (120, 160)}


def frames_of(seconds, fps):
    return (-(-int(seconds * 16000) // 32000) * H_NEW + PRIOR) * fps // 15


def composition(joints, spec, out):
    """joints [N, J, 3] fp32 on the device -> out [N, H, W, 3] uint8: the definition, one bone at a time on [N, H, W] tensors."""
    dev = joints.device
    m, c = [float(v) for v in spec.camera.matrix.reshape(-1)], [float(v) for v in spec.camera.centre]
    x, y, z = joints[..., 0], joints[..., 1], joints[..., 2]
    u = ((m[0] * x + m[1] * y) + m[2] * z) + c[0]
    v = ((m[3] * x + m[4] * y) + m[5] * z) + c[1]
    X = (torch.arange(spec.width, dtype=torch.float32, device=dev) + 0.5)[None, None, :]
    Y = (torch.arange(spec.height, dtype=torch.float32, device=dev) + 0.5)[None, :, None]
    reach = float(np.float32(spec.radius) + np.float32(0.5))
    N = joints.shape[0]
    img = [torch.full((N, spec.height, spec.width), int(g), dtype=torch.int32, device=dev) for g in spec.ground]
    for k, (ja, jb) in enumerate(spec.bones):
        ax, ay = u[:, ja, None, None], v[:, ja, None, None]
        ex, ey = u[:, jb, None, None] - ax, v[:, jb, None, None] - ay
        l2 = ex * ex + ey * ey
        inv = torch.where(l2 > 0, 1.0 / l2, torch.zeros_like(l2))
        wx, wy = X - ax, Y - ay
        s = (wx * ex + wy * ey) * inv
        t = torch.where(s < 0, torch.zeros_like(s), s)
        t = torch.where(t > 1, torch.ones_like(t), t)
        dx, dy = wx - t * ex, wy - t * ey
        a = reach - torch.sqrt(dx * dx + dy * dy)
        part = a > 0
        q = torch.where(a >= 1, 255, torch.where(part, (torch.where(part, a, torch.zeros_like(a)) * 255.0 + 0.5).to(torch.int32), 0))
        for ch in range(3):
            img[ch] = torch.div(img[ch] * (255 - q) + int(spec.colours[k][ch]) * q + 127, 255, rounding_mode="floor")
    out.copy_(torch.stack(img, -1))
    return out


def matplotlib_frames(joints, bones, n):
    """The reference's figure (create_video_and_save: one 3-D axes, a plot call per bone, view_init(20, -60)) drawn for n frames: ms per frame."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig = plt.figure(figsize=(4, 4), dpi=80)
    ax = fig.add_subplot(1, 1, 1, projection="3d")
    ax.view_init(elev=20, azim=-60)
    t0 = time.perf_counter()
    for i in range(n):
        pose = joints[i]
        ax.clear()
        for a, b in bones:
            ax.plot([pose[a, 0], pose[b, 0]], [pose[a, 2], pose[b, 2]], [pose[a, 1], pose[b, 1]], zdir="z", linewidth=1.5)
        ax.set_xlim3d(-0.5, 0.5)
        ax.set_ylim3d(0.5, -0.5)
        ax.set_zlim3d(0.5, -0.5)
        fig.canvas.draw()
    dt = (time.perf_counter() - t0) * 1e3 / n
    plt.close(fig)
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--cases", default="u8_30s_x8,ragged64_x4,ragged64_x4_30fps,ten_min_30fps")
    ap.add_argument("--sizes", default="240,120")
    ap.add_argument("--composition-frames", type=int, default=1024)
    ap.add_argument("--eager-case", default=None, help="NAME@SIZE: run that case eagerly --eager-iters times and exit (for a rocprofv3 run)")
    ap.add_argument("--eager-iters", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import preview as PV
    from emotiongestures_amd import skeleton as SK
    dev = torch.device("cuda:0")
    sk = SK.ted_expressive()
    rng = np.random.default_rng(64)
    seconds = rng.uniform(14, 88, 64)
    # name -> (frames per recording, takes, fps)
    cases = {"u8_30s_x8": ([frames_of(30, 15)] * 8, 8, 15), "ragged64_x4": ([frames_of(s, 15) for s in seconds], 4, 15),
             "ragged64_x4_30fps": ([frames_of(s, 30) for s in seconds], 4, 30), "ten_min_30fps": ([frames_of(600, 30)], 1, 30)}

    def setup(name, size):
        frames, R, fps = cases[name]
        Hh, Ww = SIZES[size]
        spec = PV.PreviewSpec(sk, Hh, Ww, camera=PV.Camera.orbit(span=1.4, height=Hh, width=Ww), radius=1.5)
        full = len(frames)
        while len(frames) > 1 and spec.out_bytes(len(frames) * R, max(frames)) > spec.max_bytes:
            frames = frames[:-1]
        spec.fit(len(frames) * R, max(frames), f"bench_preview: {name}@{size}")
        g = torch.Generator(device=dev).manual_seed(len(frames))
        track = torch.randn(len(frames) * R, max(frames), sk.pose_dim, generator=g, device=dev)
        joints = SK.launch_joints(track, sk, None, 1, 1, None, True, (1, 1))              # unit bones: the body at its real size
        del track
        d_frames = torch.tensor(frames, dtype=torch.int32, device=dev)
        out = torch.empty((len(frames) * R, max(frames)) + spec.frame_shape(), dtype=torch.uint8, device=dev)
        return frames, R, fps, spec, joints, d_frames, out, full, (lambda: PV.launch_preview(joints, spec, d_frames, R, out=out))

    if a.eager_case:
        name, size = a.eager_case.split("@")
        *_rest, out, _full, run = setup(name, size)
        for _ in range(a.eager_iters):
            run()
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "bytes": out.numel()}))
        return

    res = {"metric": "preview_frames", "unit": "device events, graphs replayed; host and matplotlib: wall clock on 16 frames, scaled",
           "rounds": a.rounds, "window_s": a.window_s, "bones": len(sk.dir_vec_pairs), "radius": 1.5, "composition_frames": a.composition_frames,
           "device": torch.cuda.get_device_name(dev)}
    holds, losers = True, []
    with torch.no_grad():
        for name in a.cases.split(","):
            for size in a.sizes.split(","):
                frames, R, fps, spec, joints, d_frames, out, full, run = setup(name, size)
                valid = R * sum(frames)
                g_new, _ = graph_of(run)
                # the first composition_frames valid frames of the shape, row by row
                pick = [(b, t) for b in range(len(frames) * R) for t in range(frames[b // R])][:a.composition_frames]
                pb, pt = (torch.tensor(v, device=dev) for v in zip(*pick))
                sample = joints[pb, pt].contiguous()
                y_buf = torch.empty((len(pick), spec.height, spec.width, 3), dtype=torch.uint8, device=dev)
                g_old, y_old = graph_of(lambda: composition(sample, spec, y_buf), warmup=2)
                g_floor, _ = graph_of(lambda: out.fill_(255))
                g_new.replay()
                torch.cuda.synchronize()
                mine = out[pb, pt]
                scale_b = valid / len(pick)
                entry = {"recordings": len(frames), "takes": R, "fps": fps, "height": spec.height, "width": spec.width,
                         "frames": [min(frames), max(frames)], "frames_valid": valid, "frames_written": out.shape[0] * out.shape[1],
                         "bytes": out.numel(), "bytes_equal_composition": bool(torch.equal(mine, y_old)),
                         "share_of_pixels_drawn": round(float((mine != 255).any(-1).float().mean()), 4)}
                if len(frames) != full:
                    entry["shrunk_from_recordings"] = full
                t, reps = alternate({"graph": g_new, "composition": g_old, "floor": g_floor}, a.rounds, a.window_s)
                t["composition"] = [v * scale_b for v in t["composition"]]
                for k, v in t.items():
                    entry[k] = summary(v)
                entry["composition"]["scaled"] = f"measured on {len(pick)} frames, x {scale_b:.2f}"
                sec = statistics.median(t["graph"]) * 1e-3
                entry["GBps_written"] = round(out.numel() / sec / 1e9, 1)
                entry["ns_per_frame"] = round(1e9 * sec / (out.shape[0] * out.shape[1]), 2)
                entry["graph_over_floor"] = round(statistics.median(t["graph"]) / statistics.median(t["floor"]), 2)
                entry["share_above_floor"] = round(1 - statistics.median(t["floor"]) / statistics.median(t["graph"]), 3)
                entry["composition_over_graph"] = round(statistics.median(t["composition"]) / statistics.median(t["graph"]), 1)
                entry["rule_holds"] = bool(max(t["graph"]) < min(t["composition"]))
                holds &= entry["rule_holds"]
                if not entry["rule_holds"]:
                    losers.append(f"{name}@{size}")
                if not a.no_host:
                    few = sample[:16].cpu().numpy()
                    host = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        PV.render_joints(few, spec)
                        host.append((time.perf_counter() - t0) * 1e3 * valid / len(few))
                    entry["host_numpy"] = dict(summary(host), scaled=f"measured on {len(few)} frames, x {valid / len(few):.0f}")
                    entry["host_over_graph"] = round(statistics.median(host) / statistics.median(t["graph"]), 0)
                    try:
                        per = matplotlib_frames(few, spec.bones, len(few))
                        entry["matplotlib"] = {"ms_per_frame": round(per, 2), "scaled_ms": round(per * valid, 0),
                                               "over_graph": round(per * valid / statistics.median(t["graph"]), 0)}
                    except ImportError:
                        entry["matplotlib"] = "not importable here"
                entry["replays_per_window"] = reps["graph"]
                res[f"{name}@{size}"] = entry
                print(f"{name}@{size}: launch {entry['graph']['median_ms']} ms, floor {entry['floor']['median_ms']} ms, composition "
                      f"{entry['composition']['median_ms']} ms (scaled)", file=sys.stderr, flush=True)
                del joints, out, y_buf, y_old, mine, sample, g_new, g_old, g_floor
                torch.cuda.empty_cache()
    res["rule_holds_everywhere"] = holds
    res["rule_fails_at"] = losers
    write_line(res, a.out)


if __name__ == "__main__":
    main()
