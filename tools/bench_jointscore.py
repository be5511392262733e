#!/usr/bin/env python3
"""SRGR and L1 diversity (jointscore.launch_srgr / launch_l1div: eg_srgr_tracks, eg_l1div_tracks) timed on the joints of whole tracks with
the TED geometry (43 joints, 30 new poses per 2 s window + 4) -- bench_skeleton.py's four shapes: 8 recordings x 30 s x 8 takes, 1 x 10 min
x 32 takes, 64 ragged recordings of 12-89 s x 4 takes at the native rate and at 15 -> 30 fps (twice the frames).  The targets are random
walks (steps of about 1 cm), the takes sit within 7 cm per coordinate of their recording's target, the weights are uniform in [0, 1).  One
captured graph per contender, device events after warm-up, alternating rounds: every timed window is sized to at least --window-s seconds
of replays, --rounds windows per figure: median, min and max.

Beside each of the two calls:
  composition  the same definition from torch ops on the same GPU, on the padded rectangle with masks: subtract, abs, widen, add, compare,
               masked sums (SRGR); widen, masked mean, subtract, abs, masked sum (L1 diversity);
  floor        a device copy that moves the same bytes: (bytes in + bytes out) / 2 read and written;
  host         copy the joints to the host and run the numpy definition there (srgr_of_joints / l1div_of_tracks on arrays; host clock from
               the device tensors to the numpy result).
The expectation the result is held against: SRGR reads results and targets once, L1 diversity reads its input twice, and both write almost
nothing, while a composition makes a pass per operator; so each call should sit within a small multiple of its floor and ahead of its
composition at every shape ("rule_holds": the slowest window of the kernel beats the fastest window of the composition).  Whatever is
measured is written down.

    python tools/bench_jointscore.py [--rounds 5] [--window-s 0.2] [--out profiles/jointscore_bench_line.json]
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
from tools._timing import alternate, graph_of, summary, write_line  # noqa: E402
H, P, J = 30, 4, 43


def frames_of(seconds):
    return -(-int(seconds * 16000) // 32000) * H + P


def srgr_composition(r, g, w, n, R, threshold, scale):
    """r [rows, T, J, 3], g [rows / R, T, J, 3], w [rows / R, T] fp32, n [rows] int64 -> (srgr [rows], recall [rows] float64, hits [rows, J])."""
    rows, T, Jn, _ = r.shape
    a = (r.view(rows // R, R, T, Jn, 3) - g[:, None]).abs().double()
    hit = (((a[..., 0] + a[..., 1]) + a[..., 2]) < threshold).view(rows, T, Jn)
    hit = hit & (torch.arange(T, device=r.device)[None, :, None] < n[:, None, None])
    hits = hit.sum(1, dtype=torch.int32)
    cells = n.double() * Jn
    weighted = (hit.sum(2).double().view(rows // R, R, T) * w.double()[:, None]).sum(2).reshape(rows)
    return weighted * scale / cells, hits.sum(1).double() / cells, hits


def l1_composition(x, n):
    """x [rows, T, D] fp32, n [rows] int64 -> (mean [rows, D], l1_sum [rows], l1div [rows]) float64."""
    valid = (torch.arange(x.shape[1], device=x.device)[None, :] < n[:, None])[:, :, None]
    v = torch.where(valid, x.double(), 0.0)
    mean = v.sum(1) / n.double()[:, None]
    l1 = torch.where(valid, (v - mean[:, None]).abs(), 0.0).sum((1, 2))
    return mean, l1, l1 / n.double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--cases", default="u8_30s_x8,ten_min_x32,ragged64_x4,ragged64_x4_30fps")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import jointscore as JS
    dev = torch.device("cuda:0")
    lib = JS.L.load()
    rng = np.random.default_rng(64)
    ragged = [frames_of(s) for s in rng.uniform(12, 89, 64)]
    # name -> (frames per recording, takes, output frames per source frame)
    cases = {"u8_30s_x8": ([frames_of(30)] * 8, 8, 1), "ten_min_x32": ([frames_of(600)], 32, 1), "ragged64_x4": (ragged, 4, 1),
             "ragged64_x4_30fps": (ragged, 4, 2)}
    res = {"metric": "jointscore_srgr_l1div", "unit": "device events, graphs replayed; host: wall clock from the device tensors to the numpy result",
           "rounds": a.rounds, "window_s": a.window_s, "tile_frames": JS.TILE_FRAMES, "joints": J, "device": torch.cuda.get_device_name(dev)}
    holds = True
    med = lambda v: statistics.median(v)
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R, up = cases[name]
            frames = [n * up for n in frames]
            U, rows, T = len(frames), len(frames) * R, max(frames)
            gen = torch.Generator(device=dev).manual_seed(U)
            n_rec = torch.tensor(frames, device=dev)
            n_rows = n_rec.repeat_interleave(R)
            keep = lambda n: (torch.arange(T, device=dev)[None, :] < n[:, None])[:, :, None, None]
            g = (torch.cumsum(torch.randn(U, T, J, 3, generator=gen, device=dev) * (0.01 / up), 1) * keep(n_rec)).contiguous()
            r = ((g.repeat_interleave(R, 0) + (torch.rand(rows, T, J, 3, generator=gen, device=dev) - 0.5) * 0.14) * keep(n_rows)).contiguous()
            w = torch.rand(U, T, generator=gen, device=dev)
            x = r.view(rows, T, J * 3)
            d_frames = torch.tensor(frames, dtype=torch.int32, device=dev)
            ws_s = torch.empty(int(lib.eg_srgr_workspace_bytes(rows, T, J)), dtype=torch.uint8, device=dev)
            ws_l = torch.empty(int(lib.eg_l1div_workspace_bytes(rows, T, J * 3)), dtype=torch.uint8, device=dev)
            out_s = tuple(torch.empty_like(t) for t in JS.launch_srgr(r, g, w, frames, d_frames, R, workspace=ws_s))
            out_l = tuple(torch.empty_like(t) for t in JS.launch_l1div(x, frames, d_frames, R, workspace=ws_l))
            g_s, _ = graph_of(lambda: JS.launch_srgr(r, g, w, frames, d_frames, R, workspace=ws_s, out=out_s))
            g_l, _ = graph_of(lambda: JS.launch_l1div(x, frames, d_frames, R, workspace=ws_l, out=out_l))
            c_s, y_s = graph_of(lambda: srgr_composition(r, g, w, n_rows, R, 0.1, JS.SCALE), warmup=2)
            c_l, y_l = graph_of(lambda: l1_composition(x, n_rows), warmup=2)
            cells = sum(frames) * J * 3
            bytes_s = 4 * (R + 1) * cells + 4 * sum(frames) + 16 * rows + 4 * rows * J
            bytes_l = 2 * 4 * R * cells + 8 * rows * (J * 3 + 2)
            copies = {}
            for key, nbytes in (("srgr", bytes_s), ("l1div", bytes_l)):
                src = torch.empty(max(1, nbytes // 8), dtype=torch.float32, device=dev)
                dst = torch.empty_like(src)
                copies[key] = (graph_of(lambda s=src, d=dst: d.copy_(s))[0], src, dst)
            g_s.replay()
            g_l.replay()
            torch.cuda.synchronize()
            rel = lambda got, want: float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
            entry = {"recordings": U, "takes": R, "frames": [min(frames), max(frames)], "frames_in": R * sum(frames),
                     "srgr": {"bytes": bytes_s, "workspace_bytes": ws_s.numel(), "launches": 2, "hits_equal_composition": bool(torch.equal(out_s[2], y_s[2])),
                              "max_rel_diff_vs_composition": rel(out_s[0], y_s[0]), "mean_recall": float(out_s[1].mean())},
                     "l1div": {"bytes": bytes_l, "workspace_bytes": ws_l.numel(), "launches": 4, "max_rel_diff_vs_composition": rel(out_l[1], y_l[1]),
                               "mean_l1div": float(out_l[2].mean())}}
            t, reps = alternate({"srgr": g_s, "srgr_composition": c_s, "srgr_floor": copies["srgr"][0], "l1div": g_l, "l1div_composition": c_l,
                                 "l1div_floor": copies["l1div"][0]}, a.rounds, a.window_s)
            for key, nbytes in (("srgr", bytes_s), ("l1div", bytes_l)):
                e = entry[key]
                e["graph"], e["composition"], e["floor"] = summary(t[key]), summary(t[key + "_composition"]), summary(t[key + "_floor"])
                e["GBps"] = round(nbytes / (med(t[key]) * 1e-3) / 1e9, 1)
                e["graph_over_floor"] = round(med(t[key]) / med(t[key + "_floor"]), 2)
                e["composition_over_graph"] = round(med(t[key + "_composition"]) / med(t[key]), 2)
                e["rule_holds"] = bool(max(t[key]) < min(t[key + "_composition"]))
                e["replays_per_window"] = reps[key]
                holds &= e["rule_holds"]
            if not a.no_host:
                rs, host_s, host_l = r.view(U, R, T, J, 3), [], []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ys = JS.srgr_of_joints(rs.cpu().numpy(), g.cpu().numpy(), w.cpu().numpy(), frames=frames)
                    host_s.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    yl = JS.l1div_of_tracks(rs.cpu().numpy().reshape(U, R, T, J * 3), frames=frames)
                    host_l.append((time.perf_counter() - t0) * 1e3)
                entry["srgr"]["host_copy_plus_numpy"] = summary(host_s)
                entry["srgr"]["host_over_graph"] = round(med(host_s) / med(t["srgr"]), 1)
                entry["srgr"]["hits_equal_host"] = bool(np.array_equal(out_s[2].cpu().numpy(), ys["hits"].reshape(rows, J)))
                entry["srgr"]["srgr_equals_host"] = bool(np.array_equal(out_s[0].cpu().numpy(), ys["srgr"].reshape(rows)))
                entry["l1div"]["host_copy_plus_numpy"] = summary(host_l)
                entry["l1div"]["host_over_graph"] = round(med(host_l) / med(t["l1div"]), 1)
                entry["l1div"]["max_rel_diff_vs_host"] = float((np.abs(out_l[1].cpu().numpy() - yl["l1_sum"].reshape(rows)) / yl["l1_sum"].reshape(rows)).max())
            res[name] = entry
            del r, g, w, x, out_s, out_l, ws_s, ws_l, g_s, g_l, c_s, c_l, y_s, y_l, copies
            torch.cuda.empty_cache()
    res["rule_holds_everywhere"] = holds
    write_line(res, a.out)


if __name__ == "__main__":
    main()
