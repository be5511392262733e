#!/usr/bin/env python3
"""Take diversity of whole tracks (takes.take_diversity: eg_track_rows_pack -> FGD encoder -> eg_take_distance) timed on bench_beat_tracks.py's
shapes: 8 recordings of 30 s with 8 takes, 8 x 60 s x 8, 1 x 10 min x 32, and 64 recordings of 10-90 s with 4 takes on a padded rectangle
(282 pose columns, 15 fps).  Device events after warm-up, every timed window sized to at least --window-s seconds of calls, --rounds windows
per figure: median, min and max.

(a) the new call eagerly and as one captured graph, and its three stages as graphs of their own: pack, features (three products on the
    packed rows), distance (two launches).  The distance stage's achieved bytes per second stand beside its algorithmic bytes (every feature
    read once, N * K * 4) and the bytes its loads ask for (take r's chunk once per base take, every other take's once per pair).
(b) the composition a user has without it, on the same GPU: ``fgd(track)[1]`` on the padded rectangle (padding included), then masked fp64
    pairwise differences in torch, one base take at a time (the [U, R, R, T, 512] fp64 broadcast does not fit the larger shapes).
New call and composition alternate inside one process; outputs are compared (the composition sums in another order: relative difference).

--ab-lib OTHER.so: also times eg_take_distance of a second build of the library on the same features, alternating (e.g. a build that stages
take r's chunk in LDS instead of registers), and reports whether the two agree bit for bit.
Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_take_diversity.py --eager-case ten_min_r32

    python tools/bench_take_diversity.py [--rounds 5] [--window-s 0.4] [--out profiles/take_diversity_bench_line.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import alternate, graph_of, summary, write_line  # noqa: E402
SR, FPS, D, K = 16000, 15, 282, 512


def make(frames, R, seed, dev):
    """Cumulative-sum poses [U, R, Tmax, 282] made on the device, zero beyond frames[u] (what the ragged roll-out leaves there)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    U, Tmax = len(frames), max(frames)
    track = torch.cumsum(torch.randn(U, R, Tmax, D, generator=g, device=dev) * 0.05, dim=2)
    live = torch.arange(Tmax, device=dev)[None, :] < torch.tensor(frames, device=dev)[:, None]
    return (track * live[:, None, :, None]).contiguous()


def composition(fgd, track, live, span_scale):
    """fgd on the padded rectangle, then masked fp64 pairwise differences, one base take at a time -> distance [U, R, R], diversity [U]."""
    U, R, T, _ = track.shape
    feat = fgd(track)[1].double()                                       # [U, R, T, 512]
    rows = []
    for r in range(R):
        d = feat[:, r:r + 1] - feat                                     # [U, R, T, 512]
        s = (d * d).sum(dim=3)                                          # [U, R, T]
        rows.append(torch.where(live[:, None, :], s, torch.zeros((), dtype=s.dtype, device=s.device)).sum(dim=2))
    dist = torch.sqrt(torch.stack(rows, dim=1) * span_scale[:, None, None])
    div = dist.triu(1).sum(dim=(1, 2)) * (2.0 / (R * (R - 1)))
    return dist, div


class Eager:
    """The call itself with a graph's replay(): timed from the host side of the stream, launch overhead included."""
    def __init__(self, fn):
        self.fn = fn

    def replay(self):
        self.fn()


def bind_other(path):
    from emotiongestures_amd import _lib as L
    lib = C.CDLL(path)
    for name in ("eg_take_distance", "eg_take_distance_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--cases", default="u8_30s_r8,u8_60s_r8,ten_min_r32,ragged64_r4")
    ap.add_argument("--eager-case", default=None, help="run that case eagerly --eager-iters times and exit (for a rocprofv3 kernel trace)")
    ap.add_argument("--eager-iters", type=int, default=20)
    ap.add_argument("--ab-lib", default=None, help="a second build of libemogest_hip.so whose eg_take_distance is timed beside this one's")
    ap.add_argument("--no-composition", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd import harness as H
    from emotiongestures_amd import ops, takes
    from emotiongestures_amd.synth import load_synth_weights
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(64)
    cases = {"u8_30s_r8": ([30 * FPS] * 8, 8), "u8_60s_r8": ([60 * FPS] * 8, 8), "ten_min_r32": ([600 * FPS], 32),
             "ragged64_r4": ([int(v) * FPS // SR for v in rng.integers(10 * SR, 90 * SR, 64)], 4)}
    fgd = load_synth_weights(H.MLP_Reconstruct(pose_dim=D, precision="bf16x3"), 7).eval().to(dev)
    span = 60
    if a.eager_case:
        frames, R = cases[a.eager_case]
        track = make(frames, R, 1, dev)
        with torch.no_grad():
            for _ in range(a.eager_iters):
                out = takes.take_diversity(fgd, track, frames, span=span)
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "finite": int(torch.isfinite(out["diversity"]).sum())}))
        return

    other = bind_other(a.ab_lib) if a.ab_lib else None
    res = {"metric": "take_diversity", "unit": "device events; graphs replayed, eager calls issued from the host", "rounds": a.rounds,
           "window_s": a.window_s, "pose": "282 columns, 15 fps", "fgd_precision": fgd.precision, "span": span,
           "chunk_frames": 16, "device": torch.cuda.get_device_name(dev)}
    lib = L.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R = cases[name]
            U, sumf = len(frames), sum(frames)
            N = R * sumf
            track = make(frames, R, 20 + U, dev)
            live = torch.arange(max(frames), device=dev)[None, :] < torch.tensor(frames, device=dev)[:, None]
            scale = torch.tensor([span / f for f in frames], dtype=torch.float64, device=dev)
            ws = torch.empty(takes.workspace_bytes(frames, R), dtype=torch.uint8, device=dev)
            out = {"distance": torch.zeros(U, R, R, dtype=torch.float64, device=dev), "diversity": torch.zeros(U, dtype=torch.float64, device=dev)}
            call = lambda: takes.take_diversity(fgd, track, frames, span=span, workspace=ws, out=out)
            g_new, _ = graph_of(call)
            rows, _f, _o = takes.pack_rows(track, frames)
            feat, _f, _o = takes.track_features(fgd, track, frames)
            g_pack, _ = graph_of(lambda: takes.pack_rows(track, frames))

            def encoder():
                x = rows
                for i, lin in enumerate((fgd.Encoder[0], fgd.Encoder[2], fgd.Encoder[4])):
                    pk = rows.shape[1] - D if i == 0 else 0
                    x = ops.linear(x, fgd._cache.padded_weight(lin) if pk else lin.weight, lin.bias, precision=fgd.precision,
                                   packed=fgd._cache.get(lin, dev, pad_k=pk))
                return x
            g_feat, _ = graph_of(encoder)
            g_dist, _ = graph_of(lambda: takes.take_distance(feat, frames, R, span=span, workspace=ws, out=out))
            graphs = {"graph": g_new, "eager": Eager(call), "pack": g_pack, "features": g_feat, "distance": g_dist}
            entry = {"recordings": U, "draws": R, "frames": [min(frames), max(frames)], "rows": N,
                     "padded_rows": U * R * max(frames)}
            if not a.no_composition:
                g_old, (d_old, v_old) = graph_of(lambda: composition(fgd, track, live, scale), warmup=2)
                graphs["composition"] = g_old
                g_new.replay()
                torch.cuda.synchronize()
                entry["max_rel_diff_vs_composition"] = float(((out["diversity"] - v_old).abs() / v_old.abs()).max())
            if other is not None:
                fr = np.ascontiguousarray(frames, np.int32)
                meta = takes._TakesPlan.get(lib, frames, R, dev).meta
                o2 = {k: torch.zeros_like(v) for k, v in out.items()}

                def run_other():
                    rc = other.eg_take_distance(ptr(feat), U, R, K, C.c_void_p(fr.ctypes.data), ptr(meta), span, ptr(ws), ws.numel(),
                                                ptr(o2["distance"]), ptr(o2["diversity"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                    assert rc == 0, rc
                g_other, _ = graph_of(run_other)
                graphs["distance_other_lib"] = g_other
                g_dist.replay()
                g_other.replay()
                torch.cuda.synchronize()
                entry["other_lib_bitwise_equal"] = bool(torch.equal(out["distance"].view(torch.int64), o2["distance"].view(torch.int64)))
            t, reps = alternate(graphs, a.rounds, a.window_s)
            for k, v in t.items():
                entry[k] = summary(v)
            dist_s = statistics.median(t["distance"]) * 1e-3
            P = R * (R - 1) // 2
            algo, asked = N * K * 4, sumf * K * 4 * ((R - 1) + P)
            entry["distance_bytes"] = {"algorithmic": algo, "asked_by_loads": asked, "algorithmic_GBps": round(algo / dist_s / 1e9, 1),
                                       "asked_GBps": round(asked / dist_s / 1e9, 1)}
            entry["us_per_take"] = round(1000 * statistics.median(t["graph"]) / (U * R), 3)
            if "composition" in t:
                entry["composition_over_graph"] = round(statistics.median(t["composition"]) / statistics.median(t["graph"]), 2)
            if "distance_other_lib" in t:
                entry["other_lib_over_this"] = round(statistics.median(t["distance_other_lib"]) / statistics.median(t["distance"]), 3)
            entry["replays_per_window"] = reps["graph"]
            res[name] = entry
            del track, rows, feat, g_new, g_pack, g_feat, g_dist, graphs
            torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
