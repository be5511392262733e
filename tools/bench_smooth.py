#!/usr/bin/env python3
"""Smoothed output (smooth.smooth_tracks: eg_smooth_tracks; smooth.StreamSmoother: eg_smooth_stream_push) timed on whole tracks with the TED
geometry (126 columns, 30 new poses per 2 s window + 4) -- 8 recordings x 30 s x 8 takes, 1 x 10 min x 32 takes, 64 ragged recordings of
12-89 s x 4 takes, each at window 9 / polyorder 3 and at window 31 / polyorder 3 -- and on one stream step (30 poses per row, window 9) for
1, 8 and 64 rows.  One captured graph per contender, device events after warm-up, alternating rounds: every timed window is sized to at
least --window-s seconds of replays, --rounds windows per figure: median, min and max.

Beside every case:
  composition  the same definition from torch ops on the same GPU: a depthwise conv1d with the table's centre row for the interior, two small
               matmuls with the head and tail rows for the edges (the tail's frames gathered per row), a mask for ragged rows; for a stream
               step the conv1d over [history | chunk], the valid mask and the history copy;
  floor        a device copy that moves the same bytes: (bytes in + bytes out) / 2 read and written;
  host         what a user does today: copy the track to the host, scipy.signal.savgol_filter(mode="interp") in float64 per recording, copy
               the result back (host clock around all three).
The project's rule against the composition: the slowest window of the kernel beats the fastest window of the composition at every shape
("rule_holds").  The ratio to the floor is reported, not gated.
Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_smooth.py --eager-case ten_min_x32_k31

    python tools/bench_smooth.py [--rounds 5] [--window-s 0.4] [--out profiles/smooth_bench_line.json]
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
H, P, D = 30, 4, 126


def frames_of(seconds):
    return -(-int(seconds * 16000) // 32000) * H + P


def composition(x, table, n_dev):
    """x [B, T, D] (zero behind a row's end), table [K, K] fp32 on the device, n_dev int64 [B] -> [B, T, D]."""
    B, T, Dc = x.shape
    K = table.shape[0]
    half = K // 2
    y = torch.zeros_like(x)
    w = table[half].view(1, 1, K).expand(Dc, 1, K).contiguous()
    y[:, half:T - half] = torch.nn.functional.conv1d(x.transpose(1, 2), w, groups=Dc).transpose(1, 2)
    y[:, :half] = table[:half] @ x[:, :K]
    last = (n_dev[:, None] - K + torch.arange(K, device=x.device)[None, :])                              # [B, K]: the row's last K frames
    tail = table[half + 1:] @ torch.gather(x, 1, last[:, :, None].expand(B, K, Dc))                      # [B, half, D]
    y.scatter_(1, last[:, half + 1:, None].expand(B, half, Dc), tail)
    return y * (torch.arange(T, device=x.device)[None, :, None] < n_dev[:, None, None])


def step_composition(hist, chunk, table, valid, out):
    K = table.shape[0]
    w = table[K // 2].view(1, 1, K).expand(chunk.shape[2], 1, K).contiguous()
    y = torch.nn.functional.conv1d(torch.cat([hist, chunk], 1).transpose(1, 2), w, groups=chunk.shape[2]).transpose(1, 2)
    out.copy_(y * valid[:, None, None])
    hist.copy_(chunk[:, chunk.shape[1] - (K - 1):])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--cases", default="u8_30s_x8_k9,ten_min_x32_k9,ragged64_x4_k9,u8_30s_x8_k31,ten_min_x32_k31,ragged64_x4_k31,step_1,step_8,step_64")
    ap.add_argument("--eager-case", default=None, help="run that case eagerly --eager-iters times and exit (for a rocprofv3 kernel trace or counter pass)")
    ap.add_argument("--eager-iters", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import smooth as SM
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(64)
    ragged = [frames_of(s) for s in rng.uniform(12, 89, 64)]
    # name -> (frames per recording, takes, window, a stream step?)
    cases = {}
    for K in (9, 31):
        cases.update({f"u8_30s_x8_k{K}": ([frames_of(30)] * 8, 8, K, False), f"ten_min_x32_k{K}": ([frames_of(600)], 32, K, False),
                      f"ragged64_x4_k{K}": (ragged, 4, K, False)})
    cases.update({"step_1": ([H], 1, 9, True), "step_8": ([H] * 8, 1, 9, True), "step_64": ([H] * 64, 1, 9, True)})

    def make(frames, R):
        g = torch.Generator(device=dev).manual_seed(len(frames))
        x = torch.randn(len(frames) * R, max(frames), D, generator=g, device=dev)
        live = torch.arange(max(frames), device=dev)[None, :] < torch.tensor(frames, device=dev).repeat_interleave(R)[:, None]
        return (x * live[:, :, None]).contiguous()

    def setup(name):
        frames, R, K, step = cases[name]
        sm = SM.Smoother(K, 3)
        x = make(frames, R)
        if step:
            ss = SM.StreamSmoother(len(frames), H, D, sm, device=dev)
            valid = torch.ones(len(frames), dtype=torch.int32, device=dev)
            ss.run(x, valid)                                           # every timed step is a steady-state one
            return frames, R, sm, x, ss.out, (lambda: ss.run(x, valid)), 2
        d_frames = torch.tensor(frames, dtype=torch.int32, device=dev)
        out = torch.empty_like(x)
        return frames, R, sm, x, out, (lambda: SM.launch_smooth(x, sm, frames, d_frames, R, out=out)), 1

    if a.eager_case:
        _f, _R, _sm, _x, out, run, _n = setup(a.eager_case)
        for _ in range(a.eager_iters):
            run()
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "finite": bool(torch.isfinite(out).all())}))
        return

    res = {"metric": "smooth_tracks", "unit": "device events, graphs replayed; host: wall clock from the device tensor to the device result",
           "rounds": a.rounds, "window_s": a.window_s, "tile_frames": SM.TILE_FRAMES, "tile_cols": SM.TILE_COLS, "columns": D,
           "device": torch.cuda.get_device_name(dev)}
    holds = True
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R, sm, x, out, run, launches = setup(name)
            step = cases[name][3]
            table = sm.device_table(dev)
            g_new, _ = graph_of(run)
            if step:
                hist, valid_f, y_buf = torch.randn(len(frames), sm.window - 1, D, device=dev), torch.ones(len(frames), device=dev), torch.empty_like(x)
                g_old, y_old = graph_of(lambda: step_composition(hist, x, table, valid_f, y_buf), warmup=2)
                nbytes = 4 * (2 * x.numel() + 2 * hist.numel())
            else:
                n_dev = torch.tensor(frames, device=dev).repeat_interleave(R)
                g_old, y_old = graph_of(lambda: composition(x, table, n_dev), warmup=2)
                nbytes = 4 * 2 * R * sum(frames) * D
            buf = torch.empty(max(1, nbytes // 8), dtype=torch.float32, device=dev)
            dst = torch.empty_like(buf)
            g_floor, _ = graph_of(lambda: dst.copy_(buf))
            g_new.replay()
            torch.cuda.synchronize()
            entry = {"recordings": len(frames), "takes": R, "window": sm.window, "polyorder": sm.polyorder, "frames": [min(frames), max(frames)],
                     "frames_total": R * sum(frames), "bytes": nbytes, "launches": launches}
            if not step:
                entry["max_abs_diff_vs_composition"] = float((out - y_old).abs().max())
            t, reps = alternate({"graph": g_new, "composition": g_old, "floor": g_floor}, a.rounds, a.window_s)
            for k, v in t.items():
                entry[k] = summary(v)
            sec = statistics.median(t["graph"]) * 1e-3
            entry["GBps"] = round(nbytes / sec / 1e9, 1)
            entry["ns_per_frame"] = round(1e9 * sec / (R * sum(frames)), 4)
            entry["graph_over_floor"] = round(statistics.median(t["graph"]) / statistics.median(t["floor"]), 2)
            entry["composition_over_graph"] = round(statistics.median(t["composition"]) / statistics.median(t["graph"]), 2)
            entry["rule_holds"] = bool(max(t["graph"]) < min(t["composition"]))
            holds &= entry["rule_holds"]
            if not a.no_host and not step:
                from scipy.signal import savgol_filter
                host = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    xs = x.cpu().numpy().astype(np.float64).reshape(len(frames), R, x.shape[1], D)
                    y = np.zeros_like(xs)
                    for u, n in enumerate(frames):
                        y[u, :, :n] = savgol_filter(xs[u, :, :n], sm.window, sm.polyorder, axis=1, mode="interp")
                    back = torch.from_numpy(y.astype(np.float32)).to(dev)
                    torch.cuda.synchronize()
                    host.append((time.perf_counter() - t0) * 1e3)
                entry["host_copy_plus_scipy"] = summary(host)
                entry["host_over_graph"] = round(statistics.median(host) / statistics.median(t["graph"]), 1)
                entry["max_abs_diff_vs_host"] = float((out - back.view_as(out)).abs().max())
            entry["replays_per_window"] = reps["graph"]
            res[name] = entry
            del x, out, buf, dst, g_new, g_old, g_floor, y_old
            torch.cuda.empty_cache()
    res["rule_holds_everywhere"] = holds
    write_line(res, a.out)


if __name__ == "__main__":
    main()
