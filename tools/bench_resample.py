#!/usr/bin/env python3
"""The polyphase resampler (resample.resample_audio / resample.StreamResampler: eg_resample, eg_resample_stream_push) timed on whole
recordings -- 8 x 30 s at 48 kHz, 8 x 60 s at 44.1 kHz, 1 x 10 min at 48 kHz, 64 recordings of 12-89 s at 44.1 kHz (the ragged set of
bench_take_diversity.py) -- and on one stream push for 1, 8 and 64 rows at 48 kHz; one captured graph each.  Device events after warm-up,
every timed window sized to at least --window-s seconds of replays, --rounds windows per figure: median, min and max.

Beside every case:
  host         what a user does without it: scipy.signal.resample_poly in float32 on the host, row by row, plus the copy to the device
               (host clock around work that ends in a device synchronise);
  composition  torch on the same GPU: conv1d with stride M when L = 1, one strided conv1d per phase otherwise (on the padded rectangle);
  floor        a device copy that moves the same bytes: (bytes in + bytes out) / 2 read and written.
Outputs are compared with both baselines (maximum absolute difference).
Kernel statistics, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bench_resample.py --eager-case ten_min_48k

    python tools/bench_resample.py [--rounds 5] [--window-s 0.4] [--out profiles/resample_bench_line.json]
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
SR = 16000


def composition(x, plan, bank, n_out):
    """x [U, T] zero beyond every row's end -> [U, n_out] by torch convolutions: bank [L, pitch] fp32 on the device."""
    import torch.nn.functional as F
    Lf, M, half, K = plan["L"], plan["M"], plan["half"], plan["K"]
    U, T = x.shape
    xp = F.pad(x, (K - 1, K + M))[:, None]                              # index i of x is K - 1 + i here
    y = torch.empty(U, n_out, device=x.device)
    for r in range(min(Lf, n_out)):
        p = half + r * M
        i_r, ph = p // Lf, p % Lf
        w = bank[ph, :K].flip(0)[None, None]                            # y[q*L + r] = sum_t xp[i_r + q*M + t] * w[t]
        n_r = -(-(n_out - r) // Lf)
        span = (n_r - 1) * M + K
        seg = xp[:, :, i_r:i_r + span]
        if seg.shape[2] < span:
            seg = F.pad(seg, (0, span - seg.shape[2]))
        y[:, r::Lf] = F.conv1d(seg, w, stride=M)[:, 0, :n_r]
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.4)
    ap.add_argument("--cases", default="u8_30s_48k,u8_60s_44k1,ten_min_48k,ragged64_44k1,push_1_48k,push_8_48k,push_64_48k")
    ap.add_argument("--eager-case", default=None, help="run that case eagerly --eager-iters times and exit (for a rocprofv3 kernel trace)")
    ap.add_argument("--eager-iters", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-composition", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import resample as RS
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(64)
    ragged = [int(v) * 441 // 160 for v in rng.integers(12 * SR, 89 * SR, 64)]
    cases = {"u8_30s_48k": (48000, [30 * 48000] * 8), "u8_60s_44k1": (44100, [60 * 44100] * 8), "ten_min_48k": (48000, [600 * 48000]),
             "ragged64_44k1": (44100, ragged), "push_1_48k": (48000, 1), "push_8_48k": (48000, 8), "push_64_48k": (48000, 64)}
    hop = 53333                                                         # the BEAT default: 50 poses at 15 fps

    def make(rate, lens):
        g = torch.Generator(device=dev).manual_seed(len(lens))
        x = torch.randn(len(lens), max(lens), generator=g, device=dev)
        live = torch.arange(max(lens), device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None]
        return (x * live).contiguous()

    if a.eager_case:
        rate, lens = cases[a.eager_case]
        if isinstance(lens, int):
            s = RS.StreamResampler(lens, rate, hop, device=dev)
            s.chunk.normal_()
            for _ in range(a.eager_iters):
                out = s.run()
        else:
            x = make(rate, lens)
            for _ in range(a.eager_iters):
                out = RS.resample_audio(x, rate, lengths=lens)
        torch.cuda.synchronize()
        print(json.dumps({"eager_case": a.eager_case, "iters": a.eager_iters, "finite": bool(torch.isfinite(out).all())}))
        return

    res = {"metric": "resample", "unit": "device events, graphs replayed; host: wall clock to a device synchronise", "rounds": a.rounds,
           "window_s": a.window_s, "tile": RS.TILE, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        for name in a.cases.split(","):
            rate, lens = cases[name]
            plan = RS.plan(rate)
            if isinstance(lens, int):                                   # one stream push
                s = RS.StreamResampler(lens, rate, hop, device=dev)
                s.chunk.normal_()
                g_new, _ = graph_of(s.run)
                nbytes = 4 * lens * (s.hop_in + hop + 2 * plan["Hs"])
                buf = torch.empty(max(1, nbytes // 8), dtype=torch.float32, device=dev)
                dst = torch.empty_like(buf)
                g_floor, _ = graph_of(lambda: dst.copy_(buf))
                t, reps = alternate({"graph": g_new, "floor": g_floor}, a.rounds, a.window_s)
                entry = {"rows": lens, "rate_in": rate, "hop_out": hop, "hop_in": s.hop_in, "launches": 2, "bytes": nbytes}
                for k, v in t.items():
                    entry[k] = summary(v)
                res[name] = entry
                continue
            U, n_out = len(lens), [RS.out_length(n, rate) for n in lens]
            x = make(rate, lens)
            out = torch.empty(U, max(n_out), device=dev)
            g_new, _ = graph_of(lambda: RS.resample_audio(x, rate, lengths=lens, out=out))
            nbytes = 4 * (sum(lens) + U * max(n_out))
            buf = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
            dst = torch.empty_like(buf)
            g_floor, _ = graph_of(lambda: dst.copy_(buf))
            graphs = {"graph": g_new, "floor": g_floor}
            entry = {"recordings": U, "rate_in": rate, "L": plan["L"], "M": plan["M"], "taps_per_output": plan["K"],
                     "seconds": [round(min(lens) / rate, 1), round(max(lens) / rate, 1)], "samples_in": sum(lens), "samples_out": sum(n_out),
                     "bytes": nbytes}
            if not a.no_composition:
                bank = RS._Bank.get(rate, SR, dev).bank.view(plan["L"], plan["pitch"])
                g_old, y_old = graph_of(lambda: composition(x, plan, bank, max(n_out)), warmup=2)
                graphs["composition"] = g_old
                g_new.replay()
                torch.cuda.synchronize()
                entry["max_abs_diff_vs_composition"] = max(float((out[u, :n] - y_old[u, :n]).abs().max()) for u, n in enumerate(n_out))
            t, reps = alternate(graphs, a.rounds, a.window_s)
            for k, v in t.items():
                entry[k] = summary(v)
            sec = statistics.median(t["graph"]) * 1e-3
            entry["GBps"] = round(nbytes / sec / 1e9, 1)
            entry["ns_per_output"] = round(1e9 * sec / sum(n_out), 4)
            entry["GFLOPs"] = round(2.0 * plan["K"] * sum(n_out) / sec / 1e9, 1)
            entry["graph_over_floor"] = round(statistics.median(t["graph"]) / statistics.median(t["floor"]), 2)
            if "composition" in t:
                entry["composition_over_graph"] = round(statistics.median(t["composition"]) / statistics.median(t["graph"]), 2)
            if not a.no_host:
                from scipy.signal import resample_poly
                xh = x.cpu().numpy()
                torch.cuda.synchronize()
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    rows = [resample_poly(xh[u, :n], plan["L"], plan["M"]).astype(np.float32, copy=False) for u, n in enumerate(lens)]
                    ys = [torch.from_numpy(r).to(dev) for r in rows]
                    torch.cuda.synchronize()
                    host.append((time.perf_counter() - t0) * 1e3)
                entry["host_scipy_plus_copy"] = summary(host)
                entry["host_over_graph"] = round(statistics.median(host) / statistics.median(t["graph"]), 1)
                g_new.replay()
                torch.cuda.synchronize()
                entry["max_abs_diff_vs_host"] = max(float((out[u, :n] - ys[u][:n]).abs().max()) for u, n in enumerate(n_out))
            entry["replays_per_window"] = reps["graph"]
            res[name] = entry
            del x, out, buf, dst, graphs, g_new, g_floor
            torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
