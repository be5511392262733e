"""What the bench tools share: graph capture, timed windows of replays between device events, alternating rounds, the result line."""
import json
import statistics

import torch


def graph_of(fn, warmup=3):
    """`fn` warmed up, then captured: (graph, the captured call's result)."""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, out


def capture(fn, lib):
    """`fn` warmed up on a side stream, then captured: (graph, result, the library's own launches inside the graph)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    n0 = lib.eg_launch_count()
    with torch.cuda.graph(graph), torch.no_grad():
        out = fn()
    return graph, out, lib.eg_launch_count() - n0


def window_ms(g, n):
    """ms per replay over one window of n replays between two device events; `g`: anything with replay(), or the replay callable itself."""
    replay = getattr(g, "replay", g)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(graphs, rounds, window_s, min_reps=5, probe=3):
    """{name: graph} -> ({name: per-round ms}, {name: replays per window}); every round times each graph once, in turn.  A window holds at
    least `window_s` seconds of replays (sized from a probe of `probe` replays) and at least `min_reps` of them."""
    reps = {k: max(min_reps, int(window_s * 1000.0 / max(window_ms(g, probe), 1e-3)) + 1) for k, g in graphs.items()}
    res = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            res[k].append(window_ms(g, reps[k]))
    return res, reps


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def write_line(res, out=None):
    """Print the result as one JSON line; with `out` also write it to that file."""
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
