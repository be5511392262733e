#!/usr/bin/env python3
"""Emotion recognition of whole tracks (emotion.emotion_of_tracks: eg_track_rows_pack, the per-pose embedding, eg_emotion_window_embed, the
classifier's encoder and head per range of clips, eg_emotion_vote) timed on bench_take_diversity.py's four shapes -- 8 recordings x 30 s x
8 takes, 8 x 60 s x 8, 1 x 10 min x 32 takes, 64 ragged recordings of 10-90 s x 4 takes, 282-column poses at 15 fps -- with the
reference-size classifier (d_model 512, d_inner 2048, 3 layers, 8 heads, F = 60), at stride F and F / 4.

Beside the call:
  composition  the same definition from torch ops on the same GPU: ``unfold`` the windows of every recording (plus the tail window),
               ``classifier(windows)`` in the same ranges of clips, ``argmax`` / masked ``index_add_`` sums per take, the tie-broken ``pred``;
  parts        the call's own stages alone: the logits (``window_logits``), the encoder layers and head on ready encoder inputs (the
               "encoder products"), the embed launches, the votes (one captured graph).
``window_logits`` allocates per range, so neither contender is captured: both are timed eagerly from the host side of the stream, launch
overhead included, in alternating rounds of windows of at least --window-s seconds; median, min and max of --rounds windows.  Whatever
is measured is written down; no ratio is fixed in advance.

    python tools/bench_emotion.py [--rounds 5] [--window-s 0.3] [--out profiles/emotion_bench_line.json]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import alternate, graph_of, summary, write_line  # noqa: E402
SR, FPS, D, F, C = 16000, 15, 282, 60, 8


def make(frames, R, seed, dev):
    """Cumulative-sum poses [U, R, Tmax, 282] made on the device, zero beyond frames[u] (what the ragged roll-out leaves there)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    U, Tmax = len(frames), max(frames)
    track = torch.cumsum(torch.randn(U, R, Tmax, D, generator=g, device=dev) * 0.05, dim=2)
    live = torch.arange(Tmax, device=dev)[None, :] < torch.tensor(frames, device=dev)[:, None]
    return (track * live[:, None, :, None]).contiguous()


def composition(skel, track, frames, labels, S, chunk):
    """The definition from torch ops: -> (logits [N, C], votes [U*R, C], mean [U*R, C], pred [U*R], accuracy)."""
    U, R = track.shape[:2]
    wins, take = [], []
    for u, f in enumerate(frames):
        w = track[u, :, :f].unfold(1, F, S).permute(0, 1, 3, 2)            # [R, n, F, D]
        if (f - F) % S:
            w = torch.cat([w, track[u, :, None, f - F:f]], 1)
        wins.append(w.reshape(-1, F, D))
        take.append((u * R + torch.arange(R, device=track.device)).repeat_interleave(w.shape[1]))
    wins, take = torch.cat(wins), torch.cat(take)
    logits = torch.cat([skel(wins[c:c + chunk].contiguous())[0] for c in range(0, wins.shape[0], chunk)])
    valid = torch.isfinite(logits).all(1)
    cls = logits.argmax(1)
    votes = torch.zeros(U * R, C, dtype=torch.int32, device=track.device).index_put_((take[valid], cls[valid]), torch.ones((), dtype=torch.int32, device=track.device), accumulate=True)
    sums = torch.zeros(U * R, C, dtype=torch.float64, device=track.device).index_add_(0, take[valid], logits[valid].double())
    mean = sums / votes.sum(1, keepdim=True).double()
    key = votes.double() * 1e12 + mean.nan_to_num(0.0)                      # most votes, then the larger mean (argmax: the lowest index among equals)
    pred = torch.where(votes.sum(1) > 0, key.argmax(1), -1)
    acc = 100.0 * (pred == labels.reshape(-1)).double().sum() / (U * R)
    return logits, votes, mean, pred, acc


class Eager:
    """The call itself with a graph's replay(): timed from the host side of the stream, launch overhead included."""
    def __init__(self, fn):
        self.fn = fn

    def replay(self):
        self.fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--cases", default="u8_30s_r8,u8_60s_r8,ten_min_r32,ragged64_r4")
    ap.add_argument("--strides", default="60,15")
    ap.add_argument("--chunk-clips", type=int, default=1024)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd import emotion as EM
    from emotiongestures_amd import harness as H
    from emotiongestures_amd.synth import load_synth_weights
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(64)
    cases = {"u8_30s_r8": ([30 * FPS] * 8, 8), "u8_60s_r8": ([60 * FPS] * 8, 8), "ten_min_r32": ([600 * FPS], 32),
             "ragged64_r4": ([int(v) * FPS // SR for v in rng.integers(10 * SR, 90 * SR, 64)], 4)}
    skel = load_synth_weights(H.SkeletonTransformer(class_dim=C, pose_dim=D, d_word_vec=512, d_model=512, d_inner=2048, n_layers=3, n_head=8,
                                                    d_k=64, d_v=64, n_position=F, precision=a.precision), 7).eval().to(dev)
    head = [skel.post_projector[i] for i in (0, 2, 4, 6, 8)]
    lib = L.load()
    res = {"metric": "emotion_of_tracks", "unit": "ms per call, eager, device events around windows of calls", "rounds": a.rounds,
           "window_s": a.window_s, "chunk_clips": a.chunk_clips, "precision": a.precision, "classifier": "d_model 512, d_inner 2048, 3 layers, F 60",
           "device": torch.cuda.get_device_name(dev)}
    med = statistics.median
    with torch.no_grad():
        for name in a.cases.split(","):
            frames, R = cases[name]
            U = len(frames)
            track = make(frames, R, 1, dev)
            labels = torch.randint(0, C, (U, R), generator=torch.Generator().manual_seed(U)).to(dev).to(torch.int32)
            for S in (int(s) for s in a.strides.split(",")):
                plan = EM.window_plan(frames, F, S)
                N = R * plan.total
                ours = lambda: EM.emotion_of_tracks(skel, track, frames, labels, stride=S, chunk_clips=a.chunk_clips)
                theirs = lambda: composition(skel, track, frames, labels, S, a.chunk_clips)
                got, want = ours(), theirs()
                torch.cuda.synchronize()
                logits = got["logits"]
                xs = [torch.randn(min(a.chunk_clips, N - c), F, 512, device=dev) for c in range(0, N, a.chunk_clips)][:2]
                nx = -(-N // a.chunk_clips)

                def encoder():                                              # the encoder products of one call: nx ranges (the first and the last shape)
                    for i in range(nx):
                        x = xs[0] if i < nx - 1 or len(xs) == 1 else xs[1]
                        H._affine_chain(skel._cache, EM._encoder_layers(skel, x).reshape(x.shape[0], -1), head, True, skel.precision)
                if N % a.chunk_clips and nx > 1:
                    xs[1] = torch.randn(N % a.chunk_clips, F, 512, device=dev)
                emb = torch.randn(R * plan.sum_frames, 512, device=dev)
                pos = torch.randn(F, 512, device=dev)
                xbuf = torch.empty(min(a.chunk_clips, N) * F, 512, device=dev)
                st = torch.cuda.current_stream(dev).cuda_stream

                def embed():
                    for c0 in range(0, N, a.chunk_clips):
                        L.check(lib.eg_emotion_window_embed(emb.data_ptr(), pos.data_ptr(), U, R, F, S, 1, 512, plan.h_frames, plan.table(dev).data_ptr(),
                                                            c0, min(N, c0 + a.chunk_clips), xbuf.data_ptr(), st), "eg_emotion_window_embed")
                ws = torch.empty(EM.vote_workspace_bytes(plan, R, C), dtype=torch.uint8, device=dev)
                out = EM.emotion_votes(logits, plan, R, labels)
                g_votes, _ = graph_of(lambda: EM.emotion_votes(logits, plan, R, labels, workspace=ws, out=out))
                t, reps = alternate({"call": Eager(ours), "composition": Eager(theirs), "logits": Eager(lambda: EM.window_logits(skel, track, frames, stride=S, chunk_clips=a.chunk_clips)),
                                     "encoder": Eager(encoder), "embed": Eager(embed), "votes": g_votes}, a.rounds, a.window_s, min_reps=2)
                entry = {"recordings": U, "takes": R, "frames": [min(frames), max(frames)], "stride": S, "windows": N, "pose_rows": R * plan.sum_frames,
                         "ranges": nx, "pred_equal_composition": bool(torch.equal(got["pred"].reshape(-1).long(), want[3].long())),
                         "votes_equal_composition": bool(torch.equal(got["votes"].reshape(-1, C), want[1])),
                         "logits_rel_l2_vs_composition": float((logits - want[0]).norm() / want[0].norm()),
                         "accuracy": float(got["accuracy"]), "replays_per_window": reps}
                for k, v in t.items():
                    entry[k] = summary(v)
                entry["composition_over_call"] = round(med(t["composition"]) / med(t["call"]), 3)
                entry["encoder_share_of_call"] = round(med(t["encoder"]) / med(t["call"]), 3)
                entry["embed_share_of_call"] = round(med(t["embed"]) / med(t["call"]), 4)
                entry["votes_share_of_call"] = round(med(t["votes"]) / med(t["call"]), 4)
                res[f"{name}_s{S}"] = entry
                del got, want, logits, xs, emb, xbuf, ws, out, g_votes
                torch.cuda.empty_cache()
            del track
            torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
