#!/usr/bin/env python3
"""Streaming synthesis walk-through on synthetic data: the recordings of tools/demo_synthesize.py fed hop by hop (2 s of audio per push) through
one GestureStream, one row leaving and rejoining with a second recording while the others go on:

  push(audio [U, 32 000]) --eg_stream_push (ring + window clips)--> extract_melspectrogram --> MLP_Reconstruct_v3.sample -->
  eg_generator_stream_step (the generator at batch U seeded from the device-resident prior, then the hand-off) --> 30 finished poses per row,

all of it ONE captured hipGraph replayed per push.  Every row's emitted rows followed by its tail are checked to EQUAL the track
harness.synthesize gives for the same recording.  Weights are synthetic (integer hash), so the poses carry no meaning.
With --audio-rate HZ the recordings are made at that rate and the stream is opened with audio_rate=HZ: every push carries hop * M / L samples,
a StreamResampler runs first inside the same graph, and the rows equal synthesize on resample_audio(recording, HZ, delay=stream_delay(HZ)).
With --joints the stream is opened with joints=skeleton.ted_expressive(): one more launch inside the graph leaves the joint positions of the
rows just emitted in stream.last_joints [U, 30, 43, 3]; the script prints their shape and the wrist extent in metres per push.
With --rotations (and --joints) the stream also gets rotations=rest, the rest pose taken from the normalised first generated frame of row 0 (one
window of synthesize beforehand): another launch inside the graph leaves the local bone rotations of the rows just emitted in
stream.last_rotations [U, 30, 42, 4]; the script prints the largest elbow swing in degrees per push.
With --smooth K P (not with --joints) the stream is opened with smooth=(K, P): two more launches inside the graph leave in stream.last_smooth
[U, 30, 126] the Savitzky-Golay-smoothed frames of every row, K // 2 frames behind the rows just emitted; the script prints the frame-to-frame
step of the raw and the smoothed rows per push, and every row's smoothed rows followed by tail_smooth() are checked to EQUAL
smooth.smooth_tracks on its finished track.
With --beat the generator is BEAT-shaped (60 poses of 282 columns, 10 of them the prior; 50 poses per push).  With --beat --joints the body is a
skeleton.JointTree -- the BEAT columns are one 6-D rotation per joint -- read from the HIERARCHY block of --bvh FILE (47 joints), or a
synthetic 47-joint upper body without --bvh: ONE more launch inside the graph leaves stream.last_joints [U, 50, 47, 3] and, with --rotations,
stream.last_rotations [U, 50, 47, 4] (local joint rotations; there is no rest pose); the script prints how far the deepest joint travels and the
largest rotation angle per push.
With --euler (and --beat --joints) the stream also gets euler= -- the channel orders of --bvh FILE, or ZXY for every joint -- and one more launch
inside the graph leaves the BVH rotation channels of the rows just emitted in stream.last_euler [U, 50, 47, 3] (degrees, principal values: the
Euler filter runs on a finished track, skeleton.unwrap_angles); the script prints the largest angle per push.
With --render-fps N (TED body; optionally --smooth K P and --rotations, which then belong to the stage) the stream is opened with
render=dict(joints=ted_expressive(), unit=True, fps=(15, N), smooth=(K, P), rotations=rest) beside the raw joints= stage: the delayed output
stage leaves in stream.last_render the smoothed joints (and rotations) at N frames per second, stream.render_delay source frames behind the rows
just emitted; the script prints that delay in frames and milliseconds and the wrists' frame-to-frame step in metres per second before (raw joints
at 15 fps) and after.
usage: demo_stream.py [rows=4] [seconds=20] [--beat] [--audio-rate HZ] [--joints [--bvh FILE] [--rotations] [--euler]] [--smooth K P]
                      [--render-fps N [--smooth K P] [--rotations]]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from emotiongestures_amd import harness as H
from emotiongestures_amd.builders import build_mirror
from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
from emotiongestures_amd.synth import load_synth_weights, synth_audio

from emotiongestures_amd import resample as R_

RATE = 16000
if "--audio-rate" in sys.argv:
    i = sys.argv.index("--audio-rate")
    RATE = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
AR = {"audio_rate": RATE} if RATE != 16000 else {}
BEAT = "--beat" in sys.argv
if BEAT:
    sys.argv.remove("--beat")
BVH = None
if "--bvh" in sys.argv:
    i = sys.argv.index("--bvh")
    BVH = sys.argv[i + 1]
    del sys.argv[i:i + 2]
RENDER_FPS = None
if "--render-fps" in sys.argv:
    i = sys.argv.index("--render-fps")
    RENDER_FPS = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    if BEAT:
        sys.exit("--render-fps: this demo renders the TED body (drop --beat)")
    if "--joints" not in sys.argv:
        sys.argv.append("--joints")                      # the raw joints= stage stays beside it: the figure "before"
JOINTS, JK, TREE = "--joints" in sys.argv, {}, None
if BVH and not (BEAT and JOINTS):
    sys.exit("--bvh needs --beat --joints (a BVH hierarchy is the body of the BEAT generators' 6-D joint rotations)")
if JOINTS and BEAT:
    import emotiongestures_amd.skeleton as SK_
    from tools.bench_articulate import synthetic_tree
    sys.argv.remove("--joints")
    TREE = SK_.JointTree.from_bvh(open(BVH).read()) if BVH else synthetic_tree(SK_)
    JK = dict(joints=TREE)
    if "--euler" in sys.argv:
        from emotiongestures_amd import bvh as BVH_
        sys.argv.remove("--euler")
        JK["euler"] = BVH_.read(BVH) if BVH else "ZXY"
elif JOINTS:
    from emotiongestures_amd.skeleton import ted_expressive
    sys.argv.remove("--joints")
    JK = dict(joints=ted_expressive(), joints_unit=True)
if "--euler" in sys.argv:
    sys.exit("--euler needs --beat --joints (Euler channels are the rotations of a JointTree's joints)")
ROTATIONS = "--rotations" in sys.argv
if ROTATIONS:
    sys.argv.remove("--rotations")
    if not JOINTS:
        sys.exit("--rotations needs --joints (the rest pose belongs to the skeleton's bones)")
SMOOTH = None
if "--smooth" in sys.argv:
    i = sys.argv.index("--smooth")
    SMOOTH = (int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    del sys.argv[i:i + 3]
    if JOINTS and RENDER_FPS is None:
        sys.exit("--smooth is not combined with --joints in a stream (the smoothed rows run half a window behind; smooth the finished track with "
                 "demo_synthesize.py --smooth K P --joints)")
    if RENDER_FPS is None:
        JK["smooth"] = SMOOTH
U = int(sys.argv[1]) if len(sys.argv) > 1 else 4
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 20.0
dev = torch.device("cuda:0")
FRAMES, POSE_DIM, PRIOR, FPS = (60, 282, 10, 15) if BEAT else (34, 126, 4, 15)
total = int(seconds * RATE)                              # samples per recording at the caller's rate
to16 = lambda n: R_.out_length(n, RATE) if AR else n

gen = build_mirror("spatial", FRAMES, POSE_DIM, PRIOR, PRIOR, seed=7, precision="bf16x3").to(dev)
vae = load_synth_weights(MLP_Reconstruct_v3(frames=FRAMES), 7).eval().to(dev)
audio = torch.from_numpy(synth_audio(U, total, seed=90)).to(dev)
if ROTATIONS and TREE is not None:                       # a joint tree has no rest pose: its offsets are the bind pose
    JK["rotations"] = True
elif ROTATIONS:                                          # the rest pose: the first generated frame of row 0's first window
    first = H.synthesize((gen, vae), audio[:1], torch.zeros(1, 1, 60, dtype=torch.int64, device=dev), torch.zeros(1, PRIOR, POSE_DIM, device=dev),
                         labels=torch.nn.functional.one_hot(torch.zeros(1, dtype=torch.int64), 8).float().to(dev), z=torch.zeros(1, 1, 32), **AR)
    JK["rotations"] = first["track"][0, PRIOR].reshape(-1, 3).cpu()
if RENDER_FPS is not None:                               # the delayed stage takes the filter and the rest pose; the raw stage keeps its joints
    JK["render"] = dict(joints=JK["joints"], unit=True, fps=(FPS, RENDER_FPS), smooth=SMOOTH, rotations=JK.get("rotations"))
    SMOOTH = None                                        # nothing below reads last_smooth: the stream has no smooth= of its own
stream = H.open_stream((gen, vae), U, torch.zeros(U, PRIOR, POSE_DIM, device=dev), **AR, **JK)
if RENDER_FPS is not None:
    print(f"render: {stream.render_frames} frames per push at {RENDER_FPS} fps, render_delay {stream.render_delay} frames = "
          f"{1e3 * stream.render_delay / FPS:.0f} ms behind the rows just emitted (the first {stream.render_lead} entries of a row's first step are zeros)")
hop, hop16 = stream.hop_in, stream.hop                    # samples per push at the caller's rate and at 16 kHz
W = (to16(total) - 1) // hop16 + 1                               # windows per recording = pushes that carry its audio
short = total // 2                                       # the leaving row's first recording; its second one has `short` samples too
W_short = (to16(short) - 1) // hop16 + 1
leaver = U - 1

second = torch.from_numpy(synth_audio(1, short, seed=91)).to(dev)[0]
labels = torch.nn.functional.one_hot(torch.arange(U) % 8, 8).float().to(dev)
text = torch.zeros(U, 60, dtype=torch.int64, device=dev)
steps = W + stream.lag - 1                               # the last window comes out lag - 1 pushes after the last audio
z = torch.randn(steps, U, 32)
seed2 = torch.full((U, PRIOR, POSE_DIM), 0.1, device=dev)

# the leaving row: first recording in pushes [1, W_short], reset, second recording from push `rejoin` on
rejoin = W_short + stream.lag
feeds = {u: [(1, audio[u], total)] for u in range(U)}
feeds[leaver] = [(1, audio[leaver, :short], short), (rejoin, second, short)]
tracks = {u: [[] for _ in feeds[u]] for u in range(U)}
zs = {u: [[] for _ in feeds[u]] for u in range(U)}
smooths = {u: [[] for _ in feeds[u]] for u in range(U)}
tails, tails_smooth = {}, {}
t_steps = []
for k in range(1, steps + 1):
    if k == rejoin:
        tails[(leaver, 0)] = stream.tail()[leaver].clone()
        if SMOOTH:
            tails_smooth[(leaver, 0)] = stream.tail_smooth()[leaver].clone()
        stream.reset(rows=[leaver], seed_pose=seed2)
    chunk, ends, which = torch.zeros(U, hop, device=dev), [-1] * U, [0] * U
    for u in range(U):
        which[u] = max(i for i, (start, _a, _t) in enumerate(feeds[u]) if start <= k)
        start, a, T = feeds[u][which[u]]
        lo = (k - start) * hop
        if lo < T:
            part = a[lo: lo + hop]
            chunk[u, : len(part)] = part
            if lo + hop >= T:
                ends[u] = T - lo
    t0 = time.perf_counter()
    rows, valid = stream.push(chunk, text, labels, z[k - 1], ends=ends)
    torch.cuda.synchronize()
    t_steps.append(time.perf_counter() - t0)
    for u in range(U):
        if stream.last_valid[u]:
            tracks[u][which[u]].append(rows[u])
            zs[u][which[u]].append(z[k - 1, u])
            if SMOOTH:
                smooths[u][which[u]].append(stream.last_smooth[u])
    print(f"push {k:2d}: valid {valid.cpu().tolist()}  windows {stream.last_windows}  {1e3 * t_steps[-1]:.2f} ms")
    if TREE is not None and stream.last_joints is not None:
        j, deep = stream.last_joints, int(TREE.depth.argmax())
        print(f"         last_joints {tuple(j.shape)}: extent of joint {deep} ({int(TREE.depth[deep])} joints from the root) "
              f"{float((j[:, :, deep].amax(1) - j[:, :, deep].amin(1)).norm(dim=1).max()):.3f} m")
        if ROTATIONS:
            q = stream.last_rotations[valid.bool()]             # a row that was not valid holds zeros, not rotations
            print(f"         last_rotations {tuple(q.shape)}: largest local rotation "
                  f"{float(torch.rad2deg(2 * torch.acos(q[..., 0].clamp(max=1.0))).max()):.1f} degrees")
        if stream.last_euler is not None:
            e = stream.last_euler
            print(f"         last_euler {tuple(e.shape)}: largest channel {float(e.abs().max()):.1f} degrees, middle angles within "
                  f"{float(e[..., 1].abs().max()):.1f}")
    elif JOINTS and stream.last_joints is not None:
        j = stream.last_joints
        ext = [float((j[:, :, w].amax(1) - j[:, :, w].amin(1)).norm(dim=1).max()) for w in (6, 7)]
        print(f"         last_joints {tuple(j.shape)}: wrist extent left {ext[0]:.3f} m, right {ext[1]:.3f} m")
    if RENDER_FPS is not None and stream.last_render is not None:
        live = valid.bool() & torch.tensor([len(tracks[u][which[u]]) > 1 for u in range(U)], device=dev)        # past the first step's leading zeros
        if bool(live.any()):
            speed = lambda j, rate: float((j[live][:, 1:, 6:8] - j[live][:, :-1, 6:8]).norm(dim=3).mean()) * rate
            r = stream.last_render
            print(f"         last_render {({n: tuple(t.shape) for n, t in r.items()})}: wrists' frame-to-frame step "
                  f"{speed(stream.last_joints, FPS):.3f} m/s raw at {FPS} fps, {speed(r['joints'], RENDER_FPS):.3f} m/s rendered at {RENDER_FPS} fps")
    if ROTATIONS and TREE is None and stream.last_rotations is not None:
        q = stream.last_rotations[valid.bool()]             # a row that was not valid holds zeros, not rotations
        deg = [float(torch.rad2deg(2 * torch.acos(q[:, :, b, 0].clamp(max=1.0))).max()) for b in (4, 21)]      # the forearm bones
        print(f"         last_rotations {tuple(q.shape)}: largest elbow swing left {deg[0]:.1f} degrees, right {deg[1]:.1f} degrees")
    if SMOOTH and stream.last_smooth is not None:
        live = valid.bool() & torch.tensor([len(smooths[u][which[u]]) > 1 for u in range(U)], device=dev)     # past step 0's leading zeros
        if bool(live.any()):
            d = lambda t: float((t[live][:, 1:] - t[live][:, :-1]).norm(dim=2).mean())
            print(f"         last_smooth {tuple(stream.last_smooth.shape)}, {stream.smooth_delay} frames behind: mean |pose[t+1] - pose[t]| "
                  f"{d(rows):.4f} raw, {d(stream.last_smooth):.4f} smoothed")
final = stream.tail()
final_smooth = stream.tail_smooth() if SMOOTH else None

ok = True
for u in range(U):
    for i, (_start, a, T) in enumerate(feeds[u]):
        n_win = len(tracks[u][i])
        if n_win == 0:
            continue
        tail = tails.get((u, i), final[u])
        got = torch.cat(tracks[u][i] + [tail], 0)
        # synthesize on a batch of two recordings of this length (chunk invariance is stated from two clips up): this one and a copy
        seedp = (seed2 if i == 1 else torch.zeros_like(seed2))[u]
        zz = torch.stack(zs[u][i])[None].expand(2, n_win, 32).contiguous()
        a16 = R_.resample_audio(a[:T].contiguous(), RATE, delay=R_.stream_delay(RATE)) if AR else a[:T]
        want = H.synthesize((gen, vae), torch.stack([a16, a16]), text[u][None, None].expand(2, n_win, 60).contiguous(), torch.stack([seedp, seedp]),
                            labels=labels[u][None].expand(2, 8).contiguous(), z=zz, windows=n_win, mel=stream.mel)["track"][0]
        same = torch.equal(got, want)
        ok &= same
        print(f"row {u} recording {i}: {T / RATE:.1f} s -> {n_win} windows -> track {tuple(got.shape)}; equals harness.synthesize: {same}")
        if SMOOTH:
            from emotiongestures_amd.smooth import smooth_tracks
            sm_got = torch.cat([torch.cat(smooths[u][i], 0)[stream.smooth_delay:], tails_smooth.get((u, i), final_smooth[u])], 0)
            same = torch.equal(sm_got, smooth_tracks(got, SMOOTH))
            ok &= same
            print(f"         smoothed rows + tail_smooth {tuple(sm_got.shape)}; equal smooth_tracks on the finished track: {same}")
print(f"steady-state push (one graph replay + copies, synchronised): {1e3 * sorted(t_steps)[len(t_steps) // 2]:.2f} ms for {hop / RATE:.1f} s of audio per row")
sys.exit(0 if ok else 1)
