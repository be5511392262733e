#!/usr/bin/env python3
"""Long-form synthesis walk-through on synthetic data, every stage on the HIP path:

  raw 16 kHz recordings [U, total_samples] --eg_window_gather + extract_melspectrogram (GPU)--> one spectrogram per window
  --MLP_Reconstruct_v3.sample per window--> emotion maps --eg_generator_forward_rollout (everything the prior does not reach once at
  batch U*W, then W dependent decoder steps, each seeded with the raw last 4 poses of the one before)--> one gesture track per recording.

Weights are synthetic (integer hash), so the poses carry no meaning; the script shows the call sequence and prints the shapes, the seam
statistics of the track and the time of one call.  With --draws R it then makes R tracks per recording in one call (draw r delivers the line
in emotion (u + r) % 8; the audio tower runs once per window, not R times) and, with --out FILE.npz, writes them: tracks [U, R, T, pose_dim].
With --draws R and more than one recording it also makes the R takes of the recordings of unequal length in one call (harness.synthesize_takes:
recording u keeps (u + 1) / U of the audio; --beat and --diversity then score every take on its recording's own samples and poses).
With --beat the generator is BEAT-shaped (60 poses of 282 columns, 10 of them the prior: the beat joints are columns 18:42 and 150:174) and every
call also returns the beat-alignment score of each track against its own audio (per recording, and per draw with --draws).
With --diversity (and --draws R, R >= 2) the draws call also returns the take diversity of every recording: the mean pairwise distance of its
R takes in FGD feature space (takes.take_diversity, fp64 on the GPU, in the unit of one generator window), and the script shows the FGD of
whole tracks from the same features (takes.track_features -> FrechetAccumulator).  On the TED shape (without --beat) it shows both also in
MotionAE's latent space: diversity=MotionAE and motionfeat.window_features (the encoder on every 34-frame window, one fused launch per range).
With --audio-rate HZ (48000, 44100, 24000, ...) the test signal is made at that rate and every call gets audio_rate=HZ: the recordings are
resampled to 16 kHz on the GPU (resample.resample_audio) before anything else runs; lengths are then counted in samples at HZ.
With --joints (TED shape only) the rectangular call also returns the joint positions of every track in metres (skeleton.ted_expressive(): 43
joints; the mean is zero here, the bones are re-normalised to unit length), with --joints-fps N resampled from 15 to N frames per second, and the
script prints their shape and how far the two wrists travel.
With --rotations (and --joints) the call also returns one local rotation per bone and frame (unit quaternions w, x, y, z relative to the parent
bone: what a rigged avatar takes) against a rest pose taken from the normalised first generated frame of recording 0, and the script prints
their shape and the largest elbow swing in degrees.
With --smooth K P the call also returns the smoothed track (smooth.smooth_tracks: a Savitzky-Golay filter of window K and polyorder P along
time, scipy.signal.savgol_filter(mode="interp"), one more launch); with --joints the joints (and rotations) are made from it, and the script
prints the mean frame-to-frame step of the left wrist before and after -- without --joints, of the pose vector.
With --kinematics (and --joints, TED shape) the call also returns the motion statistics of the joints (kinematics.kinematics_of_joints: mean
speed, acceleration and jerk per joint and a histogram of the joint speeds, one read of the joints on the device), and the script prints the
mean speed and jerk of the two wrists -- with --smooth also those of the raw joints and the Hellinger distance between the raw and the smoothed
speed histograms.
With --srgr and / or --l1div (and --joints, TED shape) the call also returns the joint-space scores of the BEAT table per recording
(jointscore.srgr_of_joints: two more launches; jointscore.l1div_of_tracks on the joints as 129 columns: four more).  There is no captured
motion here, so the stand-in target of --srgr is the joints of the same track smoothed with a (9, 3) Savitzky-Golay filter and the semantic
weights are 1 on every third second: the script prints the recall at 2 cm, the weighted rate and the L1 diversity in metres.
With --emotion the call also asks a skeleton emotion classifier (a SkeletonTransformer with synthetic weights here: d_model 64, 8 heads,
2 layers, windows of 12 poses) which emotion every returned take shows (emotion.emotion_of_tracks on the raw track: one decision per take from
the votes of its classifier windows), and the script prints per take the asked and the recognised emotion and the pooled accuracy -- with
--draws R every take of a recording is asked for its own emotion.
With --beat --joints the body is a skeleton.JointTree -- the BEAT columns are one 6-D rotation per joint -- read from the HIERARCHY block of
--bvh FILE (which must have 47 joints, or name them with --bvh-joints A,B,...), or a synthetic 47-joint upper body without --bvh: joint
positions and, with --rotations, one local rotation per joint come from ONE more launch (skeleton.launch_articulate), and the script prints their
shapes, how far the deepest joint travels and the largest rotation angle.
With --bvh FILE --bvh-out DIR the call also returns the Euler channels of every joint in the file's own channel orders (euler=BvhFile,
euler_unwrap=True: one more launch and the Euler filter's three) and the script writes DIR/recording_U[_take_R].bvh -- the file's HIERARCHY,
then the generated MOTION at the joints' frame rate -- one file per recording and take, formatted on the device in one call (bvh.BvhFile.write_tracks).
With --joints --preview DIR [--preview-size H W] (default 240 320) the call also returns stick-figure pictures of every frame (preview=: one more
launch; Y, Cb, Cr planes) and the script writes DIR/recording_U[_take_R].y4m, uncompressed YUV4MPEG2 that players and encoders read, and prints
the encoder command that would mux a file with its audio (it does not run it).
usage: demo_synthesize.py [utterances=4] [seconds=60] [--draws R] [--beat] [--diversity] [--audio-rate HZ] [--joints [--bvh FILE [--bvh-joints A,B,...] [--bvh-out DIR]] [--joints-fps N] [--rotations] [--preview DIR [--preview-size H W]]] [--smooth K P] [--kinematics] [--srgr] [--l1div] [--emotion] [--out tracks.npz]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from emotiongestures_amd import harness as H
from emotiongestures_amd import resample as R_
from emotiongestures_amd.builders import build_mirror
from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
from emotiongestures_amd.synth import load_synth_weights, synth_audio

argv, DRAWS, OUT, BEAT, DIVERSITY, RATE, JOINTS, JOINTS_FPS, ROTATIONS, SMOOTH = [], 0, None, False, False, 16000, False, None, False, None
BVH, BVH_JOINTS, BVH_OUT, KINEMATICS, SRGR, L1DIV, EMOTION = None, None, None, False, False, False, False
PREVIEW, PREVIEW_SIZE = None, (240, 320)
it = iter(sys.argv[1:])
for a in it:
    if a == "--draws":
        DRAWS = int(next(it))
    elif a == "--beat":
        BEAT = True
    elif a == "--diversity":
        DIVERSITY = True
    elif a == "--audio-rate":
        RATE = int(next(it))
    elif a == "--out":
        OUT = next(it)
    elif a == "--joints":
        JOINTS = True
    elif a == "--joints-fps":
        JOINTS_FPS = int(next(it))
    elif a == "--rotations":
        ROTATIONS = True
    elif a == "--bvh":
        BVH = next(it)
    elif a == "--bvh-joints":
        BVH_JOINTS = next(it).split(",")
    elif a == "--bvh-out":
        BVH_OUT = next(it)
    elif a == "--smooth":
        SMOOTH = (int(next(it)), int(next(it)))
    elif a == "--kinematics":
        KINEMATICS = True
    elif a == "--srgr":
        SRGR = True
    elif a == "--l1div":
        L1DIV = True
    elif a == "--emotion":
        EMOTION = True
    elif a == "--preview":
        PREVIEW = next(it)
    elif a == "--preview-size":
        PREVIEW_SIZE = (int(next(it)), int(next(it)))
    else:
        argv.append(a)
if DIVERSITY and DRAWS < 2:
    sys.exit("--diversity needs --draws R with R >= 2 (the take diversity is a distance between the takes of one recording)")
if BVH and not (JOINTS and BEAT):
    sys.exit("--bvh needs --beat --joints (a BVH hierarchy is the body of the BEAT generators' 6-D joint rotations)")
if BVH_OUT and not BVH:
    sys.exit("--bvh-out needs --bvh FILE (the written files repeat that file's HIERARCHY)")
if JOINTS_FPS and not JOINTS:
    sys.exit("--joints-fps needs --joints")
if PREVIEW and not JOINTS:
    sys.exit("--preview needs --joints (the pictures are those of the joints)")
if ROTATIONS and not JOINTS:
    sys.exit("--rotations needs --joints (the rest pose belongs to the skeleton's bones)")
if KINEMATICS and (not JOINTS or BEAT):
    sys.exit("--kinematics needs --joints without --beat (the statistics are those of the joints, in metres; the script names the TED wrists)")
if (SRGR or L1DIV) and (not JOINTS or BEAT):
    sys.exit("--srgr / --l1div need --joints without --beat (the scores are those of the joints, in metres)")
if SRGR and SMOOTH:
    sys.exit("--srgr without --smooth: the smoothed track's joints are the stand-in target the raw joints are scored against")
U = int(argv[0]) if len(argv) > 0 else 4
seconds = float(argv[1]) if len(argv) > 1 else 60.0
dev = torch.device("cuda:0")
FRAMES, POSE_DIM, PRIOR, FPS = 34, 126, 4, 15           # TED timing: 34 poses @ 15 fps, 4 of them the prior
if BEAT:
    FRAMES, POSE_DIM, PRIOR = 60, 282, 10               # BEAT: 60 poses of 282 columns, 10 of them the prior
HOP = FRAMES - PRIOR
hop_samples = int(round(HOP * 16000 / FPS))              # 30 poses = 2 s = 32 000 samples
total_in = int(seconds * RATE)                            # samples per recording as the caller has them
AR = {"audio_rate": RATE} if RATE != 16000 else {}
total = R_.out_length(total_in, RATE) if AR else total_in    # ... and at the model's 16 kHz
W = (total - 1) // hop_samples + 1                       # every window starts inside the recording; the last is completed by mirroring

audio = torch.from_numpy(synth_audio(U, total_in, seed=90)).to(dev)
text = torch.zeros(U, W, 60, dtype=torch.int64, device=dev)
seed_pose = torch.zeros(U, PRIOR, POSE_DIM, device=dev)
labels = torch.nn.functional.one_hot(torch.arange(U) % 8, 8).float().to(dev)     # one emotion per recording



def write_previews(jo, spec, dt_with):
    """--preview: one .y4m per recording and take from jo["preview"], and the command that would mux the first with its audio."""
    from emotiongestures_amd import preview as PV_
    os.makedirs(PREVIEW, exist_ok=True)
    pics, rate = jo["preview"], JOINTS_FPS or FPS
    takes = pics if pics.dim() == 6 else pics[:, None]                     # [U, R, T', 3, H, W]
    t0 = time.perf_counter()
    names, nbytes = [], 0
    for u in range(takes.shape[0]):
        for r in range(takes.shape[1]):
            names.append(os.path.join(PREVIEW, f"recording_{u}" + (f"_take_{r}" if pics.dim() == 6 else "") + ".y4m"))
            nbytes += PV_.write_y4m(names[-1], takes[u, r], rate, n=jo["joint_frames"][u], spec=spec)
    print(f"--preview: preview {tuple(pics.shape)} uint8 (Y, Cb, Cr planes), one more launch in the call ({1e3 * dt_with:.2f} ms); {len(names)} files, "
          f"{nbytes / 1e6:.1f} MB, written to {PREVIEW} in {time.perf_counter() - t0:.2f} s; to mux one with its audio (YOUR_AUDIO.wav: the "
          f"recording it was made from, which this script does not write):\n"
          f"  ffmpeg -i {names[0]} -i YOUR_AUDIO.wav -c:v libx264 -pix_fmt yuv420p -shortest {os.path.splitext(names[0])[0]}.mp4")


def preview_spec(body):
    from emotiongestures_amd import preview as PV_
    return PV_.PreviewSpec(body, *PREVIEW_SIZE, camera=PV_.Camera.orbit(span=1.4, height=PREVIEW_SIZE[0], width=PREVIEW_SIZE[1]), layout="chw",
                           colorspace="ycbcr")


gen = build_mirror("spatial", FRAMES, POSE_DIM, PRIOR, PRIOR, seed=7, precision="bf16x3").to(dev)
vae = load_synth_weights(MLP_Reconstruct_v3(frames=FRAMES), 7).eval().to(dev)
z = torch.randn(U, W, 32)
out = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, want_windows=True, **AR)          # warm-up (packs weights, allocates workspaces)
torch.cuda.synchronize()
t0 = time.perf_counter()
out = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, want_windows=True, beat=BEAT, **AR)
torch.cuda.synchronize()
dt = time.perf_counter() - t0

track, windows = out["track"], out["windows"]
if AR:
    print(f"--audio-rate {RATE}: L / M = {R_.ratio(RATE)}, {total_in} samples -> {tuple(out['audio'].shape)} at 16 kHz on the device")
print(f"{U} recordings x {seconds:.0f} s -> {W} windows of {FRAMES} poses (hop {HOP}) -> track {tuple(track.shape)} = {track.shape[1] / FPS:.1f} s at {FPS} fps")
step = (track[:, 1:] - track[:, :-1]).norm(dim=2)                       # pose change per frame
seams = torch.tensor([w * HOP + j for w in range(1, W) for j in range(PRIOR + 1)]) - 1
print(f"mean |pose[t+1] - pose[t]|: {float(step.mean()):.4f} over the track, {float(step[:, seams].mean()):.4f} across the cross-faded seams")
print(f"window 1 beyond its overlap (rows [{HOP + PRIOR}, {2 * HOP})) appears raw in the track: "
      f"{bool(torch.equal(track[:, HOP + PRIOR: FRAMES + HOP - PRIOR], windows[:, 1, PRIOR: HOP]))}")
print(f"one call (mel + CVAE + roll-out{' + beat score' if BEAT else ''}, eager): {1e3 * dt:.2f} ms = {1e3 * dt / (U * track.shape[1] / FPS):.4f} ms per second of audio")
if BEAT:
    print(f"--beat: beat-alignment score per recording: {[round(float(v), 4) for v in out['beat'].cpu()]}")
if JOINTS and BEAT:
    from emotiongestures_amd.skeleton import JointTree
    from tools.bench_articulate import synthetic_tree
    import emotiongestures_amd.skeleton as SK_
    tree = JointTree.from_bvh(open(BVH).read(), joints=BVH_JOINTS) if BVH else synthetic_tree(SK_)
    jk = dict(joints=tree, joints_fps=(FPS, JOINTS_FPS) if JOINTS_FPS else None, smooth=SMOOTH, rotations=True if ROTATIONS else None)
    if BVH_OUT:
        from emotiongestures_amd import bvh as BVH_
        bvh_file = BVH_.read(BVH)
        jk.update(euler=bvh_file, euler_unwrap=True)
    if PREVIEW:
        jk["preview"] = preview_spec(tree)
    H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, **jk, **AR)          # warm-up (uploads the level table)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    jo = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, **jk, **AR)
    torch.cuda.synchronize()
    dt_j = time.perf_counter() - t0
    joints = jo["joints"]
    deep = int(tree.depth.argmax())
    extent = (joints[:, :, deep].amax(1) - joints[:, :, deep].amin(1)).norm(dim=1).mean()
    print(f"--joints: {tree!r}{' from ' + BVH if BVH else ' (synthetic)'}: joints {tuple(joints.shape)} (frames per recording {jo['joint_frames']}" +
          (f", {FPS} -> {JOINTS_FPS} fps" if JOINTS_FPS else "") + f"), one more launch in the call ({1e3 * dt_j:.2f} ms against {1e3 * dt:.2f} ms); "
          f"extent of joint {deep}{' ' + tree.names[deep] if tree.names else ''} ({int(tree.depth[deep])} joints from the root): {float(extent):.3f} m")
    if PREVIEW:
        write_previews(jo, jk["preview"], dt_j)
    if SMOOTH:
        print(f"--smooth {SMOOTH[0]} {SMOOTH[1]}: the joints come from track_smooth {tuple(jo['track_smooth'].shape)}: Gram-Schmidt re-orthonormalises "
              "the filtered 6-D rows")
    if ROTATIONS:
        rot = jo["rotations"]
        print(f"--rotations: rotations {tuple(rot.shape)} from the same launch; largest local rotation: "
              f"{float(torch.rad2deg(2 * torch.acos(rot[..., 0].clamp(max=1.0))).max()):.1f} degrees")
    if BVH_OUT:
        os.makedirs(BVH_OUT, exist_ok=True)
        eul = jo["euler"]
        takes = eul if eul.dim() == 5 else eul[:, None]                  # [U, R, T', J, 3]
        names = [os.path.join(BVH_OUT, f"recording_{u}" + (f"_take_{r}" if eul.dim() == 5 else "") + ".bvh")
                 for u in range(takes.shape[0]) for r in range(takes.shape[1])]
        t0 = time.perf_counter()
        bvh_file.write_tracks(names, eul, jo["joint_frames"], joints=tree.names, frame_time=1.0 / (JOINTS_FPS or FPS))
        print(f"--bvh-out: euler {tuple(eul.shape)} in the orders of {BVH} (unwrapped), {len(names)} files in {BVH_OUT} "
              f"formatted on the device and written in {time.perf_counter() - t0:.2f} s")
elif JOINTS:
    from emotiongestures_amd.skeleton import ted_expressive
    jk = dict(joints=ted_expressive(), joints_unit=True, joints_fps=(FPS, JOINTS_FPS) if JOINTS_FPS else None, smooth=SMOOTH,
              kinematics=True if KINEMATICS else None)
    if ROTATIONS:                                        # the rest pose: the first generated frame of recording 0 (normalised by the call)
        jk["rotations"] = track[0, PRIOR].reshape(-1, 3).cpu()
    if SRGR:                                             # the stand-in target: the joints of the smoothed track; weights 1 on every third second
        from emotiongestures_amd.jointscore import SemanticTargets
        tj = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, **dict(jk, smooth=(9, 3), kinematics=None), **AR)["joints"]
        sem = ((torch.arange(tj.shape[1], device=dev) // (JOINTS_FPS or FPS)) % 3 == 0).float()[None].expand(U, -1).contiguous()
        jk["srgr"] = SemanticTargets(tj, sem, threshold=0.02)
    jk["l1div"] = L1DIV
    if PREVIEW:
        jk["preview"] = preview_spec(jk["joints"])
    H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, **jk, **AR)          # warm-up (uploads the bone table)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    jo = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, **jk, **AR)
    torch.cuda.synchronize()
    dt_j = time.perf_counter() - t0
    joints = jo["joints"]
    extent = lambda j: (joints[:, :, j].amax(1) - joints[:, :, j].amin(1)).norm(dim=1).mean()      # diagonal of the joint's bounding box
    print(f"--joints: joints {tuple(joints.shape)} (frames per recording {jo['joint_frames']}" +
          (f", {FPS} -> {JOINTS_FPS} fps" if JOINTS_FPS else "") + f"), one more launch in the call ({1e3 * dt_j:.2f} ms against {1e3 * dt:.2f} ms); "
          f"wrist extent: left {float(extent(6)):.3f} m, right {float(extent(7)):.3f} m")
    if PREVIEW:
        write_previews(jo, jk["preview"], dt_j)
    if SMOOTH:                                           # the joints above come from out["track_smooth"]; the raw track's for comparison
        from emotiongestures_amd.skeleton import joints_from_tracks
        raw = joints_from_tracks(jo["track"], jk["joints"], unit=True, fps=jk["joints_fps"])
        raw = raw[0] if isinstance(raw, tuple) else raw
        wrist_step = lambda j: float((j[:, 1:, 6] - j[:, :-1, 6]).norm(dim=2).mean())
        print(f"--smooth {SMOOTH[0]} {SMOOTH[1]}: track_smooth {tuple(jo['track_smooth'].shape)}, one more launch; mean frame-to-frame step of the left "
              f"wrist: {1e3 * wrist_step(raw):.2f} mm raw, {1e3 * wrist_step(joints):.2f} mm smoothed")
    if KINEMATICS:                                       # of jo["joints"]: the smoothed ones with --smooth
        from emotiongestures_amd import kinematics as KM
        kin = jo["kinematics"]
        wrists = lambda k, name: [round(float(k[name][:, j].mean()), 3) for j in (6, 7)]
        print(f"--kinematics: one read of the joints ({kin['speed_hist'].shape[-1]} bins up to {kin['edges'][-1]:g} m/s); mean wrist speed (left, right) "
              f"{wrists(kin, 'speed')} m/s, mean wrist jerk {wrists(kin, 'jerk')} m/s^3")
        if SMOOTH:
            from emotiongestures_amd.skeleton import joints_from_tracks
            raw_j = joints_from_tracks(jo["track"], jk["joints"], unit=True, fps=jk["joints_fps"])
            raw_k = KM.kinematics_of_joints(raw_j[0] if isinstance(raw_j, tuple) else raw_j, JOINTS_FPS or FPS, frames=jo["joint_frames"])
            full = lambda k: torch.cat([k["speed_hist"], k["speed_over"][..., None]], -1)
            print(f"--kinematics --smooth: the raw joints: mean wrist speed {wrists(raw_k, 'speed')} m/s, mean wrist jerk {wrists(raw_k, 'jerk')} m/s^3; "
                  f"Hellinger distance between the raw and the smoothed speed histograms, all joints pooled, per recording: "
                  f"{[round(float(v), 4) for v in KM.hellinger(full(raw_k), full(kin), pool=True).cpu()]}")
    if SRGR:
        sr = jo["srgr"]
        print(f"--srgr: the raw joints against those of the (9, 3)-smoothed track, two more launches: recall at 2 cm per recording "
              f"{[round(float(v), 4) for v in sr['recall'].cpu()]}, rate weighted by every third second (scale 1 / 0.165) "
              f"{[round(float(v), 4) for v in sr['srgr'].cpu()]}; the joint hit least often: {int(sr['hits'].sum(0).argmin())}")
    if L1DIV:
        l1 = jo["l1div"]
        print(f"--l1div: L1 diversity of the joints as {l1['mean'].shape[-1]} columns, four more launches: "
              f"{[round(float(v), 4) for v in l1['l1div'].cpu()]} m summed over the columns, per frame")
    if ROTATIONS:
        rot = jo["rotations"]
        swing = lambda k: float(torch.rad2deg(2 * torch.acos(rot[:, :, k, 0].clamp(max=1.0))).max())    # bone 4 / 21: left / right forearm
        print(f"--rotations: rotations {tuple(rot.shape)}, one more launch; largest elbow swing against the first generated frame: "
              f"left {swing(4):.1f} degrees, right {swing(21):.1f} degrees")
if EMOTION:
    from emotiongestures_amd.emotion import EmotionAccuracy
    NAMES = ("neutral", "happiness", "anger", "sadness", "contempt", "surprise", "fear", "disgust")
    skel = load_synth_weights(H.SkeletonTransformer(pose_dim=POSE_DIM, n_position=12, n_layers=2, d_k=64, d_v=64), 7).eval().to(dev)
    R_E = max(DRAWS, 1)
    asked = (torch.arange(U)[:, None] + 3 * torch.arange(R_E)[None, :]) % 8                       # [U, R]: each take its own emotion
    ek = dict(z=torch.randn(U, R_E, W, 32), draws=R_E) if DRAWS else dict(z=z)
    lab_e = torch.nn.functional.one_hot(asked, 8).float()[:, :, None, :].expand(U, R_E, W, 8).to(dev) if DRAWS else labels
    H.synthesize((gen, vae), audio, text, seed_pose, labels=lab_e, emotion=skel, **ek, **AR)       # warm-up (packs the classifier's weights)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    em = H.synthesize((gen, vae), audio, text, seed_pose, labels=lab_e, emotion=skel, **ek, **AR)["emotion"]
    torch.cuda.synchronize()
    dt_e = time.perf_counter() - t0
    pred, votes = em["pred"].cpu(), em["votes"].cpu()
    print(f"--emotion: {em['logits'].shape[0]} classifier windows of 12 poses ({em['windows_per'][0]} per take), the call {1e3 * dt_e:.2f} ms against "
          f"{1e3 * dt:.2f} ms without; per take asked -> recognised (votes of the recognised class / windows):")
    for u in range(U):
        print("  recording %d: " % u + ", ".join(f"{NAMES[int(asked[u, r])]} -> {NAMES[int(pred[u, r])] if pred[u, r] >= 0 else 'none'} "
                                                   f"({int(votes[u, r].max())}/{em['windows_per'][u]})" for r in range(R_E)))
    pool = EmotionAccuracy()
    pool.push(em)
    print(f"  pooled: {pool.hits} of {pool.takes} takes recognised as asked ({pool.avg():.1f} %), {pool.window_avg():.1f} % of the windows, "
          f"{pool.unscored} takes without a valid window (synthetic weights: chance is 12.5 %)")
if SMOOTH and not JOINTS:
    ts = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, smooth=SMOOTH, **AR)["track_smooth"]
    print(f"--smooth {SMOOTH[0]} {SMOOTH[1]}: track_smooth {tuple(ts.shape)}, one more launch; mean |pose[t+1] - pose[t]|: {float(step.mean()):.4f} raw, "
          f"{float((ts[:, 1:] - ts[:, :-1]).norm(dim=2).mean()):.4f} smoothed")

# Recordings of unequal length in one call: recording u keeps (u + 1) / U of the audio.  Step s runs only the recordings that still have a
# window s; the track is padded to the longest recording and zero past each recording's own end.
if U > 1:
    lengths = [max(1, total_in * (u + 1) // U) for u in range(U)]
    rag = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels, z=z, lengths=lengths, beat=BEAT, **AR)
    torch.cuda.synchronize()
    if BEAT:
        print(f"--beat: recordings of unequal length, each scored on its own samples and poses: {[round(float(v), 4) for v in rag['beat'].cpu()]}")
    frames = rag["track_frames"].tolist()
    print(f"lengths {[round(v / RATE, 1) for v in lengths]} s -> windows {rag['windows_per']} -> track {tuple(rag['track'].shape)}, frames per recording {frames}; "
          f"rows past a recording's end are zero: {all(not bool(rag['track'][u, frames[u]:].any()) for u in range(U))}; "
          f"the longest recording against the rectangular call's: rel-L2 {float((rag['track'][U - 1] - track[U - 1]).norm() / track[U - 1].norm()):.1e} "
          f"(its last steps run alone, at batch 1)")

# Several candidate performances of every recording in one call: draw r of recording u is sampled with emotion (u + r) % 8 and its own latents.
if DRAWS > 0:
    labels_r = torch.nn.functional.one_hot((torch.arange(U)[:, None] + torch.arange(DRAWS)[None, :]) % 8, 8).float()
    labels_r = labels_r[:, :, None, :].expand(U, DRAWS, W, 8).to(dev)
    zr = torch.randn(U, DRAWS, W, 32)
    fgd = load_synth_weights(H.MLP_Reconstruct(pose_dim=POSE_DIM), 7).eval().to(dev) if DIVERSITY else None
    H.synthesize((gen, vae), audio, text, seed_pose, labels=labels_r, z=zr, draws=DRAWS, diversity=fgd, **AR)    # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    div = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels_r, z=zr, draws=DRAWS, beat=BEAT, diversity=fgd, **AR)
    torch.cuda.synchronize()
    dt_r = time.perf_counter() - t0
    if BEAT:
        print(f"--beat: score per recording and draw [U, R] (the audio half runs once per recording):\n{div['beat'].cpu().numpy().round(4)}")
    tracks = div["track"]
    if DIVERSITY:
        print(f"--diversity: take diversity per recording (mean FGD-feature distance of its {DRAWS} takes, per {FRAMES}-frame window): "
              f"{[round(float(v), 4) for v in div['take_diversity'].cpu()]}")
        # FGD of whole tracks from the same features: draw 0 of every recording against draw 1, valid frames only, moments kept on the GPU
        from emotiongestures_amd import takes
        acc_a, acc_b = H.FrechetAccumulator(512, dev), H.FrechetAccumulator(512, dev)
        acc_a.push(takes.track_features(fgd, tracks[:, 0].contiguous())[0])
        acc_b.push(takes.track_features(fgd, tracks[:, 1].contiguous())[0])
        fgd_ab = H.calculate_frechet_distance(*acc_a.stats(), *acc_b.stats())
        print(f"--diversity: FGD of the draw-0 tracks against the draw-1 tracks ({U * tracks.shape[2]} feature rows each): {float(np.real(fgd_ab)):.4f}")
        if not BEAT:    # the TED shape has a feature space of its own: MotionAE's encoder on every 34-frame window, one fused launch per range
            from emotiongestures_amd import motionfeat
            from emotiongestures_amd.model.motion_ae import MotionAE
            ae = load_synth_weights(MotionAE(POSE_DIM, 128), 41).eval().to(dev)
            ted = H.synthesize((gen, vae), audio, text, seed_pose, labels=labels_r, z=zr, draws=DRAWS, diversity=ae, **AR)
            print(f"--diversity: the same in MotionAE's latent space (RMS feature distance per 34-frame window, stride 34): "
                  f"{[round(float(v), 4) for v in ted['take_diversity'].cpu()]}")
            acc_a, acc_b = H.FrechetAccumulator(128, dev), H.FrechetAccumulator(128, dev)
            fa, plan = motionfeat.window_features(ae, tracks[:, 0].contiguous(), stride=17)
            acc_a.push(fa)
            acc_b.push(motionfeat.window_features(ae, tracks[:, 1].contiguous(), stride=17)[0])
            fgd_ab = H.calculate_frechet_distance(*acc_a.stats(), *acc_b.stats())
            print(f"--diversity: MotionAE FGD of the draw-0 tracks against the draw-1 tracks ({plan.total} windows each at stride 17): "
                  f"{float(np.real(fgd_ab)):.4f}")
    spread = (tracks - tracks.mean(dim=1, keepdim=True)).norm(dim=3).mean()
    print(f"--draws {DRAWS}: tracks {tuple(tracks.shape)} in one call, {1e3 * dt_r:.2f} ms = {1e3 * dt_r / (U * DRAWS * tracks.shape[2] / FPS):.4f} ms per "
          f"second of track (one track per recording: {1e3 * dt / (U * track.shape[1] / FPS):.4f}); mean distance of a draw from its recording's mean "
          f"track: {float(spread):.4f}")
    if U > 1:       # the two combined: R takes of recordings of unequal length, one call (the tower once per window, step s at batch U_s * R)
        H.synthesize_takes((gen, vae), audio, text, seed_pose, labels_r, lengths=lengths, draws=DRAWS, z=zr, **AR)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tk = H.synthesize_takes((gen, vae), audio, text, seed_pose, labels_r, lengths=lengths, draws=DRAWS, z=zr, beat=BEAT, diversity=fgd, **AR)
        torch.cuda.synchronize()
        dt_t = time.perf_counter() - t0
        frames = tk["track_frames"].tolist()
        print(f"--draws {DRAWS} with lengths {[round(v / RATE, 1) for v in lengths]} s (synthesize_takes): windows {tk['windows_per']} -> tracks "
              f"{tuple(tk['track'].shape)}, frames per recording {frames}, {1e3 * dt_t:.2f} ms = "
              f"{1e3 * dt_t / (DRAWS * sum(frames) / FPS):.4f} ms per second of track; rows past a recording's end are zero in every take: "
              f"{all(not bool(tk['track'][u, :, frames[u]:].any()) for u in range(U))}")
        if BEAT:
            print(f"--beat: score per recording and take [U, R], each on its own samples and poses:\n{tk['beat'].cpu().numpy().round(4)}")
        if DIVERSITY:
            print(f"--diversity: take diversity per recording over its own frames: {[round(float(v), 4) for v in tk['take_diversity'].cpu()]}")
    if OUT:
        np.savez(OUT, tracks=tracks.cpu().numpy(), emotion=((torch.arange(U)[:, None] + torch.arange(DRAWS)[None, :]) % 8).numpy(), fps=FPS)
        print(f"wrote {OUT}: tracks [U, R, T, pose_dim] = {tuple(tracks.shape)}")
