"""Long-form roll-out on the GPU (eg_generator_forward_rollout through GeneratorEngine.forward_rollout / Transformer.synthesize /
harness.synthesize) against (1) goldens made by calling the reference's Transformer window after window and (2) a Python loop of
model.forward + slicing + the blend in torch on the same device and precision."""
import numpy as np
import pytest
import torch

import rollout_np as R
from conftest import build_mirror, clip_rel_l2, rel_l2
from emotiongestures_amd import _lib as L
from emotiongestures_amd.synth import synth_audio
from rollout_np import CASES, load_case

pytestmark = pytest.mark.gpu

POSE_TOL = {"f32": 2e-5, "bf16x3": 1e-3}        # tests/test_gpu_generator.py:15
F_, D_, P_ = 34, 126, 4
H_ = F_ - P_
_MODELS = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def model_for(variant, prec, seed=7):
    key = (variant, prec, seed)
    if key not in _MODELS:
        _MODELS[key] = build_mirror(variant, F_, D_, P_, 4, seed=seed, precision=prec).to(dev())
    return _MODELS[key]


def inputs(U, W, seed, with_sampled):
    inp = R.rollout_inputs(U, W, F_, D_, P_, seed=seed)
    g = {k: torch.from_numpy(inp[k]).to(dev()) for k in ("spec", "text", "seed_pose")}
    g["sampled"] = None
    if with_sampled:
        from emotiongestures_amd.synth import hash_uniform
        g["sampled"] = torch.from_numpy(hash_uniform("rollout/sampled", (U, W, F_, 512), -1.0, 1.0, seed)).to(dev())
    return g


def torch_loop(model, spec, text, seed_pose, sampled=None, alpha=None):
    """What the library offered before the roll-out: one forward() per window, the hand-off and the blend as torch ops on the device."""
    U, W = spec.shape[:2]
    a = torch.from_numpy(R.default_alpha(P_)).to(spec.device) if alpha is None else alpha
    a = a[None, :, None]
    track = torch.empty(U, W * H_ + P_, D_, device=spec.device)
    prior, wins, aux = seed_pose, [], []
    with torch.no_grad():
        for w in range(W):
            out = model(spec[:, w].contiguous(), text[:, w].contiguous(), prior.contiguous(), None if sampled is None else sampled[:, w].contiguous())
            pose = out[0]
            if w == 0:
                track[:, :F_] = pose
            else:
                track[:, w * H_: w * H_ + P_] = (1 - a) * prior + a * pose[:, :P_]
                track[:, w * H_ + P_: w * H_ + F_] = pose[:, P_:]
            wins.append(pose)
            aux.append(out[1:])
            prior = pose[:, H_:]
    stack = lambda i: torch.stack([x[i] for x in aux], 1)
    return {"track": track, "windows": torch.stack(wins, 1), "emotion_feature": stack(0), "semantic_feature": stack(1),
            "emotion_prediction": stack(2), "text_embedding": stack(3)}


# ---- against the reference goldens ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_teacher_forced_windows_match_reference_golden(name, prec):
    """Every golden window through forward() seeded with the golden's own prior: the one-clip-at-a-time bar, which anchors the free-running one."""
    z, m, inp, sampled = load_case(name)
    model = model_for(CASES[name], prec, m["seed"])
    H = m["frames"] - m["prior"]
    with torch.no_grad():
        for w in range(m["W"]):
            prior = inp["seed_pose"] if w == 0 else z["windows"][:, w - 1, H:]
            pose = model(torch.from_numpy(inp["spec"][:, w]).to(dev()), torch.from_numpy(inp["text"][:, w]).to(dev()),
                         torch.from_numpy(np.ascontiguousarray(prior)).to(dev()), None if sampled is None else sampled[:, w].to(dev()))[0]
            e = clip_rel_l2(pose.cpu().numpy(), z["windows"][:, w])
            print(f"{name} {prec} teacher-forced window {w}: per-clip rel-L2 {e:.2e}")
            assert e < POSE_TOL[prec], (w, e)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_free_running_rollout_matches_reference_golden(name, prec):
    """forward_rollout against the reference rolled out window after window.  Window w may differ by POSE_TOL * (1 + window_gain *
    sum_{i<w} handoff_gain^i), both gains measured on the reference and read from the fixture.  The track is a convex blend of the windows,
    so it is held to the last window's bar; emotion_prediction does not depend on the prior and keeps the bar of test_gpu_generator (5 x)."""
    z, m, inp, sampled = load_case(name)
    model = model_for(CASES[name], prec, m["seed"])
    hg, wg = float(z["handoff_gain"]), float(z["window_gain"])
    out = model.synthesize(torch.from_numpy(inp["spec"]).to(dev()), torch.from_numpy(inp["text"]).to(dev()), torch.from_numpy(inp["seed_pose"]).to(dev()),
                           None if sampled is None else sampled.to(dev()), want_windows=True)
    torch.cuda.synchronize()
    win = out["windows"].cpu().numpy()
    assert win.shape == z["windows"].shape and tuple(out["track"].shape) == z["track"].shape
    for w in range(m["W"]):
        e, tol = clip_rel_l2(win[:, w], z["windows"][:, w]), R.free_running_tol(POSE_TOL[prec], wg, hg, w)
        print(f"{name} {prec} free-running window {w}: per-clip rel-L2 {e:.2e} (tolerance {tol:.2e})")
        assert e < tol, (w, e, tol)
    e = clip_rel_l2(out["track"].cpu().numpy(), z["track"])
    print(f"{name} {prec} track: per-clip rel-L2 {e:.2e}")
    assert e < R.free_running_tol(POSE_TOL[prec], wg, hg, m["W"] - 1)
    assert rel_l2(out["emotion_prediction"].cpu().numpy(), z["emotion_prediction"]) < POSE_TOL[prec] * 5
    # the track is exactly the stitch of the windows this call produced (same fp32 arithmetic on the host)
    assert np.array_equal(out["track"].cpu().numpy(), R.stitch(win, m["prior"]))


# ---- against the loop of forward() calls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sampled", [False, True])
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("U", [1, 2, 5])
@pytest.mark.parametrize("variant", ["spatial", "memory"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_rollout_equals_loop_of_forwards(prec, variant, U, W, with_sampled):
    """Same precision, same device: every window within POSE_TOL of the loop's.  From two utterances up the products accumulate K in one order
    whatever the batch, so phase A at batch U*W and the loop's forwards at batch U agree bit for bit: asserted.  With one utterance the loop's
    encoder takes the one-clip split-K of w_2 (bf16 modes only) and phase A (W > 1) does not: there, equal to rounding only (measured on MI355X:
    2.0e-5 per-clip relative L2 in bf16x3)."""
    model = model_for(variant, prec)
    g = inputs(U, W, seed=30 + U * 4 + W, with_sampled=with_sampled)
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"], g["sampled"])
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True)
    torch.cuda.synchronize()
    bitwise = torch.equal(got["windows"], want["windows"])
    worst = max(clip_rel_l2(got["windows"][:, w].cpu().numpy(), want["windows"][:, w].cpu().numpy()) for w in range(W))
    print(f"{prec} {variant} U={U} W={W} sampled={with_sampled}: windows bitwise={bitwise} worst per-clip rel-L2 {worst:.2e}; "
          f"track bitwise={torch.equal(got['track'], want['track'])}")
    assert worst < POSE_TOL[prec]
    assert clip_rel_l2(got["track"].cpu().numpy(), want["track"].cpu().numpy()) < POSE_TOL[prec]
    assert rel_l2(got["emotion_prediction"].cpu().numpy(), want["emotion_prediction"].cpu().numpy()) < POSE_TOL[prec] * 5
    if U >= 2 or W == 1 or prec == "f32":
        assert bitwise
        assert torch.equal(got["track"], want["track"])
        assert torch.equal(got["emotion_prediction"], want["emotion_prediction"])


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_one_window_is_forward(prec):
    model = model_for("spatial", prec)
    g = inputs(3, 1, seed=41, with_sampled=True)
    with torch.no_grad():
        pose, emo, sem, pred, txt = model(g["spec"][:, 0], g["text"][:, 0], g["seed_pose"], g["sampled"][:, 0])
    out = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True, want_aux=True)
    assert tuple(out["track"].shape) == (3, F_, D_)
    assert torch.equal(out["track"], pose) and torch.equal(out["windows"][:, 0], pose)
    assert torch.equal(out["emotion_prediction"][:, 0], pred)
    assert torch.equal(out["emotion_feature"][:, 0], emo) and torch.equal(out["semantic_feature"][:, 0], sem)
    assert torch.equal(out["text_embedding"][:, 0], txt)


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_alpha_windows_and_aux_equal_the_loop(variant):
    model = model_for(variant, "bf16x3")
    U, W = 3, 4
    g = inputs(U, W, seed=52, with_sampled=False)
    alpha = torch.tensor([0.9, 0.5, 0.25, 0.0], device=dev())
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"], None, alpha)
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], None, alpha=alpha, want_windows=True, want_aux=True)
    for k in ("track", "windows", "emotion_prediction", "emotion_feature", "semantic_feature", "text_embedding"):
        assert got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k
    plain = model.synthesize(g["spec"], g["text"], g["seed_pose"])
    assert set(plain) == {"track", "emotion_prediction"}
    assert torch.equal(plain["emotion_prediction"], got["emotion_prediction"])
    # the overlap rows differ from the default blend, everything else does not (the hand-off never sees alpha)
    ov = torch.zeros(W * H_ + P_, dtype=torch.bool)
    for w in range(1, W):
        ov[w * H_: w * H_ + P_] = True
    assert torch.equal(plain["track"][:, ~ov], got["track"][:, ~ov]) and not torch.equal(plain["track"][:, ov], got["track"][:, ov])
    # alpha = 0 on the last overlap frame: the old window's raw frame
    assert torch.equal(got["track"][:, H_ + 3], got["windows"][:, 0, H_ + 3])


def test_fold_affine_rollout_equals_its_loop():
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision="bf16x3")
    model.fold_affine = True
    model.to(dev())
    g = inputs(2, 3, seed=61, with_sampled=False)
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"])
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], want_windows=True)
    assert torch.equal(got["windows"], want["windows"]) and torch.equal(got["track"], want["track"])


def test_rollout_is_capturable_in_one_graph():
    """Captured once, replayed three times with fresh inputs copied into the static buffers: bitwise the eager call on those inputs.  The capture
    enqueues exactly the launches of an eager call, and a replay makes no library launch on the host."""
    lib = L.load()
    model = model_for("memory", "bf16x3")
    U, W = 2, 3
    static = inputs(U, W, seed=70, with_sampled=True)
    run = lambda g: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True, want_aux=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)                         # workspace, weight arena: outside the capture
        n0 = lib.eg_launch_count()
        run(static)
        eager_launches = lib.eg_launch_count() - n0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    n0 = lib.eg_launch_count()
    with torch.cuda.graph(graph):
        out = run(static)
    assert lib.eg_launch_count() - n0 == eager_launches
    print(f"roll-out U={U} W={W}: {eager_launches} launches ({eager_launches / W:.1f} per window)")
    for r in range(3):
        fresh = inputs(U, W, seed=71 + r, with_sampled=True)
        for k, v in fresh.items():
            static[k].copy_(v)
        n0 = lib.eg_launch_count()
        graph.replay()
        torch.cuda.synchronize()
        assert lib.eg_launch_count() == n0
        got = {k: v.clone() for k, v in out.items()}
        want = run(fresh)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(got[k], want[k]), (r, k)


def test_window_gather_and_harness_synthesize_from_raw_audio():
    """harness.synthesize(raw audio) == MelFrontEnd on explicit slices + forward_rollout, bit for bit; the last window runs past the end of the
    track and is completed as make_audio_fixed_length does (np.pad mode="symmetric")."""
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.engine import MelFrontEnd
    from emotiongestures_amd.synth import load_synth_weights
    model = model_for("spatial", "bf16x3")
    vae = load_synth_weights(MLP_Reconstruct_v3(frames=F_), 7).eval().to(dev())
    U, W = 2, 3
    hop, n = 32000, (124 - 1) * 512                                  # 30 poses at 15 fps = 2 s
    total = 2 * hop + n - 9000                                       # the last window is 9000 samples short
    audio = synth_audio(U, total, seed=80)
    clips = np.stack([np.pad(audio[u, w * hop: w * hop + n], (0, max(0, w * hop + n - total)), mode="symmetric") for u in range(U) for w in range(W)])
    assert clips.shape == (U * W, n)
    inp = R.rollout_inputs(U, W, F_, D_, P_, seed=80)
    text, seed_pose = torch.from_numpy(inp["text"]).to(dev()), torch.from_numpy(inp["seed_pose"]).to(dev())
    labels, z = torch.from_numpy(inp["label"]).to(dev()), torch.from_numpy(inp["z"]).to(dev())
    mel = MelFrontEnd(dev())
    spec = mel(torch.from_numpy(clips).to(dev()), out_frames=124).view(U, W, 128, 124)
    assert torch.equal(mel.windows(torch.from_numpy(audio).to(dev()), W, hop, n, out_frames=124), spec)
    with torch.no_grad():
        sampled = vae.sample(labels.reshape(U * W, 8), z=z.reshape(U * W, 32)).view(U, W, F_, 512)
    want = model.engine().forward_rollout(spec, text, seed_pose, sampled, want_windows=True)
    got = Hs.synthesize((model, vae), torch.from_numpy(audio).to(dev()), text, seed_pose, labels=labels, hop_samples=hop, z=z, want_windows=True)
    assert torch.equal(got["spec"], spec)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert tuple(got["track"].shape) == (U, W * H_ + P_, D_)
    with pytest.raises(L.EgError, match="windows=5"):               # a window that starts past the end of the recording
        mel.windows(torch.from_numpy(audio).to(dev()), 5, hop, n, out_frames=124)
