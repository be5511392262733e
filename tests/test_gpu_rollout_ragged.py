"""Ragged roll-out on the GPU (eg_generator_forward_rollout_ragged through GeneratorEngine.forward_rollout_ragged, Transformer.synthesize
(windows_per=) and harness.synthesize(lengths=)) against (1) the reference goldens of the rectangular roll-out, which hold every window of
both recordings, (2) the rectangular roll-out the library already has, (3) a Python loop of model.forward on the active rows of every step,
(4) a GestureStream whose rows end at their own lengths."""
import numpy as np
import pytest
import torch

import rollout_np as R
import rollout_ragged_np as RR
from conftest import build_mirror, clip_rel_l2, rel_l2
from emotiongestures_amd import _lib as L
from emotiongestures_amd.synth import hash_uniform, load_synth_weights, synth_audio
from rollout_np import CASES, load_case

pytestmark = pytest.mark.gpu

POSE_TOL = {"f32": 2e-5, "bf16x3": 1e-3}        # tests/test_gpu_generator.py:15
F_, D_, P_ = 34, 126, 4
H_ = F_ - P_
HOP, NS = 32000, (124 - 1) * 512                # 30 poses at 15 fps = 2 s; the shortest clip with 124 spectrogram columns
_MODELS, _VAES = {}, {}
PER_WINDOW = ("windows", "emotion_prediction", "emotion_feature", "semantic_feature", "text_embedding")


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def model_for(variant, prec, seed=7):
    key = (variant, prec, seed)
    if key not in _MODELS:
        _MODELS[key] = build_mirror(variant, F_, D_, P_, 4, seed=seed, precision=prec).to(dev())
    return _MODELS[key]


def vae_for(seed=7):
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    if seed not in _VAES:
        _VAES[seed] = load_synth_weights(MLP_Reconstruct_v3(frames=F_), seed).eval().to(dev())
    return _VAES[seed]


def inputs(wp, seed, with_sampled):
    """Padded [U, Wmax, ...] inputs from the fixtures' generator and their packed [N, ...] form, on the device."""
    U, Wmax = len(wp), max(wp)
    inp = R.rollout_inputs(U, Wmax, F_, D_, P_, seed=seed)
    pad = {k: inp[k] for k in ("spec", "text", "label", "z")}
    pad["sampled"] = hash_uniform("rollout/sampled", (U, Wmax, F_, 512), -1.0, 1.0, seed) if with_sampled else None
    g = {"seed_pose": torch.from_numpy(inp["seed_pose"]).to(dev()), "pad": {}}
    for k, v in pad.items():
        g["pad"][k] = None if v is None else torch.from_numpy(v).to(dev())
        g[k] = None if v is None else torch.from_numpy(RR.pack(v, wp)).to(dev())
    return g


def torch_loop(model, spec, text, seed_pose, wp, sampled=None, alpha=None):
    """What a user can do without the ragged entry and with the same semantics: per step one forward() on the ACTIVE recordings (longer first,
    ties by index), the hand-off and the blend as torch ops on the device (tests/test_gpu_rollout.py's torch_loop restricted to the active set).
    Packed inputs, packed outputs."""
    pl = RR.plan(wp)
    U, N, Wmax, off = len(wp), sum(wp), max(wp), pl["offsets"]
    a = (torch.from_numpy(R.default_alpha(P_)).to(spec.device) if alpha is None else alpha)[:, None]
    track = torch.zeros(U, Wmax * H_ + P_, D_, device=spec.device)
    prior = {int(u): seed_pose[int(u)] for u in pl["order"]}
    per = {k: [None] * N for k in PER_WINDOW}
    with torch.no_grad():
        for s in range(Wmax):
            act = [int(u) for u in pl["order"][: pl["step_batch"][s]]]
            rows = torch.as_tensor([int(off[u]) + s for u in act], device=spec.device)
            out = model(spec[rows].contiguous(), text[rows].contiguous(), torch.stack([prior[u] for u in act]).contiguous(),
                        None if sampled is None else sampled[rows].contiguous())
            for i, u in enumerate(act):
                pose, row = out[0][i], int(off[u]) + s
                if s == 0:
                    track[u, :F_] = pose
                else:
                    track[u, s * H_: s * H_ + P_] = (1 - a) * prior[u] + a * pose[:P_]
                    track[u, s * H_ + P_: s * H_ + F_] = pose[P_:]
                per["windows"][row], per["emotion_feature"][row], per["semantic_feature"][row] = pose, out[1][i], out[2][i]
                per["emotion_prediction"][row], per["text_embedding"][row] = out[3][i], out[4][i]
                prior[u] = pose[H_:]
    res = {k: torch.stack(v) for k, v in per.items()}
    res["track"] = track
    return res


def rows_of(wp, u):
    off = sum(wp[:u])
    return slice(off, off + wp[u])


# ---- 1: the reference goldens already pin the ragged result ------------------------------------------------------------------------------
@pytest.mark.parametrize("wp", [(4, 2), (1, 4), (3, 4)])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_ragged_rollout_matches_reference_golden(name, prec, wp):
    """Recording u's window w within the fixture's free-running bar POSE_TOL * (1 + window_gain * sum_{i<w} handoff_gain^i) of the golden's
    window (u, w), whatever the other recording does; the track within its last window's bar of the stitch of the golden's first W_u windows;
    emotion_prediction within 5 x POSE_TOL; the track bitwise the stitch of the windows this call produced.  Inputs go in padded."""
    z, m, inp, sampled = load_case(name)
    model = model_for(CASES[name], prec, m["seed"])
    hg, wg = float(z["handoff_gain"]), float(z["window_gain"])
    Wmax = max(wp)
    cut = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, :Wmax])).to(dev())
    out = model.synthesize(cut(inp["spec"]), cut(inp["text"]), torch.from_numpy(inp["seed_pose"]).to(dev()),
                           None if sampled is None else cut(sampled.numpy()), want_windows=True, windows_per=wp)
    torch.cuda.synchronize()
    win, track, pred = out["windows"].cpu().numpy(), out["track"].cpu().numpy(), out["emotion_prediction"].cpu().numpy()
    H, P = m["frames"] - m["prior"], m["prior"]
    assert win.shape == (sum(wp), m["frames"], m["pose_dim"]) and track.shape == (2, Wmax * H + P, m["pose_dim"])
    assert out["track_frames"].tolist() == [w * H + P for w in wp] and out["window_offsets"].tolist() == [0, wp[0]]
    for u, W_u in enumerate(wp):
        rows = rows_of(wp, u)
        for w in range(W_u):
            e, tol = clip_rel_l2(win[rows][w][None], z["windows"][u, w][None]), R.free_running_tol(POSE_TOL[prec], wg, hg, w)
            print(f"{name} {prec} {wp} recording {u} window {w}: rel-L2 {e:.2e} (tolerance {tol:.2e})")
            assert e < tol, (u, w, e, tol)
        T = W_u * H + P
        e = clip_rel_l2(track[u:u + 1, :T], R.stitch(z["windows"][u:u + 1, :W_u], P))
        print(f"{name} {prec} {wp} recording {u} track: rel-L2 {e:.2e}")
        assert e < R.free_running_tol(POSE_TOL[prec], wg, hg, W_u - 1)
        assert rel_l2(pred[rows], z["emotion_prediction"][u, :W_u]) < POSE_TOL[prec] * 5
        assert np.array_equal(track[u:u + 1, :T], R.stitch(win[rows][None], P))       # same fp32 arithmetic on the host
        assert not track[u, T:].any()


# ---- 2: equal counts are the rectangular roll-out ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("U", [1, 2, 5])
@pytest.mark.parametrize("variant", ["spatial", "memory"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_equal_counts_are_the_rectangular_rollout(prec, variant, U, W):
    model = model_for(variant, prec)
    wp = (W,) * U
    g = inputs(wp, seed=30 + U * 4 + W, with_sampled=True)
    p = g["pad"]
    want = model.synthesize(p["spec"], p["text"], g["seed_pose"], p["sampled"], want_windows=True, want_aux=True)
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True, want_aux=True, windows_per=wp)
    torch.cuda.synchronize()
    assert torch.equal(got["track"], want["track"])
    for k in PER_WINDOW:
        assert torch.equal(got[k], want[k].reshape((U * W,) + tuple(want[k].shape[2:]))), k
    assert got["track_frames"].tolist() == [W * H_ + P_] * U


# ---- 3: against the loop of forward() calls on the active rows -----------------------------------------------------------------------------
LOOP_VECTORS = [(5, 3, 2), (1, 2, 4), (3, 1, 3, 2, 1), (1, 9, 1, 2), (4,), (1, 1, 1), (1,)]


@pytest.mark.parametrize("with_sampled", [False, True])
@pytest.mark.parametrize("wp", LOOP_VECTORS)
@pytest.mark.parametrize("variant", ["spatial", "memory"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_ragged_equals_loop_on_active_rows(prec, variant, wp, with_sampled):
    """Every window within POSE_TOL of the loop's.  Bit for bit in f32, and in bf16x3 for every window of a step with two or more active
    recordings (the products accumulate K in one order whatever the batch); a step with ONE active recording takes the one-clip split-K of
    w_2 in the loop's encoder while phase A, at batch N >= 2, does not: there, equal to rounding only."""
    model = model_for(variant, prec)
    g = inputs(wp, seed=90 + len(wp) * 7 + sum(wp), with_sampled=with_sampled)
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"], wp, g["sampled"])
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True, windows_per=wp)
    torch.cuda.synchronize()
    N, sb = sum(wp), RR.plan(wp)["step_batch"]
    exact_steps = len(sb) if prec == "f32" or N == 1 else int((sb >= 2).sum())         # step_batch is non-increasing
    worst = 0.0
    for u, W_u in enumerate(wp):
        rows = rows_of(wp, u)
        for w in range(W_u):
            a, b = got["windows"][rows][w], want["windows"][rows][w]
            worst = max(worst, clip_rel_l2(a[None].cpu().numpy(), b[None].cpu().numpy()))
            if w < exact_steps:
                assert torch.equal(a, b), (u, w)
                assert torch.equal(got["emotion_prediction"][rows][w], want["emotion_prediction"][rows][w]), (u, w)
        T = W_u * H_ + P_
        assert clip_rel_l2(got["track"][u:u + 1, :T].cpu().numpy(), want["track"][u:u + 1, :T].cpu().numpy()) < POSE_TOL[prec]
        if W_u <= exact_steps:
            assert torch.equal(got["track"][u], want["track"][u]), u        # tail included: the loop's buffer starts as zeros
        assert not got["track"][u, T:].any()
    print(f"{prec} {variant} {wp} sampled={with_sampled}: worst per-window rel-L2 {worst:.2e}, bitwise through step {exact_steps} of {len(sb)}")
    assert worst < POSE_TOL[prec]
    assert rel_l2(got["emotion_prediction"].cpu().numpy(), want["emotion_prediction"].cpu().numpy()) < POSE_TOL[prec] * 5


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_alpha_windows_and_aux_equal_the_loop(variant):
    model = model_for(variant, "bf16x3")
    wp = (3, 2, 3)                                   # two or more active recordings in every step: everything bit for bit
    g = inputs(wp, seed=52, with_sampled=False)
    alpha = torch.tensor([0.9, 0.5, 0.25, 0.0], device=dev())
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"], wp, None, alpha)
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], None, alpha=alpha, want_windows=True, want_aux=True, windows_per=wp)
    for k in ("track",) + PER_WINDOW:
        assert got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k
    plain = model.synthesize(g["spec"], g["text"], g["seed_pose"], windows_per=wp)
    assert set(plain) == {"track", "track_frames", "window_offsets", "emotion_prediction"}
    assert torch.equal(plain["emotion_prediction"], got["emotion_prediction"])
    only_windows = model.synthesize(g["spec"], g["text"], g["seed_pose"], windows_per=wp, want_windows=True)
    assert set(only_windows) == set(plain) | {"windows"} and torch.equal(only_windows["track"], plain["track"])
    # the overlap rows differ from the default blend, everything else does not (the hand-off never sees alpha)
    ov = torch.zeros(3 * H_ + P_, dtype=torch.bool)
    for w in range(1, 3):
        ov[w * H_: w * H_ + P_] = True
    assert torch.equal(plain["track"][:, ~ov], got["track"][:, ~ov]) and not torch.equal(plain["track"][0, ov], got["track"][0, ov])
    # alpha = 0 on the last overlap frame: the old window's raw frame
    assert torch.equal(got["track"][2, H_ + 3], got["windows"][rows_of(wp, 2)][0, H_ + 3])


def test_fold_affine_ragged_equals_its_loop():
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision="bf16x3")
    model.fold_affine = True
    model.to(dev())
    wp = (2, 3, 3)
    g = inputs(wp, seed=61, with_sampled=False)
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"], wp)
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], want_windows=True, windows_per=wp)
    assert torch.equal(got["windows"], want["windows"]) and torch.equal(got["track"], want["track"])


# ---- 4: a recording of a ragged call is that recording alone (spatial: rows are independent) --------------------------------------------------
def test_spatial_recording_equals_its_own_synthesize():
    model = model_for("spatial", "f32")
    wp = (2, 4, 1, 3)
    g = inputs(wp, seed=120, with_sampled=True)
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True, windows_per=wp)
    for u, W_u in enumerate(wp):
        p = g["pad"]
        alone = model.synthesize(p["spec"][u:u + 1, :W_u].contiguous(), p["text"][u:u + 1, :W_u].contiguous(), g["seed_pose"][u:u + 1],
                                 p["sampled"][u:u + 1, :W_u].contiguous(), want_windows=True)
        T = W_u * H_ + P_
        assert torch.equal(got["track"][u, :T], alone["track"][0]), u
        assert torch.equal(got["windows"][rows_of(wp, u)], alone["windows"][0]), u
        assert torch.equal(got["emotion_prediction"][rows_of(wp, u)], alone["emotion_prediction"][0]), u


# ---- 5: nothing of an inactive recording enters a step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["spatial", "memory"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_padding_past_a_recordings_end_is_never_read(prec, variant):
    """Padded [U, Wmax, ...] inputs whose entries past W_u are NaN give the packed call's outputs bit for bit, all finite."""
    model = model_for(variant, prec)
    wp = (2, 4, 1, 3)
    g = inputs(wp, seed=130, with_sampled=True)
    p = {k: (None if v is None else v.clone()) for k, v in g["pad"].items()}
    for u, W_u in enumerate(wp):
        p["spec"][u, W_u:] = float("nan")
        p["sampled"][u, W_u:] = float("nan")
        p["text"][u, W_u:] = 1                      # a valid word index: the text branch reads indices, not values
    run = lambda a, b, c: model.synthesize(a, b, g["seed_pose"], c, want_windows=True, want_aux=True, windows_per=wp)
    want, got = run(g["spec"], g["text"], g["sampled"]), run(p["spec"], p["text"], p["sampled"])
    torch.cuda.synchronize()
    for k in ("track",) + PER_WINDOW:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]), k


def test_track_tails_are_zero_written_by_the_library():
    model = model_for("memory", "bf16x3")
    wp = (2, 5, 1, 5, 3)
    g = inputs(wp, seed=140, with_sampled=False)
    eng = model.engine()
    buf = torch.full((len(wp), max(wp) * H_ + P_, D_), float("nan"), device=dev())
    out = eng.forward_rollout_ragged(g["spec"], g["text"], g["seed_pose"], wp, track=buf)
    torch.cuda.synchronize()
    assert out["track"] is buf
    for u, W_u in enumerate(wp):
        T = W_u * H_ + P_
        assert out["track_frames"][u] == T
        assert bool(torch.isfinite(buf[u, :T]).all()) and bool(buf[u, :T].any()), u
        assert buf[u, T:].numel() == (max(wp) - W_u) * H_ * D_ and not bool((buf[u, T:] != 0).any()), u       # exactly zero, no NaN left
    assert torch.equal(eng.forward_rollout_ragged(g["spec"], g["text"], g["seed_pose"], wp)["track"], buf)
    with pytest.raises(L.EgError, match="track: need"):
        eng.forward_rollout_ragged(g["spec"], g["text"], g["seed_pose"], wp, track=buf[:, :-1])


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_caller_order_is_kept(prec):
    """Permuting the recordings of a call permutes its outputs and changes nothing else (spatial: rows are independent)."""
    model = model_for("spatial", prec)
    wp = (3, 1, 4, 2)
    g = inputs(wp, seed=150, with_sampled=True)
    base = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True, want_aux=True, windows_per=wp)
    perm = [2, 0, 3, 1]
    wq = tuple(wp[u] for u in perm)
    take = lambda t: torch.cat([t[rows_of(wp, u)] for u in perm])
    got = model.synthesize(take(g["spec"]), take(g["text"]), g["seed_pose"][perm].contiguous(), take(g["sampled"]), want_windows=True, want_aux=True,
                           windows_per=wq)
    assert torch.equal(got["track"], base["track"][perm]) and got["track_frames"].tolist() == [base["track_frames"][u].item() for u in perm]
    for k in PER_WINDOW:
        assert torch.equal(got[k], take(base[k])), k


# ---- 6: raw audio ---------------------------------------------------------------------------------------------------------------------
LENGTHS = [2 * HOP + NS - 9000, 2 * HOP, HOP + 500]          # 4, 2 and 2 windows: a short last window, an exact multiple of hop, a 500-sample stub


def raw_audio(seed):
    U, stride = len(LENGTHS), max(LENGTHS)
    audio = synth_audio(U, stride, seed=seed)
    wp = [-(-T // HOP) for T in LENGTHS]
    return audio, wp


def test_harness_synthesize_with_lengths_from_raw_audio():
    """harness.synthesize(lengths=) == MelFrontEnd on explicit numpy slices (np.pad mode="symmetric" on each recording's OWN samples) +
    forward_rollout_ragged, bit for bit; samples past lengths[u] set to NaN change nothing."""
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd.engine import MelFrontEnd
    model, vae = model_for("spatial", "bf16x3"), vae_for()
    audio, wp = raw_audio(80)
    assert wp == [4, 2, 2]
    U, N = len(wp), sum(wp)
    clips = np.stack([np.pad(audio[u, w * HOP: min(w * HOP + NS, LENGTHS[u])], (0, max(0, w * HOP + NS - LENGTHS[u])), mode="symmetric")
                      for u in range(U) for w in range(wp[u])])
    assert clips.shape == (N, NS)
    g = inputs(tuple(wp), seed=80, with_sampled=False)
    mel = MelFrontEnd(dev())
    spec = mel(torch.from_numpy(clips).to(dev()), out_frames=124)
    poisoned = torch.from_numpy(audio).to(dev())
    for u, T in enumerate(LENGTHS):
        poisoned[u, T:] = float("nan")
    got_spec, got_wp = mel.windows_ragged(poisoned, LENGTHS, HOP, NS, out_frames=124)
    assert got_wp == wp and torch.equal(got_spec, spec)
    with torch.no_grad():
        sampled = vae.sample(g["label"], z=g["z"])
    want = model.engine().forward_rollout_ragged(spec, g["text"], g["seed_pose"], wp, sampled, want_windows=True)
    p = g["pad"]
    for a in (torch.from_numpy(audio).to(dev()), poisoned):
        for text, labels, z in ((p["text"], p["label"], p["z"]), (g["text"], g["label"], g["z"])):         # padded and packed
            got = Hs.synthesize((model, vae), a, text, g["seed_pose"], labels=labels, hop_samples=HOP, z=z, want_windows=True, lengths=LENGTHS, mel=mel)
            assert got["windows_per"] == wp and torch.equal(got["spec"], spec)
            for k in want:
                assert torch.equal(got[k], want[k]), k
            assert bool(torch.isfinite(got["track"]).all())
    assert tuple(want["track"].shape) == (U, 4 * H_ + P_, D_) and want["track_frames"].tolist() == [w * H_ + P_ for w in wp]
    with pytest.raises(L.EgError, match=r"lengths\[1\]=0"):
        mel.windows_ragged(poisoned, [5, 0, 7], HOP, NS)
    with pytest.raises(L.EgError, match=r"lengths\[2\]="):
        mel.windows_ragged(poisoned, [5, 6, poisoned.shape[1] + 1], HOP, NS)


def test_stream_rows_ending_at_their_own_lengths_are_the_ragged_tracks():
    """include/emogest.h: a stream row's emitted rows followed by its tail are the roll-out's track for that recording -- here for rows that end
    at different lengths (f32, spatial: bit for bit)."""
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd import streaming as S
    from emotiongestures_amd.engine import MelFrontEnd
    model, vae, mel = model_for("spatial", "f32"), vae_for(), MelFrontEnd(dev())
    audio, wp = raw_audio(81)
    U, Wmax = len(wp), max(wp)
    g = inputs(tuple(wp), seed=81, with_sampled=False)
    p = g["pad"]
    a = torch.from_numpy(audio).to(dev())
    want = Hs.synthesize((model, vae), a, p["text"], g["seed_pose"], labels=p["label"], hop_samples=HOP, z=p["z"], lengths=LENGTHS, mel=mel)
    s = Hs.open_stream((model, vae), U, g["seed_pose"], mel=mel, hop_samples=HOP)
    steps = max(-(-T // HOP) for T in LENGTHS) + s.lag
    plans = [S.plan(HOP, NS, T, steps) for T in LENGTHS]
    assert [sum(i["valid"] for i in pl) for pl in plans] == wp                  # streaming and offline count the same windows
    padded = torch.zeros(U, steps * HOP, device=dev())
    for u, T in enumerate(LENGTHS):
        padded[u, :T] = a[u, :T]
    emitted = [[] for _ in range(U)]
    for k in range(1, steps + 1):
        col = [plans[u][k - 1]["w"] if plans[u][k - 1]["valid"] else 0 for u in range(U)]
        pick = lambda t: torch.stack([t[u, col[u]] for u in range(U)])
        ends = [T - (k - 1) * HOP if (k - 1) * HOP < T <= k * HOP else -1 for T in LENGTHS]
        r, v = s.push(padded[:, (k - 1) * HOP: k * HOP].contiguous(), pick(p["text"]), pick(p["label"]), pick(p["z"]), ends=ends)
        assert v.cpu().tolist() == [int(plans[u][k - 1]["valid"]) for u in range(U)], k
        for u in range(U):
            if plans[u][k - 1]["valid"]:
                emitted[u].append(r[u])
    tail = s.tail()
    for u in range(U):
        T = int(want["track_frames"][u])
        assert torch.equal(torch.cat(emitted[u] + [tail[u]], 0), want["track"][u, :T]), u


# ---- 7: one graph ---------------------------------------------------------------------------------------------------------------------
def test_ragged_rollout_is_capturable_in_one_graph():
    """Captured once for a fixed (W_u), replayed three times with fresh inputs copied into the static buffers: bitwise the eager call on those
    inputs.  The capture enqueues exactly the launches of an eager call, and a replay makes no library launch on the host."""
    lib = L.load()
    model = model_for("memory", "bf16x3")
    wp = (3, 1, 2)
    keys = ("spec", "text", "seed_pose", "sampled")
    static = inputs(wp, seed=70, with_sampled=True)
    run = lambda g: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], want_windows=True, want_aux=True, windows_per=wp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)                         # workspace, plan table, weight arena: outside the capture
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
    print(f"ragged roll-out {wp}: N={sum(wp)} Wmax={max(wp)}: {eager_launches} launches per call")
    for r in range(3):
        fresh = inputs(wp, seed=71 + r, with_sampled=True)
        for k in keys:
            static[k].copy_(fresh[k])
        n0 = lib.eg_launch_count()
        graph.replay()
        torch.cuda.synchronize()
        assert lib.eg_launch_count() == n0
        got = {k: v.clone() for k, v in out.items()}
        want = run(fresh)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(got[k], want[k]), (r, k)
