"""Takes roll-out on the GPU (eg_generator_forward_rollout_takes through GeneratorEngine.forward_rollout_takes / Transformer.synthesize_takes /
harness.synthesize_takes) against its definition: the ragged roll-out on the U*R replicated recordings, same device and precision -- and
against the two calls it generalises, the rectangular diverse call (equal counts) and the ragged call (one draw)."""
import numpy as np
import pytest
import torch

import rollout_draws_np as RD
import rollout_np as R
import rollout_ragged_np as RR
import rollout_takes_np as RT
from conftest import build_mirror, clip_rel_l2, rel_l2
from emotiongestures_amd import _lib as L
from emotiongestures_amd.synth import hash_uniform, load_synth_weights, synth_audio

pytestmark = pytest.mark.gpu

POSE_TOL = {"f32": 2e-5, "bf16x3": 1e-3}        # tests/test_gpu_generator.py:15
F_, D_, P_ = 34, 126, 4
H_ = F_ - P_
HOP, NS = 32000, (124 - 1) * 512
AUX = ("emotion_prediction", "emotion_feature", "semantic_feature", "text_embedding")
HOST = ("track_frames", "window_offsets", "take_window_offsets")
_MODELS, _VAES = {}, {}


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


def pack_takes(padded, wp, Rd):
    """[U, R, Wmax, ...] -> packed [N*R, ...] in the take order: window w of draw r of recording u at row R*off[u] + r*W_u + w."""
    a = np.asarray(padded)
    return RR.pack(a.reshape((len(wp) * Rd,) + a.shape[2:]), RT.repeat(wp, Rd))


def inputs(wp, Rd, seed):
    """Padded [U, Wmax, ...] inputs from the fixtures' generator with sampled [U, R, Wmax, F, 512], and their packed forms, on the device."""
    U, Wmax = len(wp), max(wp)
    inp = R.rollout_inputs(U, Wmax, F_, D_, P_, seed=seed)
    sampled = RD.hash_sampled((U, Rd, Wmax, F_, 512), seed, amplitude=1.0).numpy()
    g = {"seed_pose": torch.from_numpy(inp["seed_pose"]).to(dev()), "pad": {"sampled": torch.from_numpy(sampled).to(dev())},
         "sampled": torch.from_numpy(pack_takes(sampled, wp, Rd)).to(dev())}
    for k in ("spec", "text"):
        g["pad"][k] = torch.from_numpy(inp[k]).to(dev())
        g[k] = torch.from_numpy(RR.pack(inp[k], wp)).to(dev())
    return g


def replicated(model, g, wp, Rd, **kw):
    """The definition, as the library offered it before: the ragged synthesize on the U*R replicated recordings, folded back -- track
    [U, R, T, D], windows in the replicated call's packed order (the takes call's own), the outputs that do not depend on the draw checked
    to be the same in every draw's copy and returned once, packed [N, ...]."""
    U = len(wp)
    out = model.synthesize(*RT.replicate_ragged(g["spec"], g["text"], g["seed_pose"], wp, g["sampled"]), windows_per=RT.repeat(wp, Rd), **kw)
    res = {"track": out["track"].reshape((U, Rd) + tuple(out["track"].shape[1:]))}
    if "windows" in out:
        res["windows"] = out["windows"]
    tr = RT.take_rows(wp, Rd)
    first = torch.as_tensor(RT.first_take_rows(wp, Rd), device=dev())
    for k in AUX:
        if k in out:
            for u in range(U):
                for r in range(1, Rd):
                    assert torch.equal(out[k][tr[u, r]: tr[u, r] + wp[u]], out[k][tr[u, 0]: tr[u, 0] + wp[u]]), (k, u, r)
            res[k] = out[k][first].contiguous()
    assert out["track_frames"].view(U, Rd)[:, 0].tolist() == [w * H_ + P_ for w in wp]
    return res


# ---- 1: against the replicated ragged roll-out -------------------------------------------------------------------------------------
CASES = [((3, 1, 2), 2),            # working order != caller order, a recording that ends at step 0
         ((1, 4, 4, 2, 1), 4),      # ties; U*R = 20 > N = 12: the prior encoder's buffers are taken again
         ((4, 3, 1), 5),            # U*R < N; R no multiple of 4: the unrolled draws loop and its remainder both run
         ((1,), 3)]                 # N = 1


@pytest.mark.parametrize("wp,Rd", CASES)
@pytest.mark.parametrize("variant", ["spatial", "memory"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_takes_equal_the_replicated_ragged_rollout(prec, variant, wp, Rd):
    """Everything within POSE_TOL (emotion_prediction 5 x, as tests/test_gpu_rollout_draws.py) of the ragged synthesize on the replicated
    recordings.  Fusion, encoder, K|V and the decoder steps run at the same batch and row order in both calls and the tower-side products
    accumulate K in one order from two clips up, so with N >= 2 the results are equal bit for bit: asserted.  With N == 1 the tower side
    takes the one-clip paths (the split-K of w_2, the one-clip convolution tiles) where the replicated call has R clips: equal to rounding
    only, the cause test_draws_equal_the_replicated_rollout names for its (1, 1, 3), and held to POSE_TOL (measured on MI355X at (1,) x 3,
    both variants: bitwise in f32; in bf16x3 windows and track 1.4e-5 per-clip relative L2, emotion_prediction 5.3e-6, features 3.7e-6,
    text_embedding 1.9e-7)."""
    U, N = len(wp), sum(wp)
    model = model_for(variant, prec)
    g = inputs(wp, Rd, seed=300 + 16 * U + 4 * N + Rd)
    want = replicated(model, g, wp, Rd, want_windows=True, want_aux=True)
    got = model.synthesize_takes(g["spec"], g["text"], g["seed_pose"], g["sampled"], windows_per=wp, draws=Rd, want_windows=True, want_aux=True)
    torch.cuda.synchronize()
    assert set(got) == set(want) | set(HOST) and set(want) == {"track", "windows"} | set(AUX)
    assert tuple(got["track"].shape) == (U, Rd, max(wp) * H_ + P_, D_) and tuple(got["windows"].shape) == (N * Rd, F_, D_)
    assert tuple(got["emotion_prediction"].shape) == (N, 8) and tuple(got["semantic_feature"].shape) == (N, F_, 512)
    assert tuple(got["text_embedding"].shape) == (N, 60, 512)
    assert got["track_frames"].tolist() == [w * H_ + P_ for w in wp] and got["window_offsets"].tolist() == RR.plan(wp)["offsets"].tolist()
    assert got["take_window_offsets"].tolist() == RT.take_rows(wp, Rd).tolist()
    bitwise = {k: torch.equal(got[k], want[k]) for k in sorted(want)}
    worst = max(clip_rel_l2(got["windows"][i:i + 1].cpu().numpy(), want["windows"][i:i + 1].cpu().numpy()) for i in range(N * Rd))
    e_track = clip_rel_l2(got["track"].reshape(U * Rd, -1, D_).cpu().numpy(), want["track"].reshape(U * Rd, -1, D_).cpu().numpy())
    e_aux = {k: rel_l2(got[k].cpu().numpy(), want[k].cpu().numpy()) for k in AUX}
    print(f"{prec} {variant} wp={wp} R={Rd}: bitwise {bitwise}; windows worst per-clip rel-L2 {worst:.2e}, track {e_track:.2e}, "
          + ", ".join(f"{k} {v:.2e}" for k, v in e_aux.items()))
    assert worst < POSE_TOL[prec] and e_track < POSE_TOL[prec]
    assert e_aux["emotion_prediction"] < POSE_TOL[prec] * 5
    for k in ("emotion_feature", "semantic_feature", "text_embedding"):
        assert e_aux[k] < POSE_TOL[prec], k
    if N >= 2:
        for k in sorted(want):
            assert bitwise[k], k


# ---- 2: equal counts are the rectangular diverse call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("UWR", [(2, 3, 3), (1, 3, 2)])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_equal_counts_are_the_rectangular_diverse_call(prec, UWR):
    U, W, Rd = UWR
    wp = (W,) * U
    model = model_for("memory", prec)
    g = inputs(wp, Rd, seed=340 + 16 * U + Rd)
    p = g["pad"]
    want = model.synthesize(p["spec"], p["text"], g["seed_pose"], p["sampled"], draws=Rd, want_windows=True, want_aux=True)
    for sampled in (g["sampled"], p["sampled"]):                 # packed and padded
        got = model.synthesize_takes(p["spec"], p["text"], g["seed_pose"], sampled, windows_per=wp, draws=Rd, want_windows=True, want_aux=True)
        torch.cuda.synchronize()
        assert torch.equal(got["track"], want["track"])
        assert torch.equal(got["windows"], want["windows"].reshape(U * Rd * W, F_, D_))
        for k in AUX:
            assert torch.equal(got[k], want[k].reshape((U * W,) + tuple(want[k].shape[2:]))), k


# ---- 3: one draw is the ragged call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wp", [(3, 1, 2), (1,), (4,)])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_one_draw_is_the_ragged_rollout_launch_for_launch(prec, wp):
    lib = L.load()
    U = len(wp)
    model = model_for("memory", prec)
    g = inputs(wp, 1, seed=360 + sum(wp))
    run_a = lambda: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], windows_per=wp, want_windows=True, want_aux=True)
    run_b = lambda: model.synthesize_takes(g["spec"], g["text"], g["seed_pose"], g["sampled"], windows_per=wp, draws=1, want_windows=True,
                                           want_aux=True)
    run_a(), run_b()                                 # workspaces, plan tables, weight arena
    n0 = lib.eg_launch_count()
    want = run_a()
    n1 = lib.eg_launch_count()
    got = run_b()
    n2 = lib.eg_launch_count()
    torch.cuda.synchronize()
    assert n2 - n1 == n1 - n0 > 0
    assert set(got) == set(want) | {"take_window_offsets"}
    for k in want:
        assert torch.equal(got[k], want[k].reshape(got[k].shape)), k
    assert tuple(got["track"].shape) == (U, 1, max(wp) * H_ + P_, D_) and got["take_window_offsets"][:, 0].tolist() == got["window_offsets"].tolist()


# ---- 4: the draws are indexed by recording ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_permuting_the_draws_of_one_recording_permutes_its_tracks_only(prec):
    """Spatial variant (its rows are independent): recording 1's tracks and windows follow its sampled maps bit for bit, the other
    recordings keep their bits -- an index error in the fusion kernel that the replicated comparison shared with its helper would show here."""
    model = model_for("spatial", prec)
    wp, Rd = (2, 3, 1), 3
    g = inputs(wp, Rd, seed=371)
    perm = [2, 0, 1]
    moved = g["pad"]["sampled"].clone()
    moved[1] = g["pad"]["sampled"][1][perm]
    run = lambda s: model.synthesize_takes(g["spec"], g["text"], g["seed_pose"], s, windows_per=wp, draws=Rd, want_windows=True)
    a, b = run(g["pad"]["sampled"]), run(moved)
    torch.cuda.synchronize()
    tr = a["take_window_offsets"]
    win = lambda o, u, r: o["windows"][int(tr[u, r]): int(tr[u, r]) + wp[u]]
    for u in (0, 2):
        assert torch.equal(b["track"][u], a["track"][u])
        assert all(torch.equal(win(b, u, r), win(a, u, r)) for r in range(Rd))
    for r in range(Rd):
        assert torch.equal(b["track"][1, r], a["track"][1, perm[r]]) and torch.equal(win(b, 1, r), win(a, 1, perm[r]))
    assert torch.equal(b["emotion_prediction"], a["emotion_prediction"])
    assert not torch.equal(a["track"][1, 0], a["track"][1, 1]) and not torch.equal(a["track"][0, 0], a["track"][0, 1])      # different takes


# ---- 5: tails and padding ------------------------------------------------------------------------------------------------------------------
def test_track_tails_are_zero_written_by_the_library():
    model = model_for("memory", "bf16x3")
    wp, Rd = (2, 4, 1), 2
    g = inputs(wp, Rd, seed=380)
    eng = model.engine()
    buf = torch.full((len(wp), Rd, max(wp) * H_ + P_, D_), float("nan"), device=dev())
    out = eng.forward_rollout_takes(g["spec"], g["text"], g["seed_pose"], wp, g["sampled"], track=buf)
    torch.cuda.synchronize()
    assert out["track"] is buf and bool(torch.isfinite(buf).all())
    for u, W_u in enumerate(wp):
        T = W_u * H_ + P_
        assert out["track_frames"][u] == T
        for r in range(Rd):
            assert bool(buf[u, r, :T].any()), (u, r)
            assert buf[u, r, T:].numel() == (max(wp) - W_u) * H_ * D_ and not bool((buf[u, r, T:] != 0).any()), (u, r)     # exactly zero
    assert torch.equal(eng.forward_rollout_takes(g["spec"], g["text"], g["seed_pose"], wp, g["sampled"])["track"], buf)
    with pytest.raises(L.EgError, match="track: need"):
        eng.forward_rollout_takes(g["spec"], g["text"], g["seed_pose"], wp, g["sampled"], track=buf[:, :1])


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_padding_past_a_recordings_end_is_never_read(variant):
    """Padded inputs whose entries past W_u are NaN (spec, sampled; text is int64: another valid word index) give the results of the same
    call with those entries zeroed, bit for bit, and the packed call's."""
    model = model_for(variant, "bf16x3")
    wp, Rd = (2, 4, 1), 3
    g = inputs(wp, Rd, seed=390)
    zero = {k: v.clone() for k, v in g["pad"].items()}
    nan = {k: v.clone() for k, v in g["pad"].items()}
    for u, W_u in enumerate(wp):
        zero["spec"][u, W_u:], zero["sampled"][u, :, W_u:], zero["text"][u, W_u:] = 0, 0, 0
        nan["spec"][u, W_u:], nan["sampled"][u, :, W_u:], nan["text"][u, W_u:] = float("nan"), float("nan"), 1
    run = lambda a: model.synthesize_takes(a["spec"], a["text"], g["seed_pose"], a["sampled"], windows_per=wp, draws=Rd, want_windows=True,
                                           want_aux=True)
    want, got, packed = run(zero), run(nan), run(g)
    torch.cuda.synchronize()
    for k in ("track", "windows") + AUX:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]) and torch.equal(got[k], packed[k]), k


# ---- 6: the track is the stitch of its windows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_track_is_the_stitch_of_its_windows_per_take(variant):
    model = model_for(variant, "bf16x3")
    wp, Rd = (3, 1, 2), 3
    g = inputs(wp, Rd, seed=400)
    alpha = torch.tensor([0.9, 0.5, 0.25, 0.0], device=dev())
    for a in (None, alpha):
        out = model.synthesize_takes(g["spec"], g["text"], g["seed_pose"], g["sampled"], windows_per=wp, draws=Rd, alpha=a, want_windows=True)
        torch.cuda.synchronize()
        win, track, tr = out["windows"].cpu().numpy(), out["track"].cpu().numpy(), out["take_window_offsets"].numpy()
        for u, W_u in enumerate(wp):
            for r in range(Rd):
                want = R.stitch(win[None, tr[u, r]: tr[u, r] + W_u], P_, None if a is None else a.cpu().numpy())[0]
                assert np.array_equal(track[u, r, : W_u * H_ + P_], want), (u, r)
    plain = model.synthesize_takes(g["spec"], g["text"], g["seed_pose"], g["sampled"], windows_per=wp, draws=Rd)
    assert set(plain) == {"track", "emotion_prediction"} | set(HOST)


# ---- 7: one graph ---------------------------------------------------------------------------------------------------------------------
def test_takes_rollout_is_capturable_in_one_graph():
    """Captured once for a fixed (W_u) and R, replayed twice with fresh inputs copied into the static buffers: bitwise the eager call on those
    inputs.  The capture enqueues exactly the launches of an eager call, and a replay makes no library launch on the host."""
    lib = L.load()
    model = model_for("memory", "bf16x3")
    wp, Rd = (3, 1, 2), 2
    keys = ("spec", "text", "seed_pose", "sampled")
    static = inputs(wp, Rd, seed=410)
    run = lambda g: model.synthesize_takes(g["spec"], g["text"], g["seed_pose"], g["sampled"], windows_per=wp, draws=Rd, want_windows=True,
                                           want_aux=True)
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
    assert lib.eg_launch_count() - n0 == eager_launches > 0
    print(f"takes roll-out {wp} x {Rd}: {eager_launches} launches per call")
    for r in range(2):
        fresh = inputs(wp, Rd, seed=411 + r)
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


# ---- 8: from raw audio ---------------------------------------------------------------------------------------------------------------------
def same(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        assert torch.equal(v, b[k]) if isinstance(v, torch.Tensor) else v == b[k], k


def test_harness_synthesize_takes_from_raw_audio():
    """harness.synthesize_takes with fixed z == harness.synthesize(lengths=) on the recordings repeated R times with the matching z, bit for
    bit, for padded and packed labels / z / text; joints, rotations and the take diversity are the functions on its track with the
    per-recording frames; 48 kHz audio is resampling first and calling at 16 kHz."""
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd import resample as RS
    from emotiongestures_amd import skeleton as SK
    from emotiongestures_amd.takes import take_diversity
    import rotations_np as RN
    model, vae = model_for("spatial", "bf16x3"), vae_for()
    U, Rd = 2, 3
    lengths = [2 * HOP + 5000, HOP + 700]
    wp = (3, 2)
    N, Wmax = sum(wp), max(wp)
    audio = torch.from_numpy(synth_audio(U, max(lengths), seed=420)).to(dev())
    inp = R.rollout_inputs(U, Wmax, F_, D_, P_, seed=420)
    text, seed_pose = torch.from_numpy(inp["text"]).to(dev()), torch.from_numpy(inp["seed_pose"]).to(dev())
    labels = torch.from_numpy(inp["label"]).to(dev())                # [U, Wmax, 8]
    z = torch.from_numpy(hash_uniform("rollout_takes/z", (U, Rd, Wmax, 32), -2.0, 2.0, 420))
    rep = lambda x: x[:, None].expand((U, Rd) + tuple(x.shape[1:])).reshape((U * Rd,) + tuple(x.shape[1:])).contiguous()
    kw = dict(hop_samples=HOP, want_windows=True)
    want = Hs.synthesize((model, vae), rep(audio), rep(text), rep(seed_pose), labels=rep(labels), z=z.reshape(U * Rd, Wmax, 32),
                         lengths=[n for n in lengths for _ in range(Rd)], **kw)
    got = Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels, lengths=lengths, draws=Rd, z=z, **kw)
    torch.cuda.synchronize()
    assert got["windows_per"] == list(wp) and want["windows_per"] == list(RT.repeat(wp, Rd))
    assert tuple(got["track"].shape) == (U, Rd, Wmax * H_ + P_, D_) and tuple(got["spec"].shape) == (N, 128, 124)
    assert torch.equal(got["track"], want["track"].view(U, Rd, -1, D_)) and torch.equal(got["windows"], want["windows"])
    first = torch.as_tensor(RT.first_take_rows(wp, Rd), device=dev())
    assert torch.equal(got["spec"], want["spec"][first]) and torch.equal(got["emotion_prediction"], want["emotion_prediction"][first])
    assert not torch.equal(got["track"][:, 0], got["track"][:, 1]) and not bool(got["track"][1, :, wp[1] * H_ + P_:].any())
    # packed forms of text, labels and z; labels per take
    lab4 = labels[:, None].expand(U, Rd, Wmax, 8).contiguous()
    packed = Hs.synthesize_takes((model, vae), audio, torch.from_numpy(RR.pack(inp["text"], wp)).to(dev()), seed_pose,
                                 torch.from_numpy(pack_takes(lab4.cpu().numpy(), wp, Rd)).to(dev()), lengths=lengths, draws=Rd,
                                 z=torch.from_numpy(pack_takes(z.numpy(), wp, Rd)), **kw)
    same(packed, got)
    same(Hs.synthesize_takes((model, vae), audio, text, seed_pose, lab4, lengths=lengths, draws=Rd, z=z, **kw), got)
    one = Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels[:, 0].contiguous(), lengths=lengths, draws=Rd, z=z, **kw)
    full = Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels[:, :1].expand(U, Wmax, 8).contiguous(), lengths=lengths, draws=Rd, z=z, **kw)
    same(one, full)
    with pytest.raises(L.EgError, match="z shape"):
        Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels, lengths=lengths, draws=Rd, z=z.reshape(U * Rd, Wmax, 32), **kw)
    with pytest.raises(L.EgError, match="labels shape"):
        Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels[:1], lengths=lengths, draws=Rd, z=z, **kw)
    # joints, rotations, take diversity: the functions on the track with recording u's own frames
    sk, rest = SK.ted_expressive(), RN.random_rest(42, 7)
    fgd = load_synth_weights(Hs.MLP_Reconstruct(pose_dim=D_), 5).eval().to(dev())
    frames = [w * H_ + P_ for w in wp]
    post = Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels, lengths=lengths, draws=Rd, z=z, joints=sk, rotations=rest,
                               diversity=fgd, **kw)
    torch.cuda.synchronize()
    assert set(post) == set(got) | {"joints", "joint_frames", "rotations", "take_distance", "take_diversity"}
    same({k: post[k] for k in got}, got)
    j, jf = SK.joints_from_tracks(post["track"], sk, frames=frames)
    q, _n = SK.rotations_from_tracks(post["track"], sk, rest, frames=frames)
    assert tuple(post["joints"].shape) == (U, Rd, Wmax * H_ + P_, 43, 3) and tuple(post["rotations"].shape) == (U, Rd, Wmax * H_ + P_, 42, 4)
    assert torch.equal(post["joints"], j) and post["joint_frames"] == jf and torch.equal(post["rotations"], q)
    td = take_diversity(fgd, post["track"], frames=frames, span=F_)
    assert tuple(post["take_distance"].shape) == (U, Rd, Rd) and tuple(post["take_diversity"].shape) == (U,)
    assert torch.equal(post["take_distance"], td["distance"]) and torch.equal(post["take_diversity"], td["diversity"])
    assert bool(torch.isfinite(post["take_distance"]).all()) and bool((post["take_diversity"] > 0).all())
    # lengths=None: every row at full length
    full_len = Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels, lengths=None, draws=Rd, z=z, **kw)
    same(full_len, Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels, lengths=[audio.shape[1]] * U, draws=Rd, z=z, **kw))
    assert full_len["windows_per"] == [Wmax, Wmax]
    # 48 kHz: resampling first and calling at 16 kHz
    l48 = [3 * n for n in lengths]
    a48 = torch.from_numpy(synth_audio(U, max(l48), seed=421)).to(dev())
    got48 = Hs.synthesize_takes((model, vae), a48, text, seed_pose, labels, lengths=l48, draws=Rd, z=z, audio_rate=48000, **kw)
    a16 = RS.resample_audio(a48, 48000, lengths=l48)
    l16 = [RS.out_length(n, 48000) for n in l48]
    assert torch.equal(got48["audio"], a16) and got48["lengths"] == l16 and [-(-n // HOP) for n in l16] == list(wp)
    same({k: v for k, v in got48.items() if k not in ("audio", "lengths")},
         Hs.synthesize_takes((model, vae), a16, text, seed_pose, labels, lengths=l16, draws=Rd, z=z, **kw))


def test_harness_synthesize_takes_beat_scores_every_take_on_its_own_samples():
    """A BEAT-shaped generator (pose_dim >= 174): out["beat"] [U, R] is beat_alignment_tracks on the call's own audio, lengths, track and
    per-recording frames, bit for bit, and finite."""
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd.beat import beat_alignment_tracks
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    Fb, Db, Pb = 60, 282, 10
    Hb = Fb - Pb
    model = build_mirror("spatial", Fb, Db, Pb, 10, seed=31).to(dev())
    vae = load_synth_weights(MLP_Reconstruct_v3(), 31).eval().to(dev())
    U, Rd, hop = 2, 2, 53333
    lengths = [3 * hop - 100, hop + 700]                                        # 3 and 2 windows
    rng = np.random.default_rng(5)
    a = 0.05 * rng.standard_normal((U, max(lengths))).astype(np.float32)
    for k in range(0, max(lengths), 7000):                                      # bursts: onsets for the beat score
        a[:, k:k + 800] += rng.standard_normal((U, min(800, max(lengths) - k))).astype(np.float32)
    audio = torch.from_numpy(a).to(dev())
    inp = R.rollout_inputs(U, 3, Fb, Db, Pb, seed=120)
    text, seed_pose = torch.from_numpy(inp["text"]).to(dev()), torch.from_numpy(inp["seed_pose"]).to(dev())
    labels = torch.from_numpy(inp["label"]).to(dev())
    z = torch.from_numpy(hash_uniform("rollout_takes/z", (U, Rd, 3, 32), -2.0, 2.0, 121))
    kw = dict(lengths=lengths, draws=Rd, z=z, hop_samples=hop)
    plain = Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels, **kw)
    out = Hs.synthesize_takes((model, vae), audio, text, seed_pose, labels, beat=True, **kw)
    torch.cuda.synchronize()
    assert out["windows_per"] == [3, 2] and set(out) == set(plain) | {"beat"}
    same({k: out[k] for k in plain}, plain)
    frames = [w * Hb + Pb for w in out["windows_per"]]
    want = beat_alignment_tracks(audio, out["track"], lengths=lengths, frames=frames)
    assert out["beat"].shape == (U, Rd) and out["beat"].dtype == torch.float64 and bool(torch.isfinite(out["beat"]).all())
    assert np.array_equal(out["beat"].cpu().numpy().view(np.uint64), want.cpu().numpy().view(np.uint64))
