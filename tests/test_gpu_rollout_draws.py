"""Diverse roll-out on the GPU (eg_generator_forward_rollout_draws through GeneratorEngine.forward_rollout_draws /
Transformer.synthesize(draws=) / harness.synthesize(draws=)) against its definition: the plain roll-out on the U*R replicated
recordings, same device and precision -- and against the reference golden of the plain roll-out for draw 0."""
import numpy as np
import pytest
import torch

import rollout_draws_np as RD
import rollout_np as R
from conftest import build_mirror, clip_rel_l2, rel_l2
from emotiongestures_amd import _lib as L
from emotiongestures_amd.synth import synth_audio
from rollout_np import CASES, load_case

pytestmark = pytest.mark.gpu

POSE_TOL = {"f32": 2e-5, "bf16x3": 1e-3}        # tests/test_gpu_generator.py:15
F_, D_, P_ = 34, 126, 4
H_ = F_ - P_
AUX = ("emotion_prediction", "emotion_feature", "semantic_feature", "text_embedding")
_MODELS = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def model_for(variant, prec, seed=7):
    key = (variant, prec, seed)
    if key not in _MODELS:
        _MODELS[key] = build_mirror(variant, F_, D_, P_, 4, seed=seed, precision=prec).to(dev())
    return _MODELS[key]


def inputs(U, W, Rd, seed):
    inp = R.rollout_inputs(U, W, F_, D_, P_, seed=seed)
    g = {k: torch.from_numpy(inp[k]).to(dev()) for k in ("spec", "text", "seed_pose")}
    g["sampled"] = RD.hash_sampled((U, Rd, W, F_, 512), seed, amplitude=1.0).to(dev())
    return g


def replicated(model, g, **kw):
    """The definition, as the library offered it before: synthesize on the U*R replicated recordings, folded back to [U, R, ...]."""
    U, Rd = g["sampled"].shape[:2]
    out = model.synthesize(*RD.replicate(g["spec"], g["text"], g["seed_pose"], g["sampled"]), **kw)
    fold = lambda a: a.reshape((U, Rd) + tuple(a.shape[1:]))
    res = {k: fold(v) for k, v in out.items()}
    for k in AUX:                                   # independent of the draw: every draw's copy is the same
        if k in res:
            assert all(torch.equal(res[k][:, 0], res[k][:, r]) for r in range(Rd)), k
            res[k] = res[k][:, 0].contiguous()
    return res


# ---- against the replicated roll-out -------------------------------------------------------------------------------------
@pytest.mark.parametrize("UWR", [(1, 1, 3), (1, 3, 2), (2, 3, 3), (5, 2, 4)])
@pytest.mark.parametrize("variant", ["spatial", "memory"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_draws_equal_the_replicated_rollout(prec, variant, UWR):
    """Everything within POSE_TOL (emotion_prediction 5 x, as tests/test_gpu_rollout.py) of synthesize on the replicated recordings.  Fusion,
    encoder, K|V and the decoder steps run at the same batch in both calls and the tower-side products accumulate K in one order from two
    clips up, so with U*W >= 2 the results are equal bit for bit: asserted.  With U*W == 1 the tower side takes the one-clip paths where the
    replicated call has R clips: equal to rounding only (measured on MI355X at (1, 1, 3): bitwise in f32; in bf16x3 windows and track 1.5e-5
    per-clip relative L2, emotion_prediction 8.9e-6, features 3.6e-6, text_embedding 2.6e-6)."""
    U, W, Rd = UWR
    model = model_for(variant, prec)
    g = inputs(U, W, Rd, seed=100 + 16 * U + 4 * W + Rd)
    want = replicated(model, g, want_windows=True, want_aux=True)
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=Rd, want_windows=True, want_aux=True)
    torch.cuda.synchronize()
    assert set(got) == set(want) == {"track", "windows"} | set(AUX)
    assert tuple(got["track"].shape) == (U, Rd, W * H_ + P_, D_) and tuple(got["windows"].shape) == (U, Rd, W, F_, D_)
    assert tuple(got["emotion_prediction"].shape) == (U, W, 8) and tuple(got["semantic_feature"].shape) == (U, W, F_, 512)
    bitwise = {k: torch.equal(got[k], want[k]) for k in sorted(want)}
    worst = max(clip_rel_l2(got["windows"][:, r, w].cpu().numpy(), want["windows"][:, r, w].cpu().numpy()) for r in range(Rd) for w in range(W))
    e_track = clip_rel_l2(got["track"].reshape(U * Rd, -1, D_).cpu().numpy(), want["track"].reshape(U * Rd, -1, D_).cpu().numpy())
    e_aux = {k: rel_l2(got[k].cpu().numpy(), want[k].cpu().numpy()) for k in AUX}
    print(f"{prec} {variant} U={U} W={W} R={Rd}: bitwise {bitwise}; windows worst per-clip rel-L2 {worst:.2e}, track {e_track:.2e}, "
          + ", ".join(f"{k} {v:.2e}" for k, v in e_aux.items()))
    assert worst < POSE_TOL[prec] and e_track < POSE_TOL[prec]
    assert e_aux["emotion_prediction"] < POSE_TOL[prec] * 5
    for k in ("emotion_feature", "semantic_feature", "text_embedding"):
        assert e_aux[k] < POSE_TOL[prec], k
    if U * W >= 2:
        for k in sorted(want):
            assert bitwise[k], k


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("UW", [(1, 1), (3, 1), (1, 4), (2, 3)])
def test_one_draw_is_the_rollout_launch_for_launch(prec, UW):
    lib = L.load()
    U, W = UW
    model = model_for("memory", prec)
    g = inputs(U, W, 1, seed=140 + 4 * U + W)
    flat = g["sampled"][:, 0].contiguous()
    run_a = lambda: model.synthesize(g["spec"], g["text"], g["seed_pose"], flat, want_windows=True, want_aux=True)
    run_b = lambda: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=1, want_windows=True, want_aux=True)
    run_a(), run_b()                                 # workspaces, weight arena
    n0 = lib.eg_launch_count()
    want = run_a()
    n1 = lib.eg_launch_count()
    got = run_b()
    n2 = lib.eg_launch_count()
    torch.cuda.synchronize()
    assert n2 - n1 == n1 - n0 > 0
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k].reshape(got[k].shape)), k
    assert tuple(got["track"].shape) == (U, 1, W * H_ + P_, D_) and tuple(got["windows"].shape) == (U, 1, W, F_, D_)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_permuting_the_draws_permutes_the_tracks(prec):
    """Spatial variant (its rows are independent): the tracks follow their sampled maps bit for bit -- an index error in the fusion kernel
    that the replicated comparison shared with its helper would show here."""
    model = model_for("spatial", prec)
    U, W, Rd = 3, 3, 5
    g = inputs(U, W, Rd, seed=171)
    perm = torch.tensor([3, 0, 4, 1, 2], device=dev())
    a = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=Rd, want_windows=True)
    b = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"][:, perm], draws=Rd, want_windows=True)
    torch.cuda.synchronize()
    assert torch.equal(b["track"], a["track"][:, perm]) and torch.equal(b["windows"], a["windows"][:, perm])
    assert torch.equal(b["emotion_prediction"], a["emotion_prediction"])
    assert not torch.equal(a["track"][:, 0], a["track"][:, 1])          # the draws are different tracks
    # permuting the recordings moves everything with them
    up = torch.tensor([2, 0, 1], device=dev())
    c = model.synthesize(g["spec"][up], g["text"][up], g["seed_pose"][up], g["sampled"][up], draws=Rd)
    assert torch.equal(c["track"], a["track"][up]) and torch.equal(c["emotion_prediction"], a["emotion_prediction"][up])


# ---- against the reference golden -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_draw_zero_matches_reference_golden(prec):
    """Spatial fixture, R = 2: draw 0 is the fixture's own sampled map, draw 1 a hash-generated one (tests/test_rollout_draws.py shows the two
    stand more than 100 x the loosest bar apart).  Draw 0's windows and track stay within the fixture's free-running bars."""
    name = "rollout_ted_spatial"
    z, m, inp, sampled = load_case(name)
    model = model_for(CASES[name], prec, m["seed"])
    hg, wg = float(z["handoff_gain"]), float(z["window_gain"])
    both = torch.stack([sampled, RD.hash_sampled(sampled.shape, m["seed"])], 1).to(dev())
    out = model.synthesize(torch.from_numpy(inp["spec"]).to(dev()), torch.from_numpy(inp["text"]).to(dev()), torch.from_numpy(inp["seed_pose"]).to(dev()),
                           both, draws=2, want_windows=True)
    torch.cuda.synchronize()
    win = out["windows"].cpu().numpy()
    assert win[:, 0].shape == z["windows"].shape and tuple(out["track"][:, 0].shape) == z["track"].shape
    for w in range(m["W"]):
        e, tol = clip_rel_l2(win[:, 0, w], z["windows"][:, w]), R.free_running_tol(POSE_TOL[prec], wg, hg, w)
        print(f"{name} {prec} draw 0 window {w}: per-clip rel-L2 {e:.2e} (tolerance {tol:.2e})")
        assert e < tol, (w, e, tol)
    e = clip_rel_l2(out["track"][:, 0].cpu().numpy(), z["track"])
    print(f"{name} {prec} draw 0 track: per-clip rel-L2 {e:.2e}")
    assert e < R.free_running_tol(POSE_TOL[prec], wg, hg, m["W"] - 1)
    assert rel_l2(out["emotion_prediction"].cpu().numpy(), z["emotion_prediction"]) < POSE_TOL[prec] * 5
    apart = min(clip_rel_l2(win[u:u + 1, 1, w], win[u:u + 1, 0, w]) for u in range(m["U"]) for w in range(m["W"]))
    print(f"{name} {prec} draw 1 against draw 0: smallest per-clip rel-L2 {apart:.2e}")
    assert apart > 100 * R.free_running_tol(POSE_TOL["bf16x3"], wg, hg, m["W"] - 1)


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_track_is_the_stitch_of_the_windows_per_draw(variant):
    model = model_for(variant, "bf16x3")
    U, W, Rd = 2, 4, 3
    g = inputs(U, W, Rd, seed=181)
    alpha = torch.tensor([0.9, 0.5, 0.25, 0.0], device=dev())
    for a in (None, alpha):
        out = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=Rd, alpha=a, want_windows=True)
        torch.cuda.synchronize()
        win, track = out["windows"].cpu().numpy(), out["track"].cpu().numpy()
        for r in range(Rd):
            assert np.array_equal(track[:, r], R.stitch(win[:, r], P_, None if a is None else a.cpu().numpy())), r
    plain = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=Rd)
    assert set(plain) == {"track", "emotion_prediction"}


# ---- capture ------------------------------------------------------------------------------------------------------------------
def test_draws_rollout_is_capturable_in_one_graph():
    """Captured once, replayed with fresh inputs copied into the static buffers: bitwise the eager call on those inputs.  The capture enqueues
    exactly the launches of an eager call, a replay makes no library launch on the host, and the eager call makes at most one launch more
    than synthesize on the U*R replicated recordings (the seed broadcast; the fusion kernel stands for the swap of `sampled` and the add)."""
    lib = L.load()
    model = model_for("memory", "bf16x3")
    U, W, Rd = 2, 3, 3
    static = inputs(U, W, Rd, seed=190)
    run = lambda g: model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=Rd, want_windows=True, want_aux=True)
    rep = lambda g: model.synthesize(*RD.replicate(g["spec"], g["text"], g["seed_pose"], g["sampled"]), want_windows=True, want_aux=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static), rep(static)            # workspaces, weight arena: outside the capture
        n0 = lib.eg_launch_count()
        run(static)
        eager_launches = lib.eg_launch_count() - n0
        n0 = lib.eg_launch_count()
        rep(static)
        replicated_launches = lib.eg_launch_count() - n0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    print(f"draws roll-out U={U} W={W} R={Rd}: {eager_launches} launches, replicated synthesize at U*R: {replicated_launches}")
    assert 0 < eager_launches <= replicated_launches + 1
    graph = torch.cuda.CUDAGraph()
    n0 = lib.eg_launch_count()
    with torch.cuda.graph(graph):
        out = run(static)
    assert lib.eg_launch_count() - n0 == eager_launches
    for r in range(2):
        fresh = inputs(U, W, Rd, seed=191 + r)
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


def test_fold_affine_draws_equal_their_replicated_rollout():
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision="bf16x3")
    model.fold_affine = True
    model.to(dev())
    g = inputs(2, 3, 3, seed=201)
    want = replicated(model, g, want_windows=True)
    got = model.synthesize(g["spec"], g["text"], g["seed_pose"], g["sampled"], draws=3, want_windows=True)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---- from raw audio --------------------------------------------------------------------------------------------------------------
def test_harness_synthesize_draws_from_raw_audio():
    """harness.synthesize(draws=R) with fixed z == harness.synthesize on the audio replicated R times with z.reshape(U*R, W, 32), bit for bit;
    labels [U, R, W, 8] give each draw its own emotion and change the tracks."""
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.synth import hash_uniform, load_synth_weights
    model = model_for("spatial", "bf16x3")
    vae = load_synth_weights(MLP_Reconstruct_v3(frames=F_), 7).eval().to(dev())
    U, W, Rd = 2, 3, 3
    hop, n = 32000, (124 - 1) * 512
    total = 2 * hop + n - 9000                                       # the last window is 9000 samples short
    audio = torch.from_numpy(synth_audio(U, total, seed=210)).to(dev())
    inp = R.rollout_inputs(U, W, F_, D_, P_, seed=210)
    text, seed_pose = torch.from_numpy(inp["text"]).to(dev()), torch.from_numpy(inp["seed_pose"]).to(dev())
    labels = torch.from_numpy(inp["label"]).to(dev())                # [U, W, 8]
    z = torch.from_numpy(hash_uniform("rollout_draws/z", (U, Rd, W, 32), -2.0, 2.0, 210))
    rep = lambda x: x[:, None].expand((U, Rd) + tuple(x.shape[1:])).reshape((U * Rd,) + tuple(x.shape[1:])).contiguous()
    want = Hs.synthesize((model, vae), rep(audio), rep(text), rep(seed_pose), labels=rep(labels), hop_samples=hop, z=z.reshape(U * Rd, W, 32),
                         want_windows=True)
    got = Hs.synthesize((model, vae), audio, text, seed_pose, labels=labels, hop_samples=hop, z=z, want_windows=True, draws=Rd)
    torch.cuda.synchronize()
    assert tuple(got["track"].shape) == (U, Rd, W * H_ + P_, D_) and tuple(got["spec"].shape) == (U, W, 128, 124)
    assert torch.equal(got["spec"], want["spec"].view(U, Rd, W, 128, 124)[:, 0])
    assert torch.equal(got["track"], want["track"].view(U, Rd, -1, D_)) and torch.equal(got["windows"], want["windows"].view(U, Rd, W, F_, D_))
    assert torch.equal(got["emotion_prediction"], want["emotion_prediction"].view(U, Rd, W, 8)[:, 0])
    assert not torch.equal(got["track"][:, 0], got["track"][:, 1])
    # one label per recording is the same label for every window and draw
    one = Hs.synthesize((model, vae), audio, text, seed_pose, labels=labels[:, 0], hop_samples=hop, z=z, draws=Rd)
    full = Hs.synthesize((model, vae), audio, text, seed_pose, labels=labels[:, :1, :].expand(U, W, 8)[:, None].expand(U, Rd, W, 8), hop_samples=hop,
                         z=z, draws=Rd)
    assert torch.equal(one["track"], full["track"])
    # per-draw labels: draw 1 gets another emotion, its track changes and the other draws' do not
    per = labels[:, None].expand(U, Rd, W, 8).clone()
    per[:, 1] = torch.roll(per[:, 1], 1, dims=-1)
    other = Hs.synthesize((model, vae), audio, text, seed_pose, labels=per, hop_samples=hop, z=z, draws=Rd)
    assert torch.equal(other["track"][:, 0], got["track"][:, 0]) and torch.equal(other["track"][:, 2], got["track"][:, 2])
    assert not torch.equal(other["track"][:, 1], got["track"][:, 1])
    with pytest.raises(L.EgError, match="z shape"):
        Hs.synthesize((model, vae), audio, text, seed_pose, labels=labels, hop_samples=hop, z=z.reshape(U * Rd, W, 32), draws=Rd)
    with pytest.raises(L.EgError, match="labels shape"):
        Hs.synthesize((model, vae), audio, text, seed_pose, labels=labels[:1], hop_samples=hop, z=z, draws=Rd)
