"""Streaming synthesis on the GPU (eg_stream_* / eg_generator_stream_step through streaming.GestureStream, Transformer.open_stream and
harness.open_stream) against (1) the roll-out goldens made from the reference's own Transformer, (2) a Python loop of model.forward + the
blend in torch, (3) harness.synthesize on the whole recording, and (4) itself: graph replay against eager, rows against rows."""
import numpy as np
import pytest
import torch

import rollout_np as R
from conftest import build_mirror, clip_rel_l2
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import streaming as S
from emotiongestures_amd.synth import hash_uniform, load_synth_weights, synth_audio
from rollout_np import CASES, load_case

pytestmark = pytest.mark.gpu

POSE_TOL = {"f32": 2e-5, "bf16x3": 1e-3}        # tests/test_gpu_rollout.py:16
F_, D_, P_ = 34, 126, 4
H_ = F_ - P_
HOP, N = 32000, (124 - 1) * 512                 # 30 poses at 15 fps = 2 s; the shortest clip with 124 spectrogram columns
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


def mel_front():
    from emotiongestures_amd.engine import MelFrontEnd
    return MelFrontEnd(dev())


def inputs(U, W, seed, with_sampled):
    inp = R.rollout_inputs(U, W, F_, D_, P_, seed=seed)
    g = {k: torch.from_numpy(inp[k]).to(dev()) for k in ("spec", "text", "seed_pose", "label", "z")}
    g["sampled"] = torch.from_numpy(hash_uniform("rollout/sampled", (U, W, F_, 512), -1.0, 1.0, seed)).to(dev()) if with_sampled else None
    return g


def torch_loop(model, spec, text, seed_pose, sampled=None, alpha=None):
    """tests/test_gpu_rollout.py's loop: one forward() per window, the hand-off and the blend as torch ops on the device."""
    U, W = spec.shape[:2]
    a = torch.from_numpy(R.default_alpha(P_)).to(spec.device) if alpha is None else alpha
    a = a[None, :, None]
    track = torch.empty(U, W * H_ + P_, D_, device=spec.device)
    prior, wins = seed_pose, []
    with torch.no_grad():
        for w in range(W):
            pose = model(spec[:, w].contiguous(), text[:, w].contiguous(), prior.contiguous(), None if sampled is None else sampled[:, w].contiguous())[0]
            if w == 0:
                track[:, :F_] = pose
            else:
                track[:, w * H_: w * H_ + P_] = (1 - a) * prior + a * pose[:, :P_]
                track[:, w * H_ + P_: w * H_ + F_] = pose[:, P_:]
            wins.append(pose)
            prior = pose[:, H_:]
    return {"track": track, "windows": torch.stack(wins, 1)}


def run_spec_stream(model, g, W, graph, alpha=None):
    """push_spec window after window -> (track [U, W*H + P, D], windows [U, W, F, D])."""
    s = S.GestureStream((model, None, None), g["spec"].shape[0], g["seed_pose"], alpha=alpha, graph=graph, want_windows=True)
    rows, wins = [], []
    for w in range(W):
        r, valid = s.push_spec(g["spec"][:, w], g["text"][:, w], sampled=None if g["sampled"] is None else g["sampled"][:, w])
        assert bool(valid.all()) and s.last_valid == [True] * len(valid)
        rows.append(r)
        wins.append(s.last_window)
    return torch.cat(rows + [s.tail()], 1), torch.stack(wins, 1)


# ---- 4: against the reference goldens ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_matches_reference_golden(name, prec):
    """push_spec over the fixture's W windows: window w within the fixture's own free-running bar POSE_TOL * (1 + window_gain * sum_{i<w}
    handoff_gain^i), gains read from the npz; the track is a convex blend of the windows, held to the last window's bar."""
    z, m, inp, sampled = load_case(name)
    model = model_for(CASES[name], prec, m["seed"])
    hg, wg = float(z["handoff_gain"]), float(z["window_gain"])
    g = {k: torch.from_numpy(inp[k]).to(dev()) for k in ("spec", "text", "seed_pose")}
    g["sampled"] = None if sampled is None else sampled.to(dev())
    track, win = run_spec_stream(model, g, m["W"], graph=True)
    torch.cuda.synchronize()
    win, track = win.cpu().numpy(), track.cpu().numpy()
    assert win.shape == z["windows"].shape and track.shape == z["track"].shape
    for w in range(m["W"]):
        e, tol = clip_rel_l2(win[:, w], z["windows"][:, w]), R.free_running_tol(POSE_TOL[prec], wg, hg, w)
        print(f"{name} {prec} stream window {w}: per-clip rel-L2 {e:.2e} (tolerance {tol:.2e})")
        assert e < tol, (w, e, tol)
    e = clip_rel_l2(track, z["track"])
    print(f"{name} {prec} stream track: per-clip rel-L2 {e:.2e}")
    assert e < R.free_running_tol(POSE_TOL[prec], wg, hg, m["W"] - 1)
    assert np.array_equal(track, R.stitch(win, m["prior"]))         # rows + tail are exactly the stitch of the windows this stream produced


# ---- 5: against the loop of forward() calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sampled", [False, True])
@pytest.mark.parametrize("U", [1, 2, 5])
@pytest.mark.parametrize("variant", ["spatial", "memory"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_stream_equals_loop_of_forwards_bitwise(prec, variant, U, with_sampled):
    """The step takes the product paths forward() takes at batch U (one-clip split-K included), so every U is bit for bit."""
    W = 3
    model = model_for(variant, prec)
    g = inputs(U, W, seed=30 + U * 4 + W, with_sampled=with_sampled)
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"], g["sampled"])
    track, win = run_spec_stream(model, g, W, graph=False)
    torch.cuda.synchronize()
    assert torch.equal(win, want["windows"])
    assert torch.equal(track, want["track"])


def test_stream_alpha_equals_the_loop():
    model = model_for("spatial", "bf16x3")
    g = inputs(3, 3, seed=52, with_sampled=False)
    alpha = torch.tensor([0.9, 0.5, 0.25, 0.0], device=dev())
    want = torch_loop(model, g["spec"], g["text"], g["seed_pose"], None, alpha)
    track, _win = run_spec_stream(model, g, 3, graph=False, alpha=alpha)
    assert torch.equal(track, want["track"])


# ---- 6: against harness.synthesize from raw audio ----------------------------------------------------------------------------------------
def feed_audio(s, audio, T, g, col=lambda step: max(0, step - 2), steps=None):
    """Feed recordings [U, >= T] hop by hop; the push that holds sample T - 1 ends every row.  Step k (1-based) gets the text / label / z of
    column col(k).  Returns ([rows per step], [valid per step])."""
    U = audio.shape[0]
    last = max(1, -(-T // s.hop))
    steps = last if steps is None else steps
    padded = torch.zeros(U, max(steps, last) * s.hop, device=audio.device)
    padded[:, :T] = audio[:, :T]
    out, valids = [], []
    for k in range(1, steps + 1):
        c = col(k)
        r, v = s.push(padded[:, (k - 1) * s.hop: k * s.hop].contiguous(), g["text"][:, c], g["label"][:, c], g["z"][:, c],
                      ends=T - (last - 1) * s.hop if k == last else None)
        out.append(r)
        valids.append(v.cpu().tolist())
    return out, valids


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("U", [2, 1])
def test_stream_equals_harness_synthesize_from_raw_audio(U, prec):
    """T = 2*hop + n - 9000: three full pushes (windows 0 and 1 come out of pushes 2 and 3), a fourth with ends = 21 976 (window 2, 9 000 samples
    short, padded); one more step gives window 3.  U = 2: torch.equal.  U = 1: f32 bitwise, bf16x3 within POSE_TOL (the roll-out's
    phase A does not take the one-clip split-K; measured 2.0e-5 there)."""
    model, vae = model_for("spatial", prec), vae_for()
    T = 2 * HOP + N - 9000
    assert T == 117976 and T - 3 * HOP == 21976
    audio = torch.from_numpy(synth_audio(U, T, seed=80)).to(dev())
    g = inputs(U, 4, seed=80, with_sampled=False)
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP)
    assert (s.hop, s.n, s.lag) == (HOP, N, 2)
    rows, valids = feed_audio(s, audio, T, g, steps=4)
    assert rows[0] is None and valids == [[0] * U] + [[1] * U] * 3

    def check(W, got):
        want = Hs.synthesize((model, vae), audio, g["text"][:, :W].contiguous(), g["seed_pose"], labels=g["label"][:, :W].contiguous(), hop_samples=HOP,
                             z=g["z"][:, :W].contiguous(), windows=W)["track"]
        e = clip_rel_l2(got.cpu().numpy(), want.cpu().numpy())
        print(f"U={U} {prec} W={W}: stream vs synthesize bitwise={torch.equal(got, want)} per-clip rel-L2 {e:.2e}")
        assert got.shape == want.shape
        if U >= 2 or prec == "f32":
            assert torch.equal(got, want)
        else:
            assert e < POSE_TOL[prec]
    check(3, torch.cat(rows[1:] + [s.tail()], 1))
    r5, v5 = s.push(torch.zeros(U, HOP, device=dev()), g["text"][:, 3], g["label"][:, 3], g["z"][:, 3])
    assert v5.cpu().tolist() == [1] * U
    check(4, torch.cat(rows[1:] + [r5, s.tail()], 1))
    r6, v6 = s.push(torch.zeros(U, HOP, device=dev()), g["text"][:, 3], g["label"][:, 3], g["z"][:, 3])
    assert r6 is None and v6.cpu().tolist() == [0] * U             # ceil(T / hop) = 4 windows exist


def test_row_that_ends_in_its_first_push_and_finish():
    model, vae = model_for("spatial", "bf16x3"), vae_for()
    U, T = 2, HOP // 2 + 1
    audio = torch.from_numpy(synth_audio(U, T, seed=81)).to(dev())
    g = inputs(U, 4, seed=81, with_sampled=False)
    syn = lambda a, W: Hs.synthesize((model, vae), a, g["text"][:, :W].contiguous(), g["seed_pose"], labels=g["label"][:, :W].contiguous(),
                                     hop_samples=HOP, z=g["z"][:, :W].contiguous(), windows=W)["track"]
    s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP)
    rows, valids = feed_audio(s, audio, T, g, col=lambda k: 0)
    assert valids == [[1, 1]]                               # window 0 at ring offset hop
    assert torch.equal(torch.cat(rows + [s.tail()], 1), syn(audio, 1))
    # finish(): the recording of the raw-audio test stops inside its fourth hop; two pushes, then finish with the last chunk
    T = 2 * HOP + N - 9000
    audio = torch.from_numpy(synth_audio(U, T, seed=80)).to(dev())
    s.reset()
    rows, _v = feed_audio(s, audio, 3 * HOP + 1, g, steps=3)           # three full pushes, nothing ends
    last = torch.zeros(U, HOP, device=dev())
    last[:, :T - 3 * HOP] = audio[:, 3 * HOP:]
    with pytest.raises(L.EgError, match="windows remain"):
        s.finish(g["text"][:, :3], g["label"][:, :3], g["z"][:, :3], last_chunk=last, ends=T - 3 * HOP)
    end = s.finish(g["text"][:, 2:4], g["label"][:, 2:4], g["z"][:, 2:4], last_chunk=last, ends=T - 3 * HOP)
    assert tuple(end.shape) == (U, 2 * H_ + P_, D_)
    assert torch.equal(torch.cat(rows[1:] + [end], 1), syn(audio, 4))
    with pytest.raises(L.EgError, match="push after finish"):
        s.push(last, g["text"][:, 0], g["label"][:, 0], g["z"][:, 0])


@pytest.mark.parametrize("hop,n", [(1000, 2500), (1000, 1000), (700, 3000), (64000, 62976)])
def test_push_clips_equal_the_numpy_restatement(hop, n):
    """eg_stream_push + the step's counters on the CPU test's (hop, n) grid (lag 3, 1, 5, 1), three rows of different lengths stepped well past
    their ends: every clip is bitwise the restated ring's (which test_stream_host holds to np.pad), a row without a ready window is all zero."""
    import stream_np as SN
    eng = model_for("spatial", "bf16x3").engine()
    U, lag = 3, -(-n // hop)
    T = [hop // 2 + 1, 2 * hop + max(1, n - 9), 5 * hop + 7]
    steps = 6 + lag + 2
    rng = np.random.RandomState(hop + n)
    audio = rng.standard_normal((U, steps * hop)).astype(np.float32)      # what lies past a row's end is garbage that must never reach a clip
    state = torch.zeros(eng.stream_state_bytes(U, hop, n), dtype=torch.uint8, device=dev())
    eng.stream_reset(state, U, hop, n, torch.zeros(U, P_, D_, device=dev()))
    ref = [SN.RingRow(hop, n) for _ in range(U)]
    spec = torch.zeros(U, 128, 124, device=dev())
    seen = 0
    for k in range(1, steps + 1):
        ends = [T[u] - (k - 1) * hop if (k - 1) * hop < T[u] <= k * hop else -1 for u in range(U)]
        chunk = audio[:, (k - 1) * hop: k * hop]
        clips = eng.stream_push(state, U, hop, n, torch.from_numpy(np.ascontiguousarray(chunk)).to(dev()),
                                torch.tensor(ends, dtype=torch.int32, device=dev())).cpu().numpy()
        valid = eng.stream_step(state, U, hop, n, spec)["valid"].cpu().tolist()
        for u in range(U):
            want = ref[u].push(chunk[u], ends[u])
            assert valid[u] == int(want is not None), (k, u)
            assert np.array_equal(clips[u], np.zeros(n, np.float32) if want is None else want), (k, u)
            seen += want is not None
    assert seen == sum(-(-t // hop) for t in T)


# ---- 7: one graph for every step ---------------------------------------------------------------------------------------------------------
def test_one_graph_serves_every_step():
    """Captured once (by the first valid step); six replays held to zero host-side library launches: steady state, two steps in which one row is not
    valid, the ending push, a step after it, and -- after a reset -- window 0.  The outputs are bitwise those of a graph=False session fed the
    same inputs."""
    lib = L.load()
    model, vae, mel = model_for("spatial", "bf16x3"), vae_for(), mel_front()
    U, steps = 3, 8
    T = [5 * HOP + 5000, HOP + 100, 5 * HOP + 5000]         # rows 0, 2: six windows (pushes 2..7); row 1: two (pushes 2, 3)
    audio = torch.zeros(U, steps * HOP, device=dev())
    for u in range(U):
        audio[u, :T[u]] = torch.from_numpy(synth_audio(1, T[u], seed=90 + u)[0]).to(dev())
    g = inputs(U, steps, seed=90, with_sampled=False)
    sess = {gr: S.GestureStream((model, vae, mel), U, g["seed_pose"], hop_samples=HOP, graph=gr) for gr in (True, False)}
    outs = {True: [], False: []}
    graph_obj, replays = None, 0
    for k in range(1, steps + 1):
        ends = [T[u] - (k - 1) * HOP if (k - 1) * HOP < T[u] <= k * HOP else -1 for u in range(U)]
        for gr, s in sess.items():
            n0 = lib.eg_launch_count()
            r, v = s.push(audio[:, (k - 1) * HOP: k * HOP].contiguous(), g["text"][:, k - 1], g["label"][:, k - 1], g["z"][:, k - 1], ends=ends)
            torch.cuda.synchronize()
            launched = lib.eg_launch_count() - n0
            outs[gr].append((r, v.cpu().tolist()))
            if gr and r is not None:
                if graph_obj is None:
                    graph_obj = s._graphs[False]["graph"]   # the first valid step captures (two warm-up runs + the capture)
                    assert launched > 0
                else:
                    replays += 1
                    assert launched == 0, (k, launched)     # a replay: no host-side library launch
                    assert s._graphs[False]["graph"] is graph_obj and len(s._graphs) == 1
            if not gr and r is not None:
                print(f"step {k}: eager stream step {launched} library launches")
    want_valid = [[int(i["valid"]) for i in S.plan(HOP, N, T[u], steps)] for u in range(U)]
    for k in range(steps):
        (rg, vg), (re_, ve) = outs[True][k], outs[False][k]
        assert vg == ve == [want_valid[u][k] for u in range(U)], k
        assert (rg is None) == (re_ is None) == (not any(vg))
        if rg is not None:
            assert torch.equal(rg, re_), k
            for u in range(U):
                if not vg[u]:
                    assert not rg[u].any()
    assert [v for _r, v in outs[True]] == [[0, 0, 0], [1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 0, 1], [1, 0, 1], [1, 0, 1], [0, 0, 0]]
    assert replays == 5 and torch.equal(sess[True].tail(), sess[False].tail())
    # window 0 out of a pure replay: the graph survives a reset, so a second recording's first window is served by the graph captured above
    after = {}
    for gr, s in sess.items():
        s.reset()
        for k in (1, 2):
            n0 = lib.eg_launch_count()
            r, v = s.push(audio[:, (k - 1) * HOP: k * HOP].contiguous(), g["text"][:, k - 1], g["label"][:, k - 1], g["z"][:, k - 1])
            torch.cuda.synchronize()
            launched = lib.eg_launch_count() - n0
        assert v.cpu().tolist() == [1, 1, 1] and s.last_windows == [0, 0, 0]
        if gr:
            replays += 1
            assert launched == 0 and s._graphs[False]["graph"] is graph_obj and len(s._graphs) == 1
        after[gr] = r
    assert torch.equal(after[True], after[False])
    assert torch.equal(after[True][[0, 2]], outs[True][1][0][[0, 2]])       # rows 0 and 2: the same recording's window 0 as in step 2 (row 1 ended there)
    assert replays >= 6


# ---- 8: rows are independent sessions (spatial) -------------------------------------------------------------------------------------------
def test_rows_are_independent_sessions():
    """U = 3: row 1 ends, is reset mid-stream with another seed pose and fed a second recording while rows 0 and 2 go on."""
    model, vae, mel = model_for("spatial", "bf16x3"), vae_for(), mel_front()
    U, steps = 3, 6
    TA, T1, T2 = 4 * HOP + 1234, HOP + 500, 2 * HOP - 700
    rec = lambda T, seed: torch.from_numpy(synth_audio(1, T, seed=seed)[0]).to(dev())
    a0, a2, b1, b2 = rec(TA, 100), rec(TA, 102), rec(T1, 101), rec(T2, 103)
    g = inputs(U, steps, seed=100, with_sampled=False)
    seed2 = torch.from_numpy(hash_uniform("stream/seed2", (U, P_, D_), -0.5, 0.5, 3)).to(dev())
    chunk = lambda a, T, k: torch.nn.functional.pad(a, (0, steps * HOP))[(k - 1) * HOP: k * HOP]
    end_of = lambda T, k: T - (k - 1) * HOP if (k - 1) * HOP < T <= k * HOP else -1

    def run(scenario_b):
        s = Hs.open_stream((model, vae), U, g["seed_pose"], mel=mel, hop_samples=HOP)
        out, zero_clip = [], None
        for k in range(1, steps + 1):
            if scenario_b and k == 4:
                s.reset(rows=[1], seed_pose=seed2)
            if scenario_b:
                mid, e1 = (chunk(b1, T1, k), end_of(T1, k)) if k <= 3 else (chunk(b2, T2, k - 3), end_of(T2, k - 3))
            else:
                mid, e1 = chunk(a0, TA, k) * 0.5, end_of(TA, k)
            audio = torch.stack([chunk(a0, TA, k), mid, chunk(a2, TA, k)])
            r, v = s.push(audio, g["text"][:, k - 1], g["label"][:, k - 1], g["z"][:, k - 1], ends=[end_of(TA, k), e1, end_of(TA, k)])
            out.append((r, v.cpu().tolist()))
            if scenario_b and k == 4:
                zero_clip = s._clips[1].clone()
        return out, s.tail(), zero_clip

    base, tail_a, _ = run(False)
    got, tail_b, zero_clip = run(True)
    # valid exactly where plan says; rows of a row that is not valid are zero
    p1 = [i["valid"] for i in S.plan(HOP, N, T1, 3)] + [i["valid"] for i in S.plan(HOP, N, T2, 3)]
    pa = [i["valid"] for i in S.plan(HOP, N, TA, steps)]
    assert p1 == [False, True, True, False, True, True] and pa == [False, True, True, True, True, True]
    for k in range(steps):
        r, v = got[k]
        assert v == [int(pa[k]), int(p1[k]), int(pa[k])], k
        if r is not None and not v[1]:
            assert not r[1].any()
    # rows 0 and 2 are bitwise what they are without any of that
    for k in range(1, steps):
        assert torch.equal(got[k][0][[0, 2]], base[k][0][[0, 2]]), k
    assert torch.equal(tail_b[[0, 2]], tail_a[[0, 2]])
    # the waiting row is an all-zero clip for lag - 1 = 1 step, and its spectrogram is finite: 0 dB throughout
    assert not zero_clip.any()
    zs = mel(torch.zeros(1, N, device=dev()), out_frames=124)
    assert bool(torch.isfinite(zs).all()) and float(zs.abs().max()) < 1e-6

    def syn(audio2, W, cols, seed_pose, row):
        """synthesize on a batch of two recordings of one length; text / label / z of the stream's row `row` at steps `cols`."""
        pick = lambda t: torch.stack([t[row, cols], t[(row + 1) % U, cols]])
        return Hs.synthesize((model, vae), audio2, pick(g["text"]), torch.stack([seed_pose[row], seed_pose[(row + 1) % U]]), labels=pick(g["label"]),
                             hop_samples=HOP, z=pick(g["z"]), windows=W, mel=mel)["track"][0]
    # row 1's second recording: windows out of pushes 5 and 6 (columns 4, 5), seeded with seed2
    second = torch.cat([got[4][0][1], got[5][0][1], tail_b[1]], 0)
    assert torch.equal(second, syn(torch.stack([b2, rec(T2, 104)]), 2, [4, 5], seed2, 1))
    # rows ending at different lengths: row 1's first recording (pushes 2, 3) and row 0 (pushes 2..6), each against its own length
    first = torch.cat([got[1][0][1], got[2][0][1]], 0)
    assert torch.equal(first, syn(torch.stack([b1, rec(T1, 105)]), 2, [1, 2], g["seed_pose"], 1)[: 2 * H_])
    row0 = torch.cat([got[k][0][0] for k in range(1, 6)] + [tail_b[0]], 0)
    assert torch.equal(row0, syn(torch.stack([a0, rec(TA, 106)]), 5, [1, 2, 3, 4, 5], g["seed_pose"], 0))


# ---- 9: sessions, refresh, stale graphs ---------------------------------------------------------------------------------------------------
def test_two_sessions_on_one_generator_do_not_share_state():
    model = model_for("memory", "bf16x3")
    ga, gb = inputs(2, 3, seed=110, with_sampled=True), inputs(2, 3, seed=111, with_sampled=False)
    want_a, _ = run_spec_stream(model, ga, 3, graph=False)
    want_b, _ = run_spec_stream(model, gb, 3, graph=False)
    sa, sb = S.GestureStream((model, None, None), 2, ga["seed_pose"]), S.GestureStream((model, None, None), 2, gb["seed_pose"])
    ra, rb = [], []
    for w in range(3):                                      # interleaved
        ra.append(sa.push_spec(ga["spec"][:, w], ga["text"][:, w], sampled=ga["sampled"][:, w])[0])
        rb.append(sb.push_spec(gb["spec"][:, w], gb["text"][:, w])[0])
    assert torch.equal(torch.cat(ra + [sa.tail()], 1), want_a)
    assert torch.equal(torch.cat(rb + [sb.tail()], 1), want_b)
    with pytest.raises(L.EgError, match="TM_Memory_Net couples the rows"):
        sa.reset(rows=[0])
    with pytest.raises(L.EgError, match="TM_Memory_Net couples the rows"):
        sa.push_spec(ga["spec"][:, 0], ga["text"][:, 0], sampled=ga["sampled"][:, 0], ends=[1, -1])


def test_refresh_keeps_the_state_and_a_stale_graph_raises():
    model = build_mirror("spatial", F_, D_, P_, 4, seed=7, precision="bf16x3").to(dev())
    other = build_mirror("spatial", F_, D_, P_, 4, seed=8, precision="bf16x3")
    g = inputs(2, 4, seed=120, with_sampled=False)
    step = lambda s, w: s.push_spec(g["spec"][:, w], g["text"][:, w])[0]
    sg, se = (S.GestureStream((model, None, None), 2, g["seed_pose"], graph=gr) for gr in (True, False))
    rows_g, rows_e = [step(sg, 0), step(sg, 1)], [step(se, 0), step(se, 1)]
    model.load_state_dict(other.state_dict())
    assert sg.stale()
    with pytest.raises(RuntimeError, match="refresh"):
        step(sg, 2)
    assert sg.plan.rows == [(2, 2, -1)] * 2                 # the refused push committed nothing
    sg.refresh()
    assert not sg.stale()
    for w in (2, 3):
        rows_g.append(step(sg, w))
        rows_e.append(step(se, w))                          # the eager session takes the new weights by itself
    assert torch.equal(torch.cat(rows_g + [sg.tail()], 1), torch.cat(rows_e + [se.tail()], 1))
    # windows 2 and 3 were made with the new weights from the prior the old weights left: not what either model gives alone
    assert not torch.equal(rows_g[2], run_spec_stream(model, g, 3, graph=False)[0][:, 2 * H_: 3 * H_])


def test_open_stream_entry_points_share_one_default():
    """Transformer.open_stream and harness.open_stream both make a mel front-end of the session's own unless one is passed."""
    model, vae = model_for("spatial", "bf16x3"), vae_for()
    g = inputs(2, 1, seed=131, with_sampled=False)
    mel = mel_front()
    a, b, c = model.open_stream(2, g["seed_pose"], vae=vae), Hs.open_stream((model, vae), 2, g["seed_pose"]), model.open_stream(2, g["seed_pose"], mel=mel)
    assert a.mel is not None and b.mel is not None and a.mel is not b.mel and c.mel is mel
    assert (a.hop, a.n) == (b.hop, b.n) == (HOP, N)
    veng = vae.engine()
    audio = torch.from_numpy(synth_audio(2, 2 * HOP, seed=131)).to(dev())
    for k in range(2):
        ra, _ = a.push(audio[:, k * HOP: (k + 1) * HOP].contiguous(), g["text"][:, 0], g["label"][:, 0], g["z"][:, 0])
        rb, _ = b.push(audio[:, k * HOP: (k + 1) * HOP].contiguous(), g["text"][:, 0], g["label"][:, 0], g["z"][:, 0])
    assert torch.equal(ra, rb)
    # close() gives back the session's private mel / CVAE workspaces and leaves the other session's alone
    assert any(k[-1] == a._slot for k in veng._ws) and any(k[-1] == a._slot for k in a.mel._ws)
    a.close()
    assert not any(k[-1] == a._slot for k in veng._ws) and not any(k[-1] == a._slot for k in a.mel._ws)
    assert any(k[-1] == b._slot for k in veng._ws)
    with pytest.raises(L.EgError, match="no mel front-end"):
        S.GestureStream((model, None, None), 2, g["seed_pose"], hop_samples=HOP)


def test_a_failed_launch_commits_nothing(monkeypatch):
    model = model_for("spatial", "bf16x3")
    g = inputs(2, 2, seed=132, with_sampled=False)
    s = S.GestureStream((model, None, None), 2, g["seed_pose"], graph=False)
    want = S.GestureStream((model, None, None), 2, g["seed_pose"], graph=False)

    def boom(*a, **k):
        raise RuntimeError("launch failed")
    monkeypatch.setattr(s, "_launch", boom)
    with pytest.raises(RuntimeError, match="launch failed"):
        s.push_spec(g["spec"][:, 0], g["text"][:, 0])
    assert s.plan.rows == [(0, 0, -1)] * 2 and s.last_valid == [False, False]
    monkeypatch.undo()
    for w in range(2):
        assert torch.equal(s.push_spec(g["spec"][:, w], g["text"][:, w])[0], want.push_spec(g["spec"][:, w], g["text"][:, w])[0])


def test_gpu_tensors_only():
    model = model_for("spatial", "bf16x3")
    g = inputs(2, 1, seed=130, with_sampled=False)
    s = S.GestureStream((model, None, None), 2, g["seed_pose"])
    with pytest.raises(L.EgError, match="GPU tensor"):
        s.push_spec(g["spec"][:, 0].cpu(), g["text"][:, 0])
    with pytest.raises(L.EgError, match="spec shape"):
        s.push_spec(g["spec"][:, 0, :, :100], g["text"][:, 0])
    with pytest.raises(L.EgError, match="no mel front-end"):
        s.push(torch.zeros(2, 1, device=dev()), g["text"][:, 0])
    assert s.plan.rows == [(0, 0, -1)] * 2
