"""Beat alignment of whole recordings on the GPU (eg_beat_align_tracks through beat.beat_alignment_tracks and harness.synthesize(beat=True)):
(1) bit for bit the clip call wherever the clip call exists, (2) beyond its limits against the numpy restatement of the audio half
(tests/beat_np.py), the host load_pose and the host calculate_align, (3) draws against the recordings repeated, (4) edge cases, (5) the
per-frame form of the wait-suppressed scan on constructed runs, (6) end to end from raw audio."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import beat_np
import rollout_np as R
from conftest import build_mirror
from emotiongestures_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 1e-4
SR = 16000


# ---- the seeded generators of tests/test_gpu_beat.py, copied -----------------------------------------------------------------------
def noise_bursts(b, n, seed):
    """Seeded BEAT-like audio: noise whose level jumps every 512..4096 samples (onsets at the jumps), some stretches silent."""
    rng = np.random.default_rng(seed)
    out = np.zeros((b, n), np.float32)
    for i in range(b):
        env = np.zeros(n, np.float32)
        p = 0
        while p < n:
            L_ = int(rng.integers(512, 4096))
            env[p:p + L_] = 0.0 if rng.random() < 0.25 else rng.uniform(0.01, 1.0)
            p += L_
        out[i] = rng.standard_normal(n).astype(np.float32) * env
    return out


def random_poses(b, f, d, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((b, f, d)).astype(np.float32) * np.float32(0.05), axis=1, dtype=np.float32)


def _sets(c):
    return np.repeat(np.arange(c.shape[-1]), c.astype(np.int64))


def ragged_audio(lengths, seed, stale=None):
    """[U, max length]: row u holds noise_bursts of its own length; the rest is `stale` ("noise": 1e3-scale noise, "nan")."""
    U, stride = len(lengths), max(lengths)
    a = np.zeros((U, stride), np.float32)
    if stale == "noise":
        a[:] = np.random.default_rng(seed + 999).standard_normal((U, stride)).astype(np.float32) * np.float32(1e3)
    elif stale == "nan":
        a[:] = np.nan
    for u, n in enumerate(lengths):
        a[u, :n] = noise_bursts(1, n, seed + u)[0]
    return a


def ragged_track(frames, R_, D, seed, stale_nan=False):
    U, Tmax = len(frames), max(frames)
    t = random_poses(U * R_, Tmax, D, seed).reshape(U, R_, Tmax, D)
    if stale_nan:
        for u, f in enumerate(frames):
            t[u, :, f:] = np.nan
    return t


def tracks(audio, track, lengths=None, frames=None, **kw):
    from emotiongestures_amd.beat import beat_alignment_tracks
    sc, bt = beat_alignment_tracks(torch.from_numpy(audio).to(DEV), torch.from_numpy(track).to(DEV), lengths=lengths, frames=frames,
                                   want_beats=True, **kw)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), {k: v.cpu().numpy() for k, v in bt.items()}


def clip(audio_row, pose, **kw):
    from emotiongestures_amd.beat import beat_alignment
    sc, bt = beat_alignment(torch.from_numpy(audio_row[None]).to(DEV), torch.from_numpy(pose[None]).to(DEV), want_beats=True, **kw)
    torch.cuda.synchronize()
    return sc.cpu().numpy()[0], {k: v.cpu().numpy()[0] for k, v in bt.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1: equals the clip call where the clip call exists --------------------------------------------------------------------------------
CLIP_LENGTHS = [524287, 300000, 64000, 48123, 2048]
# poses to match at 15 fps, one recording at the clip call's cap of 1025; the 2048-sample recording carries 15 poses (t_end = 1: with fewer,
# int(frames / fps) = 0 and both calls refuse t_end <= t_start)
CLIP_FRAMES = [1025, 281, 60, 45, 15]


@pytest.mark.parametrize("R_", [1, 3])
def test_equals_the_clip_call_bit_for_bit_and_ignores_stale_rows(R_):
    results = []
    for stale in ("noise", "nan"):
        audio = ragged_audio(CLIP_LENGTHS, 60, stale)
        track = ragged_track(CLIP_FRAMES, R_, 282, 61, stale_nan=(stale == "nan"))
        sc, bt = tracks(audio, track, CLIP_LENGTHS, CLIP_FRAMES)
        assert sc.shape == (5, R_) and bt["oenv"].shape == (5, 1024) and bt["pose_beats"].shape == (5, R_, 8, 1024)
        results.append((sc, bt))
        if stale == "nan":
            continue
        for u, (n, f) in enumerate(zip(CLIP_LENGTHS, CLIP_FRAMES)):
            T = 1 + n // 512
            assert bt["n_frames"][u] == T and bt["pose_frames"][u] == f
            for r in range(R_):
                csc, cbt = clip(audio[u, :n], track[u, r, :f])
                assert same_bits(sc[u, r], csc), (u, r, sc[u, r], csc)
                assert same_bits(bt["pose_beats"][u, r, :, :f - 1], cbt["pose_beats"]), (u, r)
                assert not bt["pose_beats"][u, r, :, f - 1:].any()
                if r == 0:
                    for k in ("oenv", "rms"):
                        assert same_bits(bt[k][u, :T], cbt[k]), (u, k)
                        assert not bt[k][u, T:].any()
                    assert same_bits(bt["audio_beats"][u, :, :T], cbt["audio_beats"]), u
                    assert bt["n_audio_beats"][u] == cbt["n_audio_beats"]
        assert (bt["n_audio_beats"][:4] > 0).all()
    (s0, b0), (s1, b1) = results
    assert same_bits(s0, s1)
    for k in b0:
        assert same_bits(b0[k], b1[k]), k


# ---- 2: beyond the clip call's limits ----------------------------------------------------------------------------------------------
def check_audio(y, got, tag):
    """tests/test_gpu_beat.py's _check_audio for one recording: oenv / rms within rel-L2 1e-5 of the restatement; beat decisions equal except
    where the restatement's own decision margin is below MARGIN.  Returns the recorded flips."""
    flips = []
    r = beat_np.load_audio(y)
    T = r["oenv"].size
    for k in ("oenv", "rms"):
        ref, g = r[k].astype(np.float64), got[k][:T].astype(np.float64)
        err = np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30)
        print(f"{tag}: {k} rel-L2 {err:.3e} (T = {T}, {r['raw'].size} events in the restatement)")
        assert err <= 1e-5, (tag, k, err)
    ab = got["audio_beats"][:, :T]
    got_raw = np.flatnonzero(ab[0])
    assert got["n_audio_beats"] == got_raw.size
    fragile = np.flatnonzero(r["peak_margin"] < MARGIN)
    for n in np.flatnonzero(beat_np.counts(got_raw, T) != beat_np.counts(r["raw"], T)):
        near = fragile[np.abs(fragile - n) <= 2]
        assert near.size, f"{tag}: onset flip at frame {n} without a decision margin < {MARGIN} near it"
        flips.append((tag, "raw", int(n), float(r["peak_margin"][near].min())))
    for a, (flag, mm) in enumerate(zip(r["min_flag"], r["min_margin"]), start=1):
        ref_bt = beat_np.backtrack(got_raw, flag)
        got_bt = _sets(ab[a])
        assert got_bt.size == got_raw.size, (tag, a)
        for e, g, f in zip(got_raw, got_bt, ref_bt):
            if g != f:
                lo = min(g, f)
                assert (mm[lo:e + 1] < MARGIN).any(), f"{tag}: backtrack {a} of onset {e}: {g} vs {f}"
                flips.append((tag, f"bt{a}", int(e), float(mm[lo:e + 1].min())))
    for fl in flips:
        print("beat decision flip (restatement margin < 1e-4):", fl)
    return flips


LONG_LENGTHS = [1200000, 700123, 524288, 9600000]           # 75 s, 43.8 s, the first length the clip call refuses, 10 min
LONG_FRAMES = [n * 15 // SR for n in LONG_LENGTHS]          # 1125, 656, 491, 9000


def test_beyond_the_clip_limits_against_restatement_and_host_alignment():
    from emotiongestures_amd.beat import alignment, beat_alignment
    assert LONG_FRAMES == [1125, 656, 491, 9000]
    R_ = 2
    audio = np.zeros((4, max(LONG_LENGTHS)), np.float32)
    for u, n in enumerate(LONG_LENGTHS):
        audio[u, :n] = noise_bursts(1, n, 101)[0]
    track = ragged_track(LONG_FRAMES, R_, 282, 102)
    with pytest.raises(ValueError, match="outside 2048"):                                  # the clip call still refuses these
        beat_alignment(torch.from_numpy(audio[2:3, :524288]).to(DEV), torch.from_numpy(track[2, 0, :491][None]).to(DEV))
    sc, bt = tracks(audio, track, LONG_LENGTHS, LONG_FRAMES)
    flips, total_T = [], 0
    al = alignment(0.3, 2)
    for u, (n, f) in enumerate(zip(LONG_LENGTHS, LONG_FRAMES)):
        T = 1 + n // 512
        total_T += T
        assert bt["n_frames"][u] == T
        got = {k: bt[k][u] for k in ("oenv", "rms", "audio_beats", "n_audio_beats")}
        flips += check_audio(audio[u, :n], got, f"rec{u}")
        ons = [_sets(bt["audio_beats"][u, a, :T]) for a in range(3)]
        for r in range(R_):
            sets = al.load_pose(track[u, r, :f], 0, int(f / 15), 15, True)
            for q, s in enumerate(sets):
                assert np.array_equal(s[0], np.flatnonzero(bt["pose_beats"][u, r, q])), (u, r, q)
            ref = al.calculate_align(*ons, *sets, 15)
            print(f"rec{u} draw{r}: score {sc[u, r]!r} host {ref!r} |d| {abs(sc[u, r] - ref):.2e}")
            assert abs(sc[u, r] - ref) <= 1e-12, (u, r, sc[u, r], ref)
    cap = math.ceil(total_T / 1000)
    print(f"beat decision flips admitted: {len(flips)} of at most {cap} ({total_T} onset frames)")
    assert len(flips) <= cap


# ---- 3: draws ------------------------------------------------------------------------------------------------------------------------
def test_draws_equal_the_recordings_repeated_and_share_one_audio_half():
    lengths, frames, R_ = [700123, 160000, 64000], [656, 150, 60], 4
    audio = ragged_audio(lengths, 70)
    track = ragged_track(frames, R_, 282, 71)
    sc, bt = tracks(audio, track, lengths, frames)
    rep = lambda v: [x for x in v for _ in range(R_)]
    sc_rep, bt_rep = tracks(np.repeat(audio, R_, axis=0), track.reshape(3 * R_, max(frames), 282), rep(lengths), rep(frames))
    assert sc.shape == (3, R_) and sc_rep.shape == (3 * R_,) and same_bits(sc.reshape(-1), sc_rep)
    assert same_bits(bt["pose_beats"].reshape(bt_rep["pose_beats"].shape), bt_rep["pose_beats"])
    for k in ("oenv", "rms", "audio_beats", "n_audio_beats", "n_frames"):                  # once per recording
        assert bt[k].shape[0] == 3 and same_bits(bt[k], bt_rep[k][::R_]), k
    assert np.isfinite(sc).all() and len({float(v) for v in sc[0]}) == R_                 # the draws differ


# ---- 4: edge cases ---------------------------------------------------------------------------------------------------------------------
def test_silent_recording_is_nan_and_leaves_neighbours_alone():
    lengths, frames = [700123, 300000, 600000], [656, 281, 562]
    audio = ragged_audio(lengths, 80)
    audio[1] = 0.0
    track = ragged_track(frames, 2, 282, 81)
    sc, bt = tracks(audio, track, lengths, frames)
    assert np.isnan(sc[1]).all() and bt["n_audio_beats"][1] == 0 and not bt["audio_beats"][1].any()
    for u in (0, 2):
        solo, sbt = tracks(audio[u:u + 1, :lengths[u]], track[u:u + 1, :, :frames[u]])       # U = 1, the full rectangle by default
        assert same_bits(solo[0], sc[u]) and np.isfinite(sc[u]).all()
        assert same_bits(sbt["oenv"][0], bt["oenv"][u, :sbt["oenv"].shape[1]])


def test_equal_lengths_t_start_and_repeatability():
    from emotiongestures_amd.beat import alignment
    audio = noise_bursts(3, 160000, 90)
    pose = random_poses(3, 150, 282, 91)
    sc, bt = tracks(audio, pose)                                                         # [U, T, D]: scores follow the track's rank
    assert sc.shape == (3,) and bt["pose_beats"].shape == (3, 8, 149)
    for u in range(3):
        csc, cbt = clip(audio[u], pose[u])
        assert same_bits(sc[u], csc) and same_bits(bt["audio_beats"][u], cbt["audio_beats"]) and same_bits(bt["pose_beats"][u], cbt["pose_beats"])
    sc2, bt2 = tracks(audio, pose)
    assert same_bits(sc, sc2) and all(same_bits(bt[k], bt2[k]) for k in bt)
    # t_start > 0: the audio is sliced at t_start * 16000 and the right-side curves at t_start * fps, as the clip call does
    st, btt = tracks(audio, pose, t_start=2, t_end=9)
    al = alignment(0.3, 2)
    for u in range(3):
        csc, cbt = clip(audio[u], pose[u], t_start=2, t_end=9)
        assert same_bits(st[u], csc) and same_bits(btt["pose_beats"][u], cbt["pose_beats"]) and same_bits(btt["oenv"][u], cbt["oenv"])
        sets = al.load_pose(pose[u], 2, 9, 15, True)
        ref = al.calculate_align(*[_sets(btt["audio_beats"][u, a]) for a in range(3)], *sets, 15)
        assert abs(st[u] - ref) <= 1e-12
    assert not same_bits(st, sc)
    # beyond the clip limit with t_start and per-recording t_end
    lengths, frames = [1200000, 700123], [1125, 656]
    a2, t2 = ragged_audio(lengths, 92), ragged_track(frames, 1, 282, 93)
    s3, b3 = tracks(a2, t2, lengths, frames, t_start=3, t_end=[70, 40])
    for u in range(2):
        sets = al.load_pose(t2[u, 0, :frames[u]], 3, [70, 40][u], 15, True)
        T = b3["n_frames"][u]
        assert T == 1 + (lengths[u] - 3 * SR) // 512
        for q, s in enumerate(sets):
            assert np.array_equal(s[0], np.flatnonzero(b3["pose_beats"][u, 0, q])), (u, q)
        ref = al.calculate_align(*[_sets(b3["audio_beats"][u, a, :T]) for a in range(3)], *sets, 15)
        assert abs(s3[u, 0] - ref) <= 1e-12


def test_captured_graph_replays_the_eager_bits():
    from emotiongestures_amd.beat import _run_tracks
    lengths, frames, R_ = [700123, 160000, 64000], [656, 150, 60], 2
    audio = torch.from_numpy(ragged_audio(lengths, 95)).to(DEV)
    track = torch.from_numpy(ragged_track(frames, R_, 282, 96)).to(DEV)
    args = (audio, track, lengths, frames, 15, 0, None, 0.3, 2, True)
    eager, _plan, _ws = _run_tracks(*args)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in eager.items()}
    out, _plan, ws = _run_tracks(*args)                     # buffers of their own for the graph; a warm-up on them too
    torch.cuda.synchronize()
    for v in out.values():
        v.zero_()
    ws.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run_tracks(*args, workspace=ws, out=out)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in want:
        assert same_bits(out[k].cpu().numpy(), want[k].cpu().numpy()), k
    audio.copy_(torch.from_numpy(ragged_audio(lengths, 97)).to(DEV))        # same pointers, new samples: the replay follows the data
    g.replay()
    fresh, _p, _w = _run_tracks(*args)
    torch.cuda.synchronize()
    for k in want:
        assert same_bits(out[k].cpu().numpy(), fresh[k].cpu().numpy()), k
    assert not same_bits(fresh["score"].cpu().numpy(), want["score"].cpu().numpy())


# ---- 5: the scan rule --------------------------------------------------------------------------------------------------------------
def scan_np(cand):
    ev, n = [], 0
    while n < cand.size:
        if cand[n]:
            ev.append(n)
            n += 2
        else:
            n += 1
    return np.array(ev, np.int64)


def runs(T, lens, rng, start_at_zero):
    """cand [T] made of runs of the given lengths (cycled) separated by 1..3 non-candidates."""
    c = np.zeros(T, np.uint8)
    p, i = (0 if start_at_zero else 1 + int(rng.integers(0, 3))), 0
    while p < T:
        n = lens[i % len(lens)]
        c[p:p + n] = 1
        p += n + 1 + int(rng.integers(0, 3))
        i += 1
    return c


def test_scan_rule_on_constructed_runs():
    lib = L.load()
    rng = np.random.default_rng(5)
    Ts = [300, 1000, 5000, 256, 257, 513, 5]
    cands = [runs(300, [1, 2, 3, 4, 5], rng, True), runs(1000, [5, 4, 3, 2, 1], rng, False), runs(5000, [1, 2, 3, 4, 5, 2, 1, 4], rng, False),
             np.ones(256, np.uint8),                                             # one run over a whole tile, ending at T - 1
             runs(257, [255, 300], rng, False),                                  # a run that crosses the tile boundary
             (rng.random(513) < 0.5).astype(np.uint8), np.array([0, 1, 1, 1, 1], np.uint8)]
    lengths = np.array([(T - 1) * 512 + 17 for T in Ts], np.int32)              # lengths whose onset-frame counts are Ts
    U = len(Ts)
    assert [1 + int(n) // 512 for n in lengths] == Ts
    assert [c.size for c in cands] == Ts
    meta = np.zeros(lib.eg_beat_tracks_meta_ints(U), np.int32)
    L.check(lib.eg_beat_tracks_meta(C.c_void_p(lengths.ctypes.data), None, None, 15, U, C.c_void_p(meta.ctypes.data)), "meta")
    nbytes = lib.eg_beat_tracks_workspace_bytes(C.c_void_p(lengths.ctypes.data), None, U, 1, 0)
    d_cand = torch.from_numpy(np.concatenate(cands)).to(DEV)
    d_meta = torch.from_numpy(meta).to(DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    events = torch.full((sum(Ts),), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((U,), -1, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.eg_beat_tracks_scan(p(d_cand), C.c_void_p(lengths.ctypes.data), U, p(d_meta), p(ws), nbytes, p(events), p(counts),
                                    C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)), "eg_beat_tracks_scan")
    torch.cuda.synchronize()
    events, counts = events.cpu().numpy(), counts.cpu().numpy()
    off = 0
    for u, c in enumerate(cands):
        want = scan_np(c)
        assert counts[u] == want.size, (u, counts[u], want.size)
        assert np.array_equal(events[off: off + want.size], want), u
        # the rule itself: accepted iff a candidate at an even offset from the start of its run
        start = np.zeros(c.size, np.int64)
        for t in range(c.size):
            start[t] = t if (t == 0 or not c[t - 1]) else start[t - 1]
        assert np.array_equal(np.flatnonzero(c.astype(bool) & ((np.arange(c.size) - start) % 2 == 0)), want), u
        off += c.size


# ---- 6: end to end -------------------------------------------------------------------------------------------------------------------
def test_harness_synthesize_beat_in_its_three_forms():
    from emotiongestures_amd import harness as Hs
    from emotiongestures_amd.beat import beat_alignment_tracks
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.synth import hash_uniform, load_synth_weights
    F_, D_, P_ = 60, 282, 10
    H_ = F_ - P_
    model = build_mirror("spatial", F_, D_, P_, 10, seed=31).to(DEV)
    vae = load_synth_weights(MLP_Reconstruct_v3(), 31).eval().to(DEV)
    U, W, Rd = 2, 3, 3
    hop, n = 53333, (124 - 1) * 512
    total = (W - 1) * hop + n
    audio = torch.from_numpy(noise_bursts(U, total, 120)).to(DEV)
    inp = R.rollout_inputs(U, W, F_, D_, P_, seed=120)
    text, seed_pose = torch.from_numpy(inp["text"]).to(DEV), torch.from_numpy(inp["seed_pose"]).to(DEV)
    labels, z = torch.from_numpy(inp["label"]).to(DEV), torch.from_numpy(inp["z"])

    def both(**kw):
        plain = Hs.synthesize((model, vae), audio, text, seed_pose, **kw)
        beat = Hs.synthesize((model, vae), audio, text, seed_pose, beat=True, **kw)
        torch.cuda.synchronize()
        assert "beat" not in plain and set(beat) == set(plain) | {"beat"}
        for k, v in plain.items():
            assert torch.equal(beat[k], v) if isinstance(v, torch.Tensor) else beat[k] == v, k
        return beat

    # rectangular
    out = both(labels=labels, z=z)
    assert tuple(out["track"].shape) == (U, W * H_ + P_, D_) and out["beat"].shape == (U,) and out["beat"].dtype == torch.float64
    want = beat_alignment_tracks(audio, out["track"])
    assert same_bits(out["beat"].cpu().numpy(), want.cpu().numpy()) and bool(torch.isfinite(out["beat"]).all())
    # lengths=
    lengths = [3 * hop - 100, hop + 700]                                        # 3 and 2 windows
    out = both(labels=labels[:, 0], z=z, lengths=lengths)
    assert out["windows_per"] == [3, 2] and out["beat"].shape == (U,)
    frames = [w * H_ + P_ for w in out["windows_per"]]
    want = beat_alignment_tracks(audio, out["track"], lengths=lengths, frames=frames)
    assert same_bits(out["beat"].cpu().numpy(), want.cpu().numpy()) and bool(torch.isfinite(out["beat"]).all())
    one = beat_alignment_tracks(audio[1:2, :lengths[1]].contiguous(), out["track"][1:2, :frames[1]].contiguous())
    assert same_bits(one.cpu().numpy(), want[1:2].cpu().numpy())               # recording 1 on its own samples and poses only
    # draws=R
    zz = torch.from_numpy(hash_uniform("beat_tracks/z", (U, Rd, W, 32), -2.0, 2.0, 121))
    out = both(labels=labels, z=zz, draws=Rd)
    assert tuple(out["track"].shape) == (U, Rd, W * H_ + P_, D_) and out["beat"].shape == (U, Rd)
    want = beat_alignment_tracks(audio, out["track"])
    assert same_bits(out["beat"].cpu().numpy(), want.cpu().numpy()) and bool(torch.isfinite(out["beat"]).all())
    # the refusals pinned elsewhere stay
    with pytest.raises(L.EgError, match="draws= with lengths= is not supported"):
        Hs.synthesize((model, vae), audio, text, seed_pose, labels=labels, z=zz, draws=Rd, lengths=lengths, beat=True)
