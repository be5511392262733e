"""Polyphase resampler on the GPU (eg_resample / eg_resample_stream_* through resample.resample_audio, resample.StreamResampler,
harness.synthesize(audio_rate=), GestureStream(audio_rate=) and datapath.clips_from_raw_audio(audio_rate=)) against the float64 direct sum
of tests/resample_np.py and against itself: position in the batch, delay, stream against offline, graph replay against eager.

The element-wise bound of the parity tests is derived, not tuned: K fused multiply-adds on fp32-rounded coefficients leave
|y - y64| <= (K + 2) * 2^-24 * S[n], S[n] = sum_i |x[i]| |h[...]|, for any summation order."""
import numpy as np
import pytest
import torch

import resample_np as R
import rollout_np as RO
from conftest import build_mirror
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import resample as RS
from emotiongestures_amd.synth import hash_uniform, load_synth_weights, synth_audio

pytestmark = pytest.mark.gpu

TILE = RS.TILE
_REF = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def signal(n, seed):
    """Standard-normal noise plus a sine sweep."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / max(n, 1)
    return (rng.standard_normal(n) + np.sin(2 * np.pi * (5.0 + 200.0 * t) * t)).astype(np.float32)


def length_for(target, rate, below=False):
    """The shortest input whose n_out reaches `target`: n_out == target wherever the ratio can give it (always when down-sampling).  Where
    up-sampling skips `target`: the next n_out above it, or with `below` the last one under it."""
    p = R.plan_np(rate)
    n = max(1, target * p["M"] // p["L"])
    while R.out_length_np(n, rate) < target:
        n += 1
    while n > 1 and R.out_length_np(n - 1, rate) >= target:
        n -= 1
    return n - 1 if below and n > 1 and R.out_length_np(n, rate) != target else n


def case(rate):
    """Five rows of unequal length with NaN behind every row's end, and their float64 reference (computed once per rate)."""
    if rate not in _REF:
        p = R.plan_np(rate)
        lens = [1, max(1, p["half"] // p["L"]), length_for(TILE - 1, rate, below=True), length_for(TILE, rate), length_for(2 * TILE + 3, rate)]
        stride = max(lens) + 7
        x = np.full((5, stride), np.nan, np.float32)
        for u, n in enumerate(lens):
            x[u, :n] = signal(n, 1000 * u + rate % 997)
        y64, S = R.resample_rows_np(x, lens, rate)
        _REF[rate] = (p, lens, x, y64, S)
    return _REF[rate]


def bound(p, S):
    return (p["K"] + 2) * 2.0 ** -24 * S


@pytest.mark.parametrize("rate", R.RATES)
def test_parity_with_the_float64_direct_sum(rate):
    p, lens, x, y64, S = case(rate)
    if p["L"] <= p["M"]:
        assert [R.out_length_np(n, rate) for n in lens[2:]] == [TILE - 1, TILE, 2 * TILE + 3]
    pad = 9                                                             # an output stride beyond the longest row: zeros there, too
    out = torch.full((5, y64.shape[1] + pad), float("nan"), device=dev())
    y = RS.resample_audio(torch.from_numpy(x).to(dev()), rate, lengths=lens, out=out).cpu().numpy().astype(np.float64)
    assert not np.isnan(y).any()
    err = np.abs(y[:, :y64.shape[1]] - y64)
    b = bound(p, S)
    print(f"rate {rate}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(b, 1e-300)):.3f}")
    assert (err <= b).all()
    for u, n in enumerate(lens):
        assert not y[u, R.out_length_np(n, rate):].any()                # exact zeros from n_out to the output stride
    # without `out`: the stride is the longest row's n_out
    y2 = RS.resample_audio(torch.from_numpy(x).to(dev()), rate, lengths=lens)
    assert tuple(y2.shape) == y64.shape and np.array_equal(y2.cpu().numpy(), y[:, :y64.shape[1]].astype(np.float32))


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_a_row_does_not_depend_on_its_place_in_the_batch(rate):
    p, lens, x, _y64, _S = case(rate)
    batch = RS.resample_audio(torch.from_numpy(x).to(dev()), rate, lengths=lens)
    for u in (1, 4):
        n = lens[u]
        alone = RS.resample_audio(torch.from_numpy(x[u, :n].copy()).to(dev()), rate)            # [T] in, [n_out] out
        assert alone.dim() == 1 and torch.equal(alone, batch[u, :alone.numel()])
        other = np.full((5, (n + 3) // 4 * 4 + 16), np.nan, np.float32)                         # another position, another in_stride (16-byte rows)
        other[:, :7] = 1.0
        other[(u + 2) % 5, :n] = x[u, :n]
        ln = [7] * 5
        ln[(u + 2) % 5] = n
        got = RS.resample_audio(torch.from_numpy(other).to(dev()), rate, lengths=ln)
        assert torch.equal(got[(u + 2) % 5, :alone.numel()], alone)


def test_equal_rates_return_the_input_itself():
    x = torch.randn(2, 500, device=dev())
    before = L.load().eg_launch_count()
    assert RS.resample_audio(x, 16000) is x and L.load().eg_launch_count() == before


@pytest.mark.parametrize("rate", [48000, 44100, 11025, 8000])
def test_delay_shifts_the_signal_bit_for_bit(rate):
    p = R.plan_np(rate)
    D = RS.stream_delay(rate)
    assert D == p["D"]
    n = length_for(TILE + 37, rate)
    x = signal(n, rate)
    xd = torch.from_numpy(x).to(dev())
    y0, yd = RS.resample_audio(xd, rate), RS.resample_audio(xd, rate, delay=D)
    assert y0.shape == yd.shape and torch.equal(yd[D:], y0[:-D])
    y64, S = R.resample_np(x, rate, delay=D)
    err = np.abs(yd.cpu().numpy().astype(np.float64) - y64)
    assert (err[:D] <= bound(p, S)[:D]).all() and (err <= bound(p, S)).all()


@pytest.mark.parametrize("rate", [48000, 44100, 22050, 8000])
def test_stream_is_the_delayed_offline_signal_bit_for_bit(rate):
    hop, U = 640, 3
    s = RS.StreamResampler(U, rate, hop, device=dev())
    hi = s.hop_in
    assert hi == {48000: 1920, 44100: 1764, 22050: 882, 8000: 320}[rate]
    D = RS.stream_delay(rate)
    n1 = 3 * hi + hi // 3 + 1                                           # row 1 ends inside push 4
    recs = {0: signal(6 * hi, 1), 1: signal(n1, 2), "2a": signal(2 * hi, 3), "2b": signal(4 * hi, 4)}
    outs = []
    for k in range(6):
        chunk = np.full((U, hi), np.nan, np.float32)
        chunk[0] = recs[0][k * hi:(k + 1) * hi]
        seg = recs[1][k * hi:(k + 1) * hi]
        chunk[1, :len(seg)] = seg
        chunk[2] = recs["2a"][k * hi:(k + 1) * hi] if k < 2 else recs["2b"][(k - 2) * hi:(k - 1) * hi]
        ends = [-1, len(seg) if k >= 3 else -1, -1]                     # push 4: the row's last samples; later pushes carry nothing (0)
        if k == 2:
            s.reset(rows=[2])
        outs.append(s.push(torch.from_numpy(chunk).to(dev()), ends))
    got = torch.cat(outs, 1)
    assert not torch.isnan(got).any()
    off = lambda key: RS.resample_audio(torch.from_numpy(recs[key]).to(dev()), rate, delay=D)
    assert torch.equal(got[0], off(0))
    w1 = off(1)
    assert w1.numel() == RS.out_length(n1, rate) and torch.equal(got[1, :w1.numel()], w1) and not got[1, w1.numel():].any()
    assert torch.equal(got[2, :2 * hop], off("2a")) and torch.equal(got[2, 2 * hop:], off("2b"))
    # snapshot / restore bring the history back
    snap = s.snapshot()
    a = s.push(torch.from_numpy(np.stack([signal(hi, 9)] * U)).to(dev()))
    s.restore(snap)
    assert torch.equal(s.push(torch.from_numpy(np.stack([signal(hi, 9)] * U)).to(dev())), a)


def test_offline_call_and_stream_push_replay_from_a_graph():
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    rate = 44100
    _p, lens, x, _y64, _S = case(rate)
    xd = torch.from_numpy(x).to(dev())
    eager = RS.resample_audio(xd, rate, lengths=lens)                   # also the warm-up: bank and lengths are uploaded here
    out = torch.full_like(eager, float("nan"))
    s = RS.StreamResampler(2, rate, 640, device=dev())
    s.chunk.copy_(torch.from_numpy(np.stack([signal(s.hop_in, 5), signal(s.hop_in, 6)])))
    s.run()
    snap = s.snapshot()
    eager_push = s.run().clone()
    eager_hist = s.snapshot()
    s.restore(snap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):      # one stream, no side branches
        RS.resample_audio(xd, rate, lengths=lens, out=out)
        s.run()
    s.out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(s.out, eager_push) and torch.equal(s.snapshot(), eager_hist)


# ---- integration -------------------------------------------------------------------------------------------------------------------------
F_, D_, P_ = 34, 126, 4
H_ = F_ - P_
HOP, N = 32000, (124 - 1) * 512
_MODELS = {}


def ted():
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    if "ted" not in _MODELS:
        _MODELS["ted"] = (build_mirror("spatial", F_, D_, P_, 4, seed=7, precision="bf16x3").to(dev()),
                          load_synth_weights(MLP_Reconstruct_v3(frames=F_), 7).eval().to(dev()))
    return _MODELS["ted"]


def same(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        assert torch.equal(v, b[k]) if isinstance(v, torch.Tensor) else v == b[k], k


def test_synthesize_resamples_once_then_runs_unchanged():
    model, vae = ted()
    U, W = 2, 3
    inp = RO.rollout_inputs(U, 4, F_, D_, P_, seed=80)
    g = {k: torch.from_numpy(inp[k]).to(dev()) for k in ("text", "seed_pose", "label", "z")}
    T16 = 2 * HOP + N - 9000
    # rectangular, 48 kHz
    a48 = torch.from_numpy(synth_audio(U, 3 * T16, seed=80)).to(dev())
    kw = dict(labels=g["label"][:, :W].contiguous(), hop_samples=HOP, z=g["z"][:, :W].contiguous())
    got = Hs.synthesize((model, vae), a48, g["text"][:, :W].contiguous(), g["seed_pose"], audio_rate=48000, **kw)
    a16 = RS.resample_audio(a48, 48000)
    assert tuple(a16.shape) == (U, T16) and torch.equal(got["audio"], a16)
    want = Hs.synthesize((model, vae), a16, g["text"][:, :W].contiguous(), g["seed_pose"], **kw)
    assert "audio" not in want and set(got) == set(want) | {"audio"}
    same({k: v for k, v in got.items() if k != "audio"}, want)
    same(Hs.synthesize((model, vae), a16, g["text"][:, :W].contiguous(), g["seed_pose"], audio_rate=16000, **kw), want)    # equal rates: today's call
    # lengths=, 44.1 kHz
    lens = [int(T16 * 441 / 160) - 5, 200000]
    a44 = torch.full((U, max(lens) + 3), float("nan"), device=dev())
    for u, n in enumerate(lens):
        a44[u, :n] = torch.from_numpy(synth_audio(1, n, seed=81 + u)[0])
    l16 = [RS.out_length(n, 44100) for n in lens]
    Wu = [-(-n // HOP) for n in l16]
    assert Wu == [4, 3]
    kw = dict(labels=g["label"][:, 0].contiguous(), hop_samples=HOP, z=g["z"])
    got = Hs.synthesize((model, vae), a44, g["text"], g["seed_pose"], lengths=lens, audio_rate=44100, **kw)
    r16 = RS.resample_audio(a44, 44100, lengths=lens)
    assert torch.equal(got["audio"], r16) and got["lengths"] == l16 and got["windows_per"] == Wu
    want = Hs.synthesize((model, vae), r16, g["text"], g["seed_pose"], lengths=l16, **kw)
    same({k: v for k, v in got.items() if k not in ("audio", "lengths")}, want)
    # draws=2, 24 kHz
    a24 = torch.from_numpy(synth_audio(U, T16 * 3 // 2, seed=83)).to(dev())
    zz = torch.from_numpy(hash_uniform("resample/z", (U, 2, W, 32), -2.0, 2.0, 84))
    kw = dict(labels=g["label"][:, :W].contiguous(), hop_samples=HOP, z=zz, draws=2)
    got = Hs.synthesize((model, vae), a24, g["text"][:, :W].contiguous(), g["seed_pose"], audio_rate=24000, **kw)
    want = Hs.synthesize((model, vae), RS.resample_audio(a24, 24000), g["text"][:, :W].contiguous(), g["seed_pose"], **kw)
    assert tuple(got["track"].shape) == (U, 2, W * H_ + P_, D_) and torch.equal(got["audio"], RS.resample_audio(a24, 24000))
    same({k: v for k, v in got.items() if k != "audio"}, want)


def test_synthesize_beat_scores_the_resampled_audio():
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    Fb, Db, Pb = 60, 282, 10
    model = build_mirror("spatial", Fb, Db, Pb, 10, seed=31).to(dev())
    vae = load_synth_weights(MLP_Reconstruct_v3(), 31).eval().to(dev())
    U, W = 2, 2
    hop = 53333
    total = (W - 1) * hop + N
    rng = np.random.default_rng(5)
    a = 0.05 * rng.standard_normal((U, 3 * total)).astype(np.float32)
    for k in range(0, 3 * total, 3 * 7000):                            # bursts: onsets for the beat score
        a[:, k:k + 3 * 800] += rng.standard_normal((U, min(3 * 800, 3 * total - k))).astype(np.float32)
    a48 = torch.from_numpy(a).to(dev())
    inp = RO.rollout_inputs(U, W, Fb, Db, Pb, seed=120)
    text, seed_pose = torch.from_numpy(inp["text"]).to(dev()), torch.from_numpy(inp["seed_pose"]).to(dev())
    kw = dict(labels=torch.from_numpy(inp["label"]).to(dev()), z=torch.from_numpy(inp["z"]), hop_samples=hop, beat=True)
    got = Hs.synthesize((model, vae), a48, text, seed_pose, audio_rate=48000, **kw)
    want = Hs.synthesize((model, vae), RS.resample_audio(a48, 48000), text, seed_pose, **kw)
    assert got["beat"].shape == (U,) and np.array_equal(got["beat"].cpu().numpy().view(np.uint64), want["beat"].cpu().numpy().view(np.uint64))
    assert torch.equal(got["track"], want["track"])


def test_gesture_stream_at_48k_is_synthesize_on_the_delayed_resampled_audio():
    """Both rows end inside the fourth push.  Rows + tail against synthesize, compared as tests/test_gpu_stream.py compares (U = 2: bit for
    bit); graph=True against graph=False: the resampler's history is snapshotted around the capture, or the two would differ."""
    model, vae = ted()
    U, rate = 2, 48000
    T_in = 3 * (2 * HOP + N - 9000) + 1
    a48 = torch.from_numpy(synth_audio(U, T_in, seed=80)).to(dev())
    inp = RO.rollout_inputs(U, 4, F_, D_, P_, seed=80)
    g = {k: torch.from_numpy(inp[k]).to(dev()) for k in ("text", "seed_pose", "label", "z")}
    hop_in = 3 * HOP
    padded = torch.full((U, 4 * hop_in), float("nan"), device=dev())
    padded[:, :T_in] = a48
    col = lambda k: max(0, k - 2)

    def run(graph):
        s = Hs.open_stream((model, vae), U, g["seed_pose"], hop_samples=HOP, audio_rate=rate, graph=graph)
        assert (s.hop, s.hop_in, s.lag) == (HOP, hop_in, 2)
        rows, valids = [], []
        for k in range(1, 5):
            r, v = s.push(padded[:, (k - 1) * hop_in: k * hop_in].contiguous(), g["text"][:, col(k)], g["label"][:, col(k)], g["z"][:, col(k)],
                          ends=T_in - 3 * hop_in if k == 4 else None)
            rows.append(r)
            valids.append(v.cpu().tolist())
        assert rows[0] is None and valids == [[0] * U] + [[1] * U] * 3
        r5, v5 = s.push(padded[:, :hop_in].contiguous(), g["text"][:, 3], g["label"][:, 3], g["z"][:, 3])    # ended rows: the chunk is ignored
        assert v5.cpu().tolist() == [1] * U
        out3, out4 = torch.cat(rows[1:] + [s.tail()], 1), None
        out4 = torch.cat(rows[1:] + [r5, s.tail()], 1)
        with pytest.raises(L.EgError, match=r"audio shape .* != \(2,96000\)"):
            s.push(padded[:, :HOP].contiguous(), g["text"][:, 3], g["label"][:, 3], g["z"][:, 3])
        return out3, out4

    got3, got4 = run(True)
    a16 = RS.resample_audio(a48, rate, delay=RS.stream_delay(rate))
    assert a16.shape[1] == RS.out_length(T_in, rate) == 2 * HOP + N - 9000 + 1
    W = 4
    want = Hs.synthesize((model, vae), a16, g["text"][:, :W].contiguous(), g["seed_pose"], labels=g["label"][:, :W].contiguous(), hop_samples=HOP,
                         z=g["z"][:, :W].contiguous(), windows=W)["track"]
    assert got4.shape == want.shape and torch.equal(got4, want)
    assert torch.equal(got3[:, :3 * H_], want[:, :3 * H_])
    eager3, eager4 = run(False)
    assert torch.equal(eager3, got3) and torch.equal(eager4, got4)


def test_clips_from_raw_audio_at_44k1():
    from emotiongestures_amd import datapath as DP
    seconds, fps_in, joints = 9.0, 30, 43
    a44 = synth_audio(1, int(seconds * 44100), seed=5)[0]
    skel = np.zeros((int(seconds * fps_in), joints, 3), np.float32)
    words = [["w%d" % i, 0.3 * i, 0.3 * i + 0.2] for i in range(30)]
    got = DP.clips_from_raw_audio("2_scott_0_70_70", a44, skel, words, fps_in, device=dev(), audio_rate=44100)["clips"][0]
    a16 = RS.resample_audio(torch.from_numpy(a44).to(dev()), 44100).cpu().numpy()
    want = DP.clips_from_raw_audio("2_scott_0_70_70", a16, skel, words, fps_in, device=dev())["clips"][0]
    assert got["audio_raw"].shape == (int(seconds * 16000),) and np.array_equal(got["audio_raw"], want["audio_raw"])
    assert np.array_equal(got["audio_feat"], want["audio_feat"])
    assert got["end_time"] == seconds and got["end_frame_no"] == want["end_frame_no"]
