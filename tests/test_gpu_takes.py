"""Take diversity on the GPU (csrc/takes.hip through emotiongestures_amd.takes and harness.synthesize(diversity=)): (1) the pack kernel bit for
bit against torch indexing, (2) the features bit for bit against the FGD module on the same packed rows, (3) the fp64 distance against the
numpy restatement (tests/takes_np.py) computed from the same fp32 features, (4) its exact properties, (5) span, (6) graph capture, (7) end to
end from raw audio.

Tolerance of (3): an fp64 sum of n non-negative terms has relative error <= n * 2^-53; at the largest case here (n = 1000 * 512 = 512 000)
that is 5.7e-11 before the square root halves it, so RTOL = 1e-9 leaves more than a tenfold margin, and an fp32 accumulation (1e-7 and
worse) fails it."""
import ctypes as C

import numpy as np
import pytest
import torch

import rollout_np as RN
import takes_np as T
from conftest import build_mirror
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as H
from emotiongestures_amd import takes
from emotiongestures_amd.synth import hash_uniform, load_synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RTOL = 1e-9
FRAMES = [70, 34, 5, 1]                 # crosses a chunk boundary for any chunk <= 64; a one-frame recording


def same_bits(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def nan_track(U, R, Tmax, D, frames, seed):
    """N(0,1) poses, every row at or beyond frames[u] NaN."""
    rng = np.random.default_rng(seed)
    trk = rng.standard_normal((U, R, Tmax, D)).astype(np.float32)
    for u, f in enumerate(frames):
        trk[u, :, f:] = np.nan
    return trk


def torch_rows(trk, frames, pad=True):
    """The packed matrix by torch indexing (plus zero columns)."""
    U, R, _T, D = trk.shape
    u, r, t = (torch.from_numpy(a).to(trk.device) for a in T.packed_index(frames, R))
    rows = trk[u, r, t]
    if not pad or D % 4 == 0:
        return rows.contiguous()
    out = torch.zeros(rows.shape[0], (D + 3) // 4 * 4, device=trk.device)
    out[:, :D] = rows
    return out


def features(frames, R, seed, K=512):
    """N(0,1) * 8 plus a per-take offset, packed [N, K] fp32: distances neither tiny nor equal."""
    rng = np.random.default_rng(seed)
    _u, r, _t = T.packed_index(frames, R)
    return (rng.standard_normal((r.size, K)) * 8 + 0.75 * r[:, None]).astype(np.float32)


def run_distance(feat, frames, R, **kw):
    out = takes.take_distance(torch.from_numpy(feat).to(DEV), frames, R, **kw)
    torch.cuda.synchronize()
    return out["distance"].cpu().numpy(), out["diversity"].cpu().numpy()


# ---- 1: pack -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [282, 126, 128])
@pytest.mark.parametrize("R", [3, 1])
def test_pack_equals_torch_indexing_bit_for_bit(D, R):
    frames = [9, 4, 1]
    trk = torch.from_numpy(nan_track(3, R, 9, D, frames, 40 + D)).to(DEV)
    rows, fr, off = takes.pack_rows(trk if R > 1 else trk[:, 0], frames)         # R = 1: from a 3-d track
    torch.cuda.synchronize()
    assert fr == frames and off == [0, 9, 13]
    want = torch_rows(trk, frames)
    assert tuple(rows.shape) == (R * 14, (D + 3) // 4 * 4)
    assert same_bits(rows, want)
    assert not bool(torch.isnan(rows).any())


def test_pack_scalar_loads_from_a_misaligned_source_and_the_grid_stride():
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    # D % 4 == 0 but the source starts 4 bytes off a 16-byte boundary: scalar loads
    frames, R, Tmax, D = [9, 4, 1], 3, 9, 128
    trk = torch.from_numpy(nan_track(3, R, Tmax, D, frames, 7)).to(DEV)
    flat = torch.empty(trk.numel() + 1, device=DEV)
    flat[1:].copy_(trk.reshape(-1))
    fr = np.ascontiguousarray(frames, np.int32)
    meta = torch.from_numpy(T.meta_np(frames)).to(DEV)
    rows = torch.full((R * 14, D), 7.0, device=DEV)
    L.check(lib.eg_track_rows_pack(C.c_void_p(flat.data_ptr() + 4), 3, R, Tmax, D, C.c_void_p(fr.ctypes.data), C.c_void_p(meta.data_ptr()),
                                   C.c_void_p(rows.data_ptr()), st), "eg_track_rows_pack")
    torch.cuda.synchronize()
    assert same_bits(rows, torch_rows(trk, frames))
    # more quads in one recording than the grid has threads: the stride loop (2 * 4100 * 128 quads > 4096 * 256)
    frames, R, Tmax, D = [4100], 2, 4101, 512
    trk = torch.from_numpy(nan_track(1, R, Tmax, D, frames, 8)).to(DEV)
    rows, _f, _o = takes.pack_rows(trk, frames)
    torch.cuda.synchronize()
    assert same_bits(rows, trk[0, :, :4100].reshape(R * 4100, D))


# ---- 2: features ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("D", [282, 126, 128])
def test_track_features_equal_the_fgd_module_on_the_packed_rows(D, precision):
    frames, R = [9, 4, 1], 3
    fgd = load_synth_weights(H.MLP_Reconstruct(pose_dim=D, precision=precision), 5).eval().to(DEV)
    trk = torch.from_numpy(nan_track(3, R, 9, D, frames, 50 + D) * np.float32(0.5)).to(DEV)
    with torch.no_grad():
        feat, fr, off = takes.track_features(fgd, trk, frames)
        want = fgd(torch_rows(trk, frames, pad=False))[1]                       # the same row count, hence the same product path
        one, _f, _o = takes.track_features(fgd, trk[:, 0], frames)              # R = 1 from a 3-d track
        want_one = fgd(torch_rows(trk[:, :1], frames, pad=False))[1]
    torch.cuda.synchronize()
    assert tuple(feat.shape) == (R * 14, 512) and fr == frames and off == [0, 9, 13]
    assert bool(torch.isfinite(feat).all())
    assert same_bits(feat, want)
    assert same_bits(one, want_one)


# ---- 3: distance against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 3, 5])
def test_distance_equals_the_float64_restatement(R):
    feat = features(FRAMES, R, 60 + R)
    want_d, want_v = T.take_distance_np(feat, FRAMES, R)
    dist, div = run_distance(feat, FRAMES, R)
    off = ~np.eye(R, dtype=bool)
    print("max rel err distance", np.abs(dist / np.where(want_d == 0, 1, want_d) - 1)[:, off].max(), "diversity", np.abs(div / want_v - 1).max())
    assert dist.shape == (4, R, R) and dist.dtype == np.float64 and div.shape == (4,) and div.dtype == np.float64
    assert (want_d[:, off] > 1.0).all()
    np.testing.assert_allclose(dist, want_d, rtol=RTOL, atol=0)
    np.testing.assert_allclose(div, want_v, rtol=RTOL, atol=0)


def test_many_chunks_against_the_restatement():
    frames, R = [1000], 2
    feat = features(frames, R, 71)
    want_d, want_v = T.take_distance_np(feat, frames, R)
    dist, div = run_distance(feat, frames, R)
    print("max rel err", abs(dist[0, 0, 1] / want_d[0, 0, 1] - 1))
    np.testing.assert_allclose(dist, want_d, rtol=RTOL, atol=0)
    np.testing.assert_allclose(div, want_v, rtol=RTOL, atol=0)


@pytest.mark.parametrize("K,R,frames", [(64, 3, [20, 3]), (520, 3, [20, 3]), (1024, 2, [33]), (512, 64, [17, 1])])
def test_other_widths_and_the_most_draws(K, R, frames):
    """K < 512 (part of the register tile), K > 512 (the path that re-reads both takes), and draws = 64 (2016 pairs per recording)."""
    feat = features(frames, R, 80 + K + R, K=K)
    want_d, want_v = T.take_distance_np(feat, frames, R)
    dist, div = run_distance(feat, frames, R)
    np.testing.assert_allclose(dist, want_d, rtol=RTOL, atol=0)
    np.testing.assert_allclose(div, want_v, rtol=RTOL, atol=0)
    assert np.array_equal(dist, dist.transpose(0, 2, 1)) and not dist[:, np.eye(R, dtype=bool)].any()


# ---- 4: exact properties -------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    R, U = 5, len(FRAMES)
    feat = features(FRAMES, R, 90)
    blocks = [T.takes_of(feat, FRAMES, R, u).copy() for u in range(U)]          # [R, f, K] per recording
    for b in blocks:
        b[2] = b[0]                                                             # take 2 is a copy of take 0
    pack = lambda bl: np.concatenate([b.reshape(-1, 512) for b in bl])
    feat = pack(blocks)
    dist, div = run_distance(feat, FRAMES, R)
    # symmetric bit for bit, the diagonal exactly zero
    assert same_bits(dist, np.ascontiguousarray(dist.transpose(0, 2, 1)))
    assert not dist[:, np.eye(R, dtype=bool)].any() and not np.signbit(dist[:, np.eye(R, dtype=bool)]).any()
    # a copied take: exactly zero apart, and its row is the original's
    assert not dist[:, 0, 2].any() and same_bits(dist[:, 0, :], dist[:, 2, :])
    assert (dist[:, 0, 1] > 0).all() and np.isfinite(dist).all() and np.isfinite(div).all()
    # two calls: the same bits
    again, again_v = run_distance(feat, FRAMES, R)
    assert same_bits(dist, again) and same_bits(div, again_v)
    # permuting the draws permutes the matrix
    perm = [3, 0, 4, 1, 2]
    dist_p, _ = run_distance(pack([b[perm] for b in blocks]), FRAMES, R)
    assert same_bits(dist_p, dist[:, perm][:, :, perm])
    # a recording alone gets the bits it gets in the batch
    for u in range(U):
        d1, v1 = run_distance(blocks[u].reshape(-1, 512), [FRAMES[u]], R)
        assert same_bits(d1[0], dist[u]) and same_bits(v1[0], div[u]), u


def test_nan_beyond_frames_of_a_padded_track_never_appears():
    R, D = 3, 126
    fgd = load_synth_weights(H.MLP_Reconstruct(pose_dim=D), 5).eval().to(DEV)
    trk = nan_track(len(FRAMES), R, 70, D, FRAMES, 95) * np.float32(0.5)
    zero = np.nan_to_num(trk, nan=0.0)
    with torch.no_grad():
        a = takes.take_diversity(fgd, torch.from_numpy(trk).to(DEV), FRAMES)
        b = takes.take_diversity(fgd, torch.from_numpy(zero).to(DEV), FRAMES)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a["distance"]).all()) and bool(torch.isfinite(a["diversity"]).all())
    assert same_bits(a["distance"], b["distance"]) and same_bits(a["diversity"], b["diversity"])
    assert bool((a["diversity"] > 0).all())


# ---- 5: span -------------------------------------------------------------------------------------------------------------------------
def test_span():
    R = 3
    feat = features([34, 34], R, 100)
    raw, raw_v = run_distance(feat, [34, 34], R)
    same, same_v = run_distance(feat, [34, 34], R, span=34)
    assert same_bits(raw, same) and same_bits(raw_v, same_v)                   # frames == span: scale is exactly 1
    frames = [68, 34]
    feat = features(frames, R, 101)
    raw, _ = run_distance(feat, frames, R)
    got, _ = run_distance(feat, frames, R, span=34)
    want = raw * np.sqrt(34.0 / np.asarray(frames, np.float64))[:, None, None]
    np.testing.assert_allclose(got, want, rtol=4e-15, atol=0)
    assert same_bits(got[1], raw[1])


# ---- 6: graph ------------------------------------------------------------------------------------------------------------------------
def test_take_diversity_captures_into_a_graph_and_follows_the_data():
    U, R, Tmax, D = 2, 3, 20, 126
    frames = [20, 7]
    fgd = load_synth_weights(H.MLP_Reconstruct(pose_dim=D), 5).eval().to(DEV)
    contents = [torch.from_numpy(nan_track(U, R, Tmax, D, frames, 110 + i) * np.float32(0.5)).to(DEV) for i in range(3)]
    trk = contents[0].clone()
    with torch.no_grad():
        takes.take_diversity(fgd, trk, frames, span=34)                         # eager warm-up: packs the weights, uploads the meta table
        torch.cuda.synchronize()
        ws = torch.empty(takes.workspace_bytes(frames, R), dtype=torch.uint8, device=DEV)
        out = {"distance": torch.zeros(U, R, R, dtype=torch.float64, device=DEV), "diversity": torch.zeros(U, dtype=torch.float64, device=DEV)}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            takes.take_diversity(fgd, trk, frames, span=34, workspace=ws, out=out)
        for new in contents[1:]:
            trk.copy_(new)
            for v in out.values():
                v.zero_()
            g.replay()
            torch.cuda.synchronize()
            eager = takes.take_diversity(fgd, new, frames, span=34)
            torch.cuda.synchronize()
            assert same_bits(out["distance"], eager["distance"]) and same_bits(out["diversity"], eager["diversity"])
            assert bool((out["diversity"] > 0).all())


# ---- 7: end to end -------------------------------------------------------------------------------------------------------------------
def test_harness_synthesize_diversity_end_to_end():
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    F_, D_, P_ = 60, 282, 10
    model = build_mirror("spatial", F_, D_, P_, 10, seed=31).to(DEV)
    vae = load_synth_weights(MLP_Reconstruct_v3(), 31).eval().to(DEV)
    fgd = load_synth_weights(H.MLP_Reconstruct(), 31).eval().to(DEV)
    U, W, Rd = 2, 2, 3
    hop, n = 53333, (124 - 1) * 512
    total = (W - 1) * hop + n
    audio = torch.from_numpy(np.random.default_rng(120).standard_normal((U, total)).astype(np.float32) * np.float32(0.1)).to(DEV)
    inp = RN.rollout_inputs(U, W, F_, D_, P_, seed=120)
    text, seed_pose = torch.from_numpy(inp["text"]).to(DEV), torch.from_numpy(inp["seed_pose"]).to(DEV)
    labels = torch.from_numpy(inp["label"]).to(DEV)
    zz = torch.from_numpy(hash_uniform("takes/z", (U, Rd, W, 32), -2.0, 2.0, 121))
    plain = H.synthesize((model, vae), audio, text, seed_pose, labels=labels, z=zz, draws=Rd)
    out = H.synthesize((model, vae), audio, text, seed_pose, labels=labels, z=zz, draws=Rd, diversity=fgd)
    torch.cuda.synchronize()
    assert set(out) == set(plain) | {"take_distance", "take_diversity"}
    for k, v in plain.items():
        assert same_bits(out[k], v) if isinstance(v, torch.Tensor) else out[k] == v, k
    assert tuple(out["track"].shape) == (U, Rd, W * (F_ - P_) + P_, D_)
    want = takes.take_diversity(fgd, out["track"], span=F_)
    torch.cuda.synchronize()
    assert same_bits(out["take_distance"], want["distance"]) and same_bits(out["take_diversity"], want["diversity"])
    d = out["take_distance"].cpu().numpy()
    assert d.shape == (U, Rd, Rd) and d.dtype == np.float64 and out["take_diversity"].shape == (U,)
    off = ~np.eye(Rd, dtype=bool)
    assert np.isfinite(d).all() and (d[:, off] > 0).all() and not d[:, ~off].any()
    with pytest.raises(L.EgError, match="diversity= needs draws >= 2"):
        H.synthesize((model, vae), audio, text, seed_pose, labels=labels, z=zz[:, 0], diversity=fgd)
