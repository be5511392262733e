"""Emotion recognition of whole tracks, CPU side: the window plan (a host function of the library) against its numpy restatement, the C ABI's
refusals by name before any device use, the numpy path of emotion_votes on hand-made logits, EmotionAccuracy's pooling, the clip metric
(harness.compute_acc) as the one-window case, and the harness's refusals before any model call.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import emotion_np as E
from conftest import build_mirror
from emotiongestures_amd import _lib as L
from emotiongestures_amd import emotion as EM

NEW_SYMBOLS = ("eg_emotion_meta_ints", "eg_emotion_meta", "eg_emotion_window_embed", "eg_emotion_vote_workspace_bytes", "eg_emotion_vote")
F = 12


def _i32(v):
    a = np.ascontiguousarray(v, np.int32)
    return a, C.c_void_p(a.ctypes.data)


def small_classifier(pose_dim, **kw):
    """d_model 64, 8 heads, d_inner 512, 2 layers, n_position 12; heads of 64, the one width the library's attention has."""
    from emotiongestures_amd import harness as H
    return H.SkeletonTransformer(pose_dim=pose_dim, n_position=F, n_layers=2, d_k=64, d_v=64, **kw)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
PLANS = [
    ([F], None, True), ([F + 1], None, True), ([F + 1], None, False),
    ([2 * F + 7, F, 3 * F], F, True), ([2 * F + 7, F, 3 * F], F // 4, True), ([2 * F + 7, F, 3 * F], 1, True),
    ([2 * F + 7, F, 3 * F], 2 * F, True), ([2 * F + 7, F, 3 * F], F // 4, False), ([54000, 60, 9000], 15, True),
]


@pytest.mark.parametrize("frames,stride,tail", PLANS, ids=[f"{f}-{s}-{t}" for f, s, t in PLANS])
def test_plan_equals_restatement_and_the_library_meta(frames, stride, tail):
    window = 60 if max(frames) > 1000 else F
    meta_np, starts = E.plan_np(frames, window, stride, tail)
    plan = EM.window_plan(frames, window, stride, tail)
    U = len(frames)
    assert np.array_equal(plan.meta[:4 * U], meta_np)
    assert plan.total == sum(len(s) for s in starts) and plan.counts.tolist() == [len(s) for s in starts]
    for u in range(U):
        assert plan.starts(u).tolist() == starts[u]
        assert starts[u][0] == 0 and starts[u][-1] + window <= frames[u]
        if tail:                                                    # every valid pose is seen
            seen = np.zeros(frames[u], bool)
            for s in starts[u]:
                seen[s:s + window] = True
            assert seen.all() or (stride or window) > window
    # the raw entry, into a poisoned table
    lib = L.load()
    assert lib.eg_emotion_meta_ints(U) == 4 * U
    raw = np.full(4 * U, -7, np.int32)
    _f, pf = _i32(frames)
    got = lib.eg_emotion_meta(pf, U, window, window if stride is None else stride, int(tail), C.c_void_p(raw.ctypes.data))
    assert got == plan.total and np.array_equal(raw, meta_np)
    assert EM.window_plan(frames, window, stride, tail) is plan     # cached


def test_plan_hand_cases():
    assert E.starts_np(F, F) == [0] and EM.window_plan([F], F).counts.tolist() == [1]
    assert E.starts_np(F + 1, F) == [0, 1] and EM.window_plan([F + 1], F).starts(0).tolist() == [0, 1]
    assert E.starts_np(F + 1, F, tail=False) == [0] and EM.window_plan([F + 1], F, tail=False).starts(0).tolist() == [0]
    # (frames - F) % S == 0: the last strided window already ends at the last pose, no tail window
    for f, S in ((3 * F, F), (F + 9, 3), (2 * F + 7, 1), (F, 5)):
        assert (f - F) % S == 0
        assert EM.window_plan([f], F, S).starts(0).tolist() == EM.window_plan([f], F, S, tail=False).starts(0).tolist() == list(range(0, f - F + 1, S))
    assert EM.window_plan([2 * F + 7], F, 2 * F).starts(0).tolist() == [0, F + 7]      # a stride beyond the window still sees the end


def test_meta_refusals_by_name():
    lib = L.load()
    assert lib.eg_emotion_meta_ints(0) == 0 and lib.eg_emotion_meta_ints(-2) == 0 and lib.eg_emotion_meta_ints(65536) == 0
    meta = np.zeros(64, np.int32)
    pm = C.c_void_p(meta.ctypes.data)
    _g, pg = _i32([30, 12, 40])
    err = lambda: lib.eg_last_error().decode()
    assert lib.eg_emotion_meta(None, 3, F, F, 1, pm) == 0 and "eg_emotion_meta: null frames" in err()
    assert lib.eg_emotion_meta(pg, 3, F, F, 1, None) == 0 and "eg_emotion_meta: null meta" in err()
    assert lib.eg_emotion_meta(pg, 0, F, F, 1, pm) == 0 and "U=0" in err()
    assert lib.eg_emotion_meta(pg, 65536, F, F, 1, pm) == 0 and "U=65536" in err()
    assert lib.eg_emotion_meta(pg, 3, 13, F, 1, pm) == 0 and "frames[1]=12 < window=13" in err()
    assert lib.eg_emotion_meta(pg, 3, 0, F, 1, pm) == 0 and "window=0" in err()
    assert lib.eg_emotion_meta(pg, 3, F, 0, 1, pm) == 0 and "stride=0" in err()
    big = np.full(3, 2 ** 30, np.int32)
    assert lib.eg_emotion_meta(C.c_void_p(big.ctypes.data), 3, F, F, 1, pm) == 0 and "index range" in err()
    two = np.full(2, 2 ** 30 - 1, np.int32)                        # C_u <= frames[u]: the window count stays in range with the frames
    assert lib.eg_emotion_meta(C.c_void_p(two.ctypes.data), 2, 1, 1, 1, pm) == 2 ** 31 - 2
    with pytest.raises(L.EgError, match=re.escape("frames[0]=11 < window=12")):
        EM.window_plan([11], F)


# ---- refusals of the two launching entries -------------------------------------------------------------------------------------------------
def _embed(lib, **over):
    """eg_emotion_window_embed with dummy non-null pointers: every refusal comes before the launch, so nothing is dereferenced."""
    frames = over.pop("frames", [30, 12, 40])
    keep = None if frames is None else _i32(frames)
    dummy = C.c_void_p(256)
    a = dict(emb=dummy, pos=dummy, U=3, R=2, F=F, S=F, tail=1, d_model=64, frames=None if keep is None else keep[1], d_meta=dummy, c0=0, c1=4,
             x=dummy, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    rc = lib.eg_emotion_window_embed(*a.values())
    return rc, lib.eg_last_error().decode()


def _vote(lib, **over):
    counts = over.pop("counts", [3, 1, 4])
    keep = None if counts is None else _i32(counts)
    dummy = C.c_void_p(256)
    a = dict(logits=dummy, U=3, R=2, C=8, counts=None if keep is None else keep[1], d_counts=dummy, d_labels=dummy, ws=dummy, ws_bytes=1 << 40,
             window_class=dummy, votes=dummy, invalid=dummy, mean_logit=dummy, pred=dummy, hit=dummy, window_hits=dummy, accuracy=dummy,
             window_accuracy=dummy, confusion=dummy, window_confusion=dummy, unscored=dummy, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    rc = lib.eg_emotion_vote(*a.values())
    return rc, lib.eg_last_error().decode()


EMBED_REFUSALS = [
    (dict(emb=None), "null emb"), (dict(pos=None), "null pos"), (dict(d_meta=None), "null d_meta"), (dict(x=None), "null x"),
    (dict(frames=None), "null frames"),
    (dict(emb=C.c_void_p(260)), "emb not 16-byte aligned"), (dict(pos=C.c_void_p(264)), "pos not 16-byte aligned"),
    (dict(x=C.c_void_p(264)), "x not 16-byte aligned"),
    (dict(d_model=62), "d_model=62"), (dict(d_model=0), "d_model=0"),
    (dict(R=0), "draws=0"), (dict(R=65), "draws=65"),
    (dict(U=0), "U=0"), (dict(U=65536), "U=65536"),
    (dict(F=0), "window=0"), (dict(S=0), "stride=0"), (dict(frames=[30, 11, 40]), "frames[1]=11 < window=12"),
    (dict(c0=-1), "clips [-1, 4)"), (dict(c1=17), "clips [0, 17) (need 0 <= c0 < c1 <= N=16)"), (dict(c0=4, c1=4), "clips [4, 4)"), (dict(c0=5, c1=3), "clips [5, 3)"),
    (dict(frames=[2 ** 30] * 3, R=64, S=2 ** 20, c1=1), "index range"),
]
VOTE_REFUSALS = [
    (dict(logits=None), "null logits"), (dict(d_counts=None), "null d_counts"), (dict(ws=None), "null workspace"),
    (dict(window_class=None), "null window_class"), (dict(votes=None), "null votes"), (dict(invalid=None), "null invalid"),
    (dict(mean_logit=None), "null mean_logit"), (dict(pred=None), "null pred"), (dict(unscored=None), "null unscored"),
    (dict(hit=None), "null hit"), (dict(window_hits=None), "null window_hits"), (dict(accuracy=None), "null accuracy"),
    (dict(window_accuracy=None), "null window_accuracy"), (dict(confusion=None), "null confusion"),
    (dict(window_confusion=None), "null window_confusion"), (dict(counts=None), "null counts"),
    (dict(ws=C.c_void_p(264)), "workspace not 16-byte aligned"), (dict(mean_logit=C.c_void_p(260)), "mean_logit not 8-byte aligned"),
    (dict(C=1), "classes=1"), (dict(C=65), "classes=65"),
    (dict(U=0), "U=0"), (dict(U=65536), "U=65536"), (dict(R=0), "draws=0"), (dict(R=65), "draws=65"),
    (dict(counts=[3, 0, 4]), "counts[1]=0"),
    (dict(counts=[2 ** 30] * 3), "index range"),
    (dict(ws_bytes=16), "workspace too small"),
]


@pytest.mark.parametrize("over,needle", EMBED_REFUSALS, ids=[f"{list(o)[0]}-{n}" for o, n in EMBED_REFUSALS])
def test_embed_refuses_by_name_before_any_device_use(over, needle):
    lib = L.load()
    before = lib.eg_launch_count()
    rc, msg = _embed(lib, **over)
    assert rc != 0 and "eg_emotion_window_embed" in msg and needle in msg, (rc, msg)
    assert lib.eg_launch_count() == before


@pytest.mark.parametrize("over,needle", VOTE_REFUSALS, ids=[f"{list(o)[0]}-{n}" for o, n in VOTE_REFUSALS])
def test_vote_refuses_by_name_before_any_device_use(over, needle):
    lib = L.load()
    before = lib.eg_launch_count()
    rc, msg = _vote(lib, **over)
    assert rc != 0 and "eg_emotion_vote" in msg and needle in msg, (rc, msg)
    assert lib.eg_launch_count() == before


def test_vote_workspace_is_positive_for_valid_and_zero_for_refused_arguments():
    lib = L.load()
    _c, pc = _i32([130, 64, 1])
    chunks = sum(-(-n // E.CHUNK) for n in [130, 64, 1])
    for R, K in ((1, 2), (3, 8), (64, 64)):
        got = lib.eg_emotion_vote_workspace_bytes(pc, 3, R, K)
        assert got >= R * chunks * (K * 8 + (K + 1) * 4), (R, K, got)      # fp64 sums, int32 counts and the invalid count per (take, chunk)
    for args in ((None, 3, 2, 8), (pc, 0, 2, 8), (pc, 3, 0, 8), (pc, 3, 65, 8), (pc, 3, 2, 1), (pc, 3, 2, 65), (_i32([130, 0, 1])[1], 3, 2, 8)):
        assert lib.eg_emotion_vote_workspace_bytes(*args) == 0, args
    assert EM.vote_workspace_bytes([130, 64, 1], 3, 8) == lib.eg_emotion_vote_workspace_bytes(pc, 3, 3, 8)
    with pytest.raises(L.EgError, match="classes=65"):
        EM.vote_workspace_bytes([130, 64, 1], 3, 65)


# ---- the numpy path on hand-made logits ----------------------------------------------------------------------------------------------------
def hand_made():
    """U = 3 recordings, R = 2 takes, C = 4 classes, counts [4, 2, 1] -> 14 windows; the cases are in the comments."""
    hot = lambda c, v=2.0: [v if k == c else 0.0 for k in range(4)]
    rows = []
    # (0, 0): classes 1, 1, 2, 2: a vote tie; class 2's mean logit is larger (3 > 2)
    rows += [hot(1), hot(1), hot(2, 3.0), hot(2, 3.0)]
    # (0, 1): classes 3, 0, 3, 0 with equal logits: a full tie (votes and means) -> the lowest index, 0
    rows += [hot(3), hot(0), hot(3), hot(0)]
    # (1, 0): a NaN window (invalid) and one window of class 2
    rows += [[0.0, float("nan"), 9.0, 0.0], hot(2)]
    # (1, 1): an inf window (invalid: not the class of its inf) and one window with equal maxima at 1 and 3 -> 1
    rows += [[float("inf"), 0.0, 0.0, 0.0], [0.0, 5.0, -1.0, 5.0]]
    # (2, 0): no valid window: pred -1, unscored, in no confusion cell
    rows += [[float("nan")] * 4]
    # (2, 1): one window, -inf (invalid) -> also unscored
    rows += [[1.0, 2.0, float("-inf"), 0.0]]
    return np.asarray(rows, np.float32), [4, 2, 1], 2, np.asarray([[2, 3], [2, 0], [1, 1]])


def test_numpy_path_on_hand_made_logits():
    logits, counts, R, labels = hand_made()
    res = EM.emotion_votes(logits, counts, R, labels)
    assert res["window_class"].tolist() == [1, 1, 2, 2, 3, 0, 3, 0, -1, 2, -1, 1, -1, -1]
    assert res["pred"].tolist() == [[2, 0], [2, 1], [-1, -1]]
    assert res["votes"][0, 0].tolist() == [0, 2, 2, 0] and res["votes"][0, 1].tolist() == [2, 0, 0, 2]
    assert res["invalid"].tolist() == [[0, 0], [1, 1], [1, 1]]
    assert res["mean_logit"][0, 0].tolist() == [0.0, 1.0, 1.5, 0.0] and res["mean_logit"][0, 1].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert res["mean_logit"][1, 0].tolist() == [0.0, 0.0, 2.0, 0.0]                # the NaN window's 9.0 is not in the mean
    assert np.isnan(res["mean_logit"][2]).all()
    assert res["hit"].tolist() == [[1, 0], [1, 0], [0, 0]] and res["window_hits"].tolist() == [[2, 2], [1, 0], [0, 0]]
    assert int(res["unscored"]) == 2
    assert res["accuracy"] == 100.0 * 2 / 6 and res["window_accuracy"] == 100.0 * 5 / 14
    conf = np.zeros((4, 4), np.int32)
    conf[2, 2] += 2; conf[3, 0] += 1; conf[0, 1] += 1                              # the two takes without a valid window are in no cell
    assert np.array_equal(res["confusion"], conf) and int(res["confusion"].sum()) == 4
    wconf = np.zeros((4, 4), np.int32)
    wconf[2] += [0, 2, 3, 0]; wconf[3] += [2, 0, 0, 2]; wconf[0] += [0, 1, 0, 0]
    assert np.array_equal(res["window_confusion"], wconf) and int(res["window_confusion"].sum()) == 10      # the valid windows
    # the restatement says the same, key by key
    want = E.votes_np(logits, counts, R, labels)
    assert set(want) == set(res)
    for k, v in want.items():
        assert np.array_equal(np.asarray(res[k]), np.asarray(v), equal_nan=True) and np.asarray(res[k]).dtype == np.asarray(v).dtype, k
    # one-hot and index labels: the same result; [U] labels are shared by the takes; CPU tensors in, tensors out
    hot = np.eye(4, dtype=np.float32)[labels]
    for other in (EM.emotion_votes(logits, counts, R, hot), EM.emotion_votes(logits, EM.window_plan([4 * F, 2 * F, F], F), R, labels)):
        for k, v in res.items():
            assert np.array_equal(np.asarray(other[k]), np.asarray(v), equal_nan=True), k
    shared = EM.emotion_votes(logits, counts, R, labels[:, 0])
    assert np.array_equal(shared["hit"], E.votes_np(logits, counts, R, np.repeat(labels[:, :1], 2, 1))["hit"])
    assert np.array_equal(EM.emotion_votes(logits, counts, R, np.eye(4)[labels[:, 0]])["hit"], shared["hit"])
    t = EM.emotion_votes(torch.from_numpy(logits), counts, R, torch.from_numpy(labels))
    assert isinstance(t["pred"], torch.Tensor) and t["pred"].tolist() == res["pred"].tolist() and float(t["accuracy"]) == res["accuracy"]
    # without labels: no label-dependent key
    bare = EM.emotion_votes(logits, counts, R)
    assert set(bare) == {"window_class", "votes", "invalid", "mean_logit", "pred", "unscored"} and int(bare["unscored"]) == 2


def test_python_surface_refusals():
    logits, counts, R, labels = hand_made()
    with pytest.raises(L.EgError, match=re.escape("labels[1, 0]=4 outside [0, 4)")):
        EM.emotion_votes(logits, counts, R, np.asarray([[2, 3], [4, 0], [1, 1]]))
    with pytest.raises(L.EgError, match=re.escape("labels[0, 1]=-1 outside [0, 4)")):
        EM.emotion_votes(logits, counts, R, np.asarray([[2, -1], [1, 0], [1, 1]]))
    with pytest.raises(L.EgError, match="labels shape"):
        EM.emotion_votes(logits, counts, R, np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError, match="draws \\* sum\\(counts\\)"):
        EM.emotion_votes(logits, counts, 3)
    with pytest.raises(L.EgError, match="classes=65"):
        EM.emotion_votes(np.zeros((14, 65), np.float32), counts, R)
    with pytest.raises(L.EgError, match="classes=1"):
        EM.emotion_votes(np.zeros((14, 1), np.float32), counts, R)
    with pytest.raises(L.EgError, match="draws=0"):
        EM.emotion_votes(logits, counts, 0)
    from emotiongestures_amd import harness as H
    skel = small_classifier(126).eval()
    with pytest.raises(RuntimeError, match="track must be a CUDA tensor"):
        EM.window_logits(skel, torch.zeros(1, 2, 30, 126))
    with pytest.raises(L.EgError, match="must be a harness.SkeletonTransformer, got MLP_Reconstruct"):
        EM.window_logits(H.MLP_Reconstruct(pose_dim=126).eval(), torch.zeros(1, 2, 30, 126))
    with pytest.raises(L.EgError, match="heads are 32 / 32 wide; the library's attention has d_k = d_v = 64 only"):
        EM.window_logits(H.SkeletonTransformer(pose_dim=126, n_position=F).eval(), torch.zeros(1, 2, 30, 126))      # the class's default heads
    with pytest.raises(L.EgError, match="EmotionAccuracy.push: the dict has no label figures"):
        EM.EmotionAccuracy().push(EM.emotion_votes(logits, counts, R))


def test_emotion_accuracy_pools_two_pushes_like_one_call_on_the_concatenation():
    rng = np.random.default_rng(3)
    K, R = 8, 3
    counts_a, counts_b = [5, 70, 1], [2, 9]
    mk = lambda counts: rng.standard_normal((R * sum(counts), K)).astype(np.float32)
    la, lb = mk(counts_a), mk(counts_b)
    la[3] = np.nan
    ya, yb = rng.integers(0, K, (3, R)), rng.integers(0, K, (2, R))
    acc = EM.EmotionAccuracy()
    acc.push(EM.emotion_votes(la, counts_a, R, ya))
    acc.push(EM.emotion_votes(torch.from_numpy(lb), counts_b, R, torch.from_numpy(yb)))
    both = EM.emotion_votes(np.concatenate([la, lb]), counts_a + counts_b, R, np.concatenate([ya, yb]))
    assert acc.avg() == both["accuracy"] and acc.window_avg() == both["window_accuracy"]
    assert acc.takes == 5 * R and acc.windows == R * (sum(counts_a) + sum(counts_b)) and acc.unscored == int(both["unscored"])
    assert np.array_equal(acc.confusion, both["confusion"]) and np.array_equal(acc.window_confusion, both["window_confusion"])


@pytest.mark.parametrize("U,R", [(8, 1), (4, 2), (2, 8)])
def test_one_window_per_take_is_the_clip_metric(U, R):
    """With one window per take and unique maxima, accuracy is compute_acc(labels, logits).  compute_acc rounds hits / n and the product with
    100 to float32; with n = U R a power of two both steps are exact, so the float64 figure must be equal, not close."""
    from emotiongestures_amd import harness as H
    rng = np.random.default_rng(U * 10 + R)
    logits = rng.standard_normal((U * R, 8)).astype(np.float32)
    assert all(np.count_nonzero(row == row.max()) == 1 for row in logits)
    labels = np.argmax(logits, 1)
    labels[::3] = (labels[::3] + 1) % 8                             # a third of the takes miss
    res = EM.emotion_votes(logits, [1] * U, R, labels.reshape(U, R))
    want = float(H.compute_acc(torch.from_numpy(labels), torch.from_numpy(logits)))
    assert 0.0 < want < 100.0
    assert res["accuracy"] == want and res["window_accuracy"] == want
    assert np.array_equal(res["pred"].reshape(-1), torch.from_numpy(logits).topk(1, 1)[1].squeeze(1).numpy())


# ---- the harness ---------------------------------------------------------------------------------------------------------------------------
def test_harness_refusals_fire_before_any_model_call():
    from emotiongestures_amd import harness as H

    class NoCall:                                                   # a VAE that must not be reached
        def sample(self, *a, **k):
            raise AssertionError("vae.sample was called")
    gen = build_mirror("spatial", 34, 126, 4, 4, seed=3).eval()    # on the CPU: its engine refuses, so reaching it fails the match below
    skel = small_classifier(126).eval()
    U, W = 2, 3
    audio, text, seed = torch.zeros(U, 3 * 32000), torch.zeros(U, W, 60, dtype=torch.long), torch.zeros(U, 4, 126)
    one = torch.eye(8)[[1, 5]]                                      # [U, 8]
    with pytest.raises(L.EgError, match="synthesize: emotion=: the classifier takes pose_dim=128"):
        H.synthesize((gen, NoCall()), audio, text, seed, one, emotion=small_classifier(128).eval())
    with pytest.raises(L.EgError, match="synthesize_takes: emotion=: the classifier is not in eval mode"):
        H.synthesize_takes((gen, NoCall()), audio, text, seed, one, draws=2, emotion=small_classifier(126).train())
    with pytest.raises(L.EgError, match="synthesize: emotion=: the classifier must be a harness.SkeletonTransformer"):
        H.synthesize((gen, NoCall()), audio, text, seed, one, emotion=H.MLP_Reconstruct(pose_dim=126).eval())
    with pytest.raises(L.EgError, match="emotion_stride=0"):
        H.synthesize((gen, NoCall()), audio, text, seed, one, emotion=skel, emotion_stride=0)
    # labels that change along a take
    moving = torch.eye(8)[torch.tensor([[1, 1, 1], [5, 5, 2]])]                   # [U, W, 8]: recording 1 changes at its last window
    msg = "emotion=: the labels of recording 1, take 0 change along its windows; one label per take"
    with pytest.raises(L.EgError, match="synthesize: " + msg):
        H.synthesize((gen, NoCall()), audio, text, seed, moving, emotion=skel)
    with pytest.raises(L.EgError, match="emotion_of_tracks"):
        H.synthesize((gen, NoCall()), audio, text, seed, moving, emotion=skel)
    with pytest.raises(L.EgError, match="synthesize: " + msg):
        H.synthesize((gen, NoCall()), audio, text, seed, moving, emotion=skel, lengths=[3 * 32000, 3 * 32000], hop_samples=32000)
    per_take = moving[:, None].expand(U, 2, W, 8).clone()
    per_take[1, 0] = per_take[1, 0, 0]                              # take (1, 0) constant now, take (1, 1) still moving
    with pytest.raises(L.EgError, match="the labels of recording 1, take 1 change"):
        H.synthesize_takes((gen, NoCall()), audio, text, seed, per_take, draws=2, emotion=skel, hop_samples=32000)
    with pytest.raises(L.EgError, match="the labels of recording 1, take 1 change"):
        H.synthesize((gen, NoCall()), audio, text, seed, per_take, draws=2, emotion=skel)
    # a shorter recording: the change lies in the padding of recording 1 (2 windows), so the labels pass and the call goes on to the
    # generator, which refuses the CPU
    with pytest.raises(L.EgError, match="runs only on a GPU"):
        H.synthesize((gen, NoCall()), audio, text, seed, moving, emotion=skel, lengths=[3 * 32000, 2 * 32000], hop_samples=32000)
    assert "emotion=" in H.synthesize.__doc__ and "emotion" in H.synthesize_takes.__doc__


def test_new_symbols_are_declared_and_bound():
    import os
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"#define EG_EMOTION_CHUNK_WINDOWS %d\b" % EM.CHUNK_WINDOWS, header) and EM.CHUNK_WINDOWS == E.CHUNK
    assert "may not index outside" in header or "never used as an index" in header
