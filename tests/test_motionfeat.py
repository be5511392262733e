"""Motion-clip features of whole tracks, the part that needs no GPU (emotiongestures_amd.motionfeat, csrc/motionfeat.hip): the window geometry
against its definition, the run plan of the kernel (every clip owned once, nothing staged beyond a recording's poses), and every refusal of the
C entry point and of the Python layers above it -- each returns before the first launch, so the fake (aligned) addresses are never touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import motionfeat_np as MN
from conftest import build_mirror
from emotiongestures_amd import _lib as L
from emotiongestures_amd import emotion as EM
from emotiongestures_amd import harness as H
from emotiongestures_amd import motionfeat as MF
from emotiongestures_amd import takes
from emotiongestures_amd.model.motion_ae import MotionAE

P = C.c_void_p
EG_ERR_BAD_ARG, EG_ERR_ALIGN = -1, -5         # include/emogest.h: EgStatus
FRAMES = [34, 35, 103]
STRIDES = [1, 2, 17, 34, 40]
WHO = "eg_motion_window_rows"


# ---- window geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("stride", STRIDES)
def test_clip_counts_and_order_equal_the_window_plan(stride, tail):
    R = 2
    plan = EM.window_plan(FRAMES, 34, stride, tail)
    want = MN.clip_list(FRAMES, R, stride, tail)
    assert plan.counts.tolist() == [len(MN.window_starts(f, stride, tail)) for f in FRAMES]
    u, r, s = MF.clip_index(plan, R)
    assert list(zip(u.tolist(), r.tolist(), s.tolist())) == want and len(want) == R * plan.total
    # clip R * coff[u] + r * C_u + j is window j of take r of recording u
    for i, (uu, rr, ss) in enumerate(want):
        j = i - (R * int(plan.coff[uu]) + rr * int(plan.counts[uu]))
        assert 0 <= j < plan.counts[uu] and plan.starts(uu)[j] == ss


def test_constants_and_the_run_plan():
    """A run of eg_motion_run_windows(S) strided windows stages at most EG_MOTION_RUN_FRAMES poses, all of them inside the recording, and the
    runs of a take (the tail window a run of its own) own every clip exactly once."""
    assert (MF.WINDOW, MF.ROW_FLOATS, MF.MAX_POSE_DIM, MF.RUN_FRAMES) == (34, 384, 128, 136)
    assert MF.run_windows(34) == 4 and MF.run_windows(1) == 96 and MF.run_windows(17) == 6 and MF.run_windows(1000) == 4
    with pytest.raises(L.EgError, match="stride=0"):
        MF.run_windows(0)
    for stride in list(range(1, 45)) + [100]:
        W = MF.run_windows(stride)
        staged = W * 34 if stride >= 34 else (W - 1) * stride + 34
        assert W >= 1 and staged <= MF.RUN_FRAMES, (stride, W, staged)
        for f in (34, 35, 34 + 2 * MF.RUN_FRAMES + 3):
            starts = MN.window_starts(f, stride, True)
            strided = (f - 34) // stride + 1
            owned = []
            for j0 in range(0, strided, W):
                run = starts[j0:min(j0 + W, strided)]
                assert run[-1] + 34 <= f
                owned += run
            owned += starts[strided:]                               # the tail run
            assert owned == starts and len(starts) - strided in (0, 1)


# ---- the C entry point ---------------------------------------------------------------------------------------------------------------
TRACK, ROWS, TABLE, WEIGHT = P(1 << 20), P(1 << 24), P(1 << 12), P(1 << 16)


def call(lib, track=TRACK, U=2, R=2, Tmax=50, D=126, window=34, stride=34, tail=1, frames=(40, 50), d_frames=TABLE, weights=None, c0=0,
         c1=4, rows=ROWS):
    fr = None if frames is None else (C.c_int32 * len(frames))(*frames)
    w = [WEIGHT] * 8 if weights is None else weights
    rc = lib.eg_motion_window_rows(track, U, R, Tmax, D, window, stride, tail, fr, d_frames, *w, c0, c1, rows, None)
    return rc, lib.eg_last_error().decode()


def test_every_refusal_of_the_entry_point_by_name():
    lib = L.load()
    names = ["w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4"]
    cases = [(dict(track=None), EG_ERR_BAD_ARG, f"{WHO}: null track"),
             (dict(frames=None), EG_ERR_BAD_ARG, f"{WHO}: null frames"),
             (dict(d_frames=None), EG_ERR_BAD_ARG, f"{WHO}: null d_frames"),
             (dict(rows=None), EG_ERR_BAD_ARG, f"{WHO}: null rows"),
             (dict(track=P(TRACK.value + 4)), EG_ERR_ALIGN, f"{WHO}: track not 16-byte aligned"),
             (dict(rows=P(ROWS.value + 8)), EG_ERR_ALIGN, f"{WHO}: rows not 16-byte aligned"),
             (dict(U=0), EG_ERR_BAD_ARG, f"{WHO}: U=0 (1..65535)"),
             (dict(U=65536), EG_ERR_BAD_ARG, f"{WHO}: U=65536 (1..65535)"),
             (dict(R=0), EG_ERR_BAD_ARG, f"{WHO}: draws=0 (1..64)"),
             (dict(R=65), EG_ERR_BAD_ARG, f"{WHO}: draws=65 (1..64)"),
             (dict(D=0), EG_ERR_BAD_ARG, f"{WHO}: pose_dim=0 (1..128)"),
             (dict(D=129), EG_ERR_BAD_ARG, f"{WHO}: pose_dim=129 (1..128)"),
             (dict(window=33), EG_ERR_BAD_ARG, f"{WHO}: window=33 (the encoder's out_net is sized for 34 frames)"),
             (dict(window=60), EG_ERR_BAD_ARG, f"{WHO}: window=60 (the encoder's out_net is sized for 34 frames)"),
             (dict(stride=0), EG_ERR_BAD_ARG, f"{WHO}: stride=0 (need >= 1)"),
             (dict(frames=(40, 33)), EG_ERR_BAD_ARG,
              f"{WHO}: frames[1]=33 < window=34 (the encoder takes whole windows: no padding, no resampling)"),
             (dict(frames=(51, 40)), EG_ERR_BAD_ARG, f"{WHO}: frames[0]=51 > Tmax=50"),
             (dict(c0=-1), EG_ERR_BAD_ARG, f"{WHO}: clips [-1, 4) (need 0 <= c0 < c1 <= N=8)"),
             (dict(c1=9), EG_ERR_BAD_ARG, f"{WHO}: clips [0, 9) (need 0 <= c0 < c1 <= N=8)"),
             (dict(c0=3, c1=3), EG_ERR_BAD_ARG, f"{WHO}: clips [3, 3) (need 0 <= c0 < c1 <= N=8)"),
             (dict(d_frames=P(TABLE.value + 2)), EG_ERR_ALIGN, f"{WHO}: d_frames not 4-byte aligned")]
    for i, n in enumerate(names):
        w = [WEIGHT] * 8
        w[i] = None
        cases.append((dict(weights=w), EG_ERR_BAD_ARG, f"{WHO}: null {n}"))
    for kw, code, text in cases:
        rc, msg = call(lib, **kw)
        assert rc == code and msg == text, (kw, rc, msg)
    # frames (40, 50) at stride 34 with the tail: 2 + 2 windows, two takes each -> N = 8 (the range messages above); without it 1 + 1
    rc, msg = call(lib, tail=0, c1=5)
    assert rc == EG_ERR_BAD_ARG and msg == f"{WHO}: clips [0, 5) (need 0 <= c0 < c1 <= N=4)"


def test_the_constants_of_the_header_are_the_bindings():
    """The symbols themselves are cross-checked by tests/test_abi_and_dist.py; the #defines are not."""
    import os
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    for name, value in (("EG_MOTION_WINDOW", 34), ("EG_MOTION_ROW_FLOATS", 384), ("EG_MOTION_MAX_POSE_DIM", 128), ("EG_MOTION_RUN_FRAMES", 136),
                        ("EG_TAKE_MAX_DRAWS", 64)):
        assert f"#define {name} {value}\n" in header and getattr(L, name) == value


# ---- the Python layers ---------------------------------------------------------------------------------------------------------------
def test_python_refusals_before_any_launch():
    ae = MotionAE(126, 32).eval()
    trk = torch.zeros(3, 2, 110, 126)
    for fn in (MF.window_rows, MF.window_features):
        who = fn.__name__
        with pytest.raises(RuntimeError, match=f"{who}: track must be a CUDA tensor"):
            fn(ae, trk, FRAMES)
        with pytest.raises(L.EgError, match=f"{who}: the feature net is not in eval mode"):
            fn(MotionAE(126, 32).train(), trk, FRAMES)
        with pytest.raises(L.EgError, match=f"{who}: track has 125 pose columns, the feature net takes pose_dim=126"):
            fn(ae, trk[..., :125], FRAMES)
        with pytest.raises(L.EgError, match=f"{who}: the feature net must be a model.motion_ae.MotionAE"):
            fn(H.MLP_Reconstruct(pose_dim=126).eval(), trk, FRAMES)
        with pytest.raises(L.EgError, match=rf"{who}: frames\[1\]=33 < window=34"):
            fn(ae, trk, [34, 33, 103])
        with pytest.raises(L.EgError, match=rf"{who}: frames\[2\]=111 > Tmax=110"):
            fn(ae, trk, [34, 35, 111])
        with pytest.raises(ValueError, match=f"{who}: frames has 2 entries for 3 recordings"):
            fn(ae, trk, [34, 35])
        with pytest.raises(L.EgError, match=f"{who}: stride=0"):
            fn(ae, trk, FRAMES, stride=0)
        with pytest.raises(ValueError, match=f"{who}: track must be"):
            fn(ae, trk[0, 0, 0], FRAMES)
        with pytest.raises(L.EgError, match=rf"{who}: pose_dim=130 \(1\.\.128\)"):
            fn(MotionAE(130, 32).eval(), torch.zeros(1, 40, 130))
    with pytest.raises(L.EgError, match=r"window_rows: clips \[0, 15\) \(need 0 <= c0 < c1 <= N=14\)"):
        MF.window_rows(ae, trk, FRAMES, clips=(0, 15))             # 1 + 2 + 4 windows, two takes
    with pytest.raises(L.EgError, match="window_features: chunk_clips=0"):
        MF.window_features(ae, trk, FRAMES, chunk_clips=0)


def test_take_diversity_refusals():
    trk = torch.zeros(2, 2, 40, 126)
    with pytest.raises(L.EgError, match="take_diversity: the MotionAE's latent_dim=30"):
        takes.take_diversity(MotionAE(126, 30).eval(), trk)
    with pytest.raises(RuntimeError, match="window_features: track must be a CUDA tensor"):
        takes.take_diversity(MotionAE(126, 32).eval(), trk, stride=17)
    with pytest.raises(L.EgError, match="take_diversity: stride= and tail= are the window arguments of a MotionAE"):
        takes.take_diversity(H.MLP_Reconstruct(pose_dim=126).eval(), trk, stride=17)
    with pytest.raises(L.EgError, match="take_diversity: track must be"):
        takes.take_diversity(MotionAE(126, 32).eval(), trk[:, 0])


def test_harness_refuses_a_motion_ae_before_anything_runs():
    class NoCall:                                                   # a VAE that must not be reached
        def sample(self, *a, **k):
            raise AssertionError("vae.sample was called")
    beat = build_mirror("spatial", 60, 282, 10, 10, seed=31).eval()          # on the CPU: its engine refuses, so reaching it fails the matches
    audio, text, seed = torch.zeros(2, 3 * 64000), torch.zeros(2, 3, 60, dtype=torch.long), torch.zeros(2, 10, 282)
    one = torch.eye(8)[[1, 5]]
    with pytest.raises(L.EgError, match="synthesize: diversity=: the MotionAE takes pose_dim=126, the generator's poses have 282 columns"):
        H.synthesize((beat, NoCall()), audio, text, seed, one, draws=2, diversity=MotionAE(126, 32).eval())
    with pytest.raises(L.EgError, match="synthesize_takes: diversity=: the MotionAE takes pose_dim=126"):
        H.synthesize_takes((beat, NoCall()), audio, text, seed, one, draws=2, diversity=MotionAE(126, 32).eval())
    ted = build_mirror("spatial", 34, 126, 4, 4, seed=3).eval()
    audio, seed = torch.zeros(2, 3 * 32000), torch.zeros(2, 4, 126)
    with pytest.raises(L.EgError, match="synthesize: diversity=: the MotionAE is not in eval mode"):
        H.synthesize((ted, NoCall()), audio, text, seed, one, draws=2, diversity=MotionAE(126, 32).train())
    with pytest.raises(L.EgError, match="synthesize: diversity=: the MotionAE's latent_dim=30"):
        H.synthesize((ted, NoCall()), audio, text, seed, one, draws=2, diversity=MotionAE(126, 30).eval())
    with pytest.raises(L.EgError, match="synthesize: diversity_stride=0"):
        H.synthesize((ted, NoCall()), audio, text, seed, one, draws=2, diversity=MotionAE(126, 32).eval(), diversity_stride=0)
    with pytest.raises(L.EgError, match="diversity= needs draws >= 2"):
        H.synthesize((ted, NoCall()), audio, text, seed, one, diversity=MotionAE(126, 32).eval())
    short = build_mirror("spatial", 30, 126, 4, 4, seed=3).eval()   # a generator whose one-window recording is shorter than a MotionAE window
    with pytest.raises(L.EgError, match="synthesize: diversity=: a recording of one generator window has 30 poses < window=34"):
        H.synthesize((short, NoCall()), audio, text, seed, one, draws=2, diversity=MotionAE(126, 32).eval())
    # everything checked: the call goes on to the generator, which refuses the CPU
    with pytest.raises(L.EgError, match="runs only on a GPU"):
        H.synthesize((ted, NoCall()), audio, text, seed, one, draws=2, diversity=MotionAE(126, 32).eval())
    assert "diversity_stride" in H.synthesize.__doc__


def test_evaluator_push_tracks_refuses_unpaired_tracks_and_keeps_the_error_lists():
    from types import SimpleNamespace
    from emotiongestures_amd.model.embedding_space_evaluator import EmbeddingSpaceEvaluator
    args = SimpleNamespace(n_pre_poses=4, n_poses=34, pose_dim=126, wordembed_dim=300)
    ev = EmbeddingSpaceEvaluator(args, {"pose_dim": 126, "latent_dim": 32, "motion_ae": MotionAE(126, 32).state_dict()}, None, "cpu")
    with pytest.raises(ValueError, match="push_tracks: generated track"):
        ev.push_tracks(torch.zeros(1, 68, 126), torch.zeros(1, 69, 126))
    with pytest.raises(RuntimeError, match="window_features: track must be a CUDA tensor"):
        ev.push_tracks(torch.zeros(1, 68, 126), torch.zeros(1, 68, 126))
    assert ev.get_no_of_samples() == 0 and not ev.recon_err_diff and "stay untouched" in EmbeddingSpaceEvaluator.push_tracks.__doc__
