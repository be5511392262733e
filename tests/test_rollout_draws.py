"""Diverse roll-out, CPU side: the definition restated over the CPU oracle against the reference golden of the plain roll-out, the
C ABI's argument checks and workspace size, and the Python surface's refusals.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rollout_draws_np as RD
import rollout_np as R
from conftest import ROOT, build_mirror, clip_rel_l2
from emotiongestures_amd import _lib as L
from oracle import emogest_oracle as O

TOL = 2e-5                      # tests/test_rollout.py: the bar the oracle's roll-out meets against the reference
POSE_TOL_LOOSEST = 1e-3         # tests/test_gpu_generator.py POSE_TOL["bf16x3"]: the loosest bar any roll-out test builds on
NEW_SYMBOLS = ("eg_generator_forward_rollout_draws", "eg_generator_rollout_draws_workspace_bytes")
FN = "eg_generator_forward_rollout_draws"


# ---- the definition, on the CPU oracle -------------------------------------------------------------------------------------
def test_oracle_rollout_draws_matches_reference_golden_and_sees_a_wrong_draw():
    """R = 2 on the spatial fixture (its rows are independent): draw 0 is the fixture's own sampled map and must reproduce the golden
    windows and track within the fixture's bars (the oracle's bar TOL through free_running_tol with the stored gains); draw 1 is a hash-generated
    map and must differ from draw 0, in every window of every recording, by more than 100 x the loosest bar any test applies to this fixture
    (the bf16x3 free-running bar of the last window, tests/test_gpu_rollout_draws.py), so a wrong draw index cannot hide."""
    name = "rollout_ted_spatial"
    z, m, inp, sampled = R.load_case(name)
    assert sampled is not None
    U, W = m["U"], m["W"]
    model = build_mirror(R.CASES[name], m["frames"], m["pose_dim"], m["prior"], m["chunk"], m["n_words"], m["seed"], m["spec_len"])
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    cfg = O.GenCfg(frames=m["frames"], pose_dim=m["pose_dim"], prior_frames=m["prior"], chunk=m["chunk"], variant=R.CASES[name])
    both = torch.stack([sampled, RD.hash_sampled(sampled.shape, m["seed"])], 1)           # [U, 2, W, F, d]
    with torch.no_grad():
        out = RD.rollout_draws(lambda s, t, p, e: O.generator_forward(sd, cfg, s, t, p, e), torch.from_numpy(inp["spec"]),
                               torch.from_numpy(inp["text"]), torch.from_numpy(inp["seed_pose"]), both)
    assert out["windows"].shape == (U, 2, W, m["frames"], m["pose_dim"]) and out["track"].shape == (U, 2) + z["track"].shape[1:]
    hg, wg = float(z["handoff_gain"]), float(z["window_gain"])
    loosest = R.free_running_tol(POSE_TOL_LOOSEST, wg, hg, W - 1)
    for w in range(W):
        e, tol = clip_rel_l2(out["windows"][:, 0, w], z["windows"][:, w]), R.free_running_tol(TOL, wg, hg, w)
        print(f"draw 0 window {w}: per-clip rel-L2 {e:.2e} (tolerance {tol:.2e})")
        assert e < tol, (w, e, tol)
    e = clip_rel_l2(out["track"][:, 0], z["track"])
    print(f"draw 0 track: per-clip rel-L2 {e:.2e}")
    assert e < R.free_running_tol(TOL, wg, hg, W - 1)
    assert np.abs(out["emotion_prediction"] - z["emotion_prediction"]).max() < TOL * max(1.0, np.abs(z["emotion_prediction"]).max())
    for r in range(2):
        assert np.array_equal(out["track"][:, r], R.stitch(out["windows"][:, r], m["prior"]))
    # per clip, so that no recording's draw 1 may coincide with its draw 0
    apart = min(clip_rel_l2(out["windows"][u:u + 1, 1, w], out["windows"][u:u + 1, 0, w]) for u in range(U) for w in range(W))
    print(f"draw 1 against draw 0: smallest per-clip rel-L2 {apart:.2e} (loosest bar {loosest:.2e})")
    assert apart > 100 * loosest


def test_replicate_puts_recording_u_draw_r_at_row_uR_plus_r():
    U, Rd, W = 3, 2, 2
    spec = torch.arange(U * W, dtype=torch.float32).reshape(U, W, 1, 1)
    sampled = torch.arange(U * Rd * W, dtype=torch.float32).reshape(U, Rd, W, 1, 1)
    s, t, p, e = RD.replicate(spec, torch.zeros(U, W, 1, dtype=torch.int64), torch.arange(U, dtype=torch.float32).reshape(U, 1, 1), sampled)
    assert s.shape == (U * Rd, W, 1, 1) and e.shape == (U * Rd, W, 1, 1) and t.shape == (U * Rd, W, 1)
    for u in range(U):
        for r in range(Rd):
            assert torch.equal(s[u * Rd + r], spec[u]) and torch.equal(e[u * Rd + r], sampled[u, r]) and float(p[u * Rd + r]) == u


# ---- C ABI / binding -------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header, re.S)
        assert decl, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
        assert len(decl.group(1).split(",")) == len(L.SIGNATURES[name][1]), name


def _generator(**over):
    lib = L.load()
    cfg = L.EgGeneratorConfig()
    L.check(lib.eg_generator_default_config(C.byref(cfg)))
    for k, v in over.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    L.check(lib.eg_generator_create(C.byref(cfg), C.byref(h)))
    return lib, h


def test_workspace_equals_the_rollouts_at_one_draw_grows_with_draws_and_is_zero_for_refused_counts():
    lib, h = _generator()
    try:
        ws = lambda u, w, r: lib.eg_generator_rollout_draws_workspace_bytes(h, u, w, r)
        for u, w in ((1, 1), (2, 3), (5, 2), (1, 7)):
            assert ws(u, w, 1) == lib.eg_generator_rollout_workspace_bytes(h, u, w) > 0
            assert ws(u, w, 1) < ws(u, w, 2) < ws(u, w, 3) < ws(u, w, 8)
        assert ws(1, 1, 2) < ws(2, 1, 2) and ws(1, 1, 2) < ws(1, 2, 2)
        # the tower side is carved once per clip: R draws cost less than R times the recordings
        assert ws(2, 3, 4) < lib.eg_generator_rollout_workspace_bytes(h, 8, 3)
        for u, w, r in ((0, 3, 2), (2, 0, 2), (2, 3, 0), (-1, 1, 1), (2, -3, 2), (2, 3, -1), (1 << 10, 1 << 10, 2), (1, 1, (1 << 20) + 1),
                        (1 << 11, 1 << 10, 1)):
            assert ws(u, w, r) == 0, (u, w, r)
        assert lib.eg_generator_rollout_draws_workspace_bytes(None, 2, 3, 2) == 0
    finally:
        lib.eg_generator_destroy(h)


def test_c_abi_refuses_bad_arguments_by_name():
    """Every refusal comes before the first launch: the buffers are never read and eg_launch_count does not move."""
    lib, h = _generator()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data - buf.ctypes.data % 16 + 16)
    odd = C.c_void_p(p.value + 4)
    err = lambda: lib.eg_last_error().decode()
    n0 = lib.eg_launch_count()
    try:
        def call(U=2, W=2, R=2, ws_bytes=1 << 50, g=h, arena=p, spec=p, text=p, seed=p, sampled=p, track=p, txt=None, ws=p):
            return lib.eg_generator_forward_rollout_draws(g, arena, U, W, R, spec, text, seed, sampled, None, track, None, None, None, None,
                                                          txt, ws, ws_bytes, None)
        for kw in (dict(g=None), dict(arena=None), dict(spec=None), dict(seed=None), dict(sampled=None), dict(track=None), dict(ws=None)):
            assert call(**kw) != 0 and FN + ": null pointer" in err(), kw
        assert call(U=0) != 0 and FN in err() and "utterances=0" in err()
        assert call(W=0) != 0 and FN in err() and "windows=0" in err()
        assert call(W=-3) != 0 and "windows=-3" in err()
        assert call(R=0) != 0 and FN in err() and "draws=0" in err()
        assert call(R=-2) != 0 and "draws=-2" in err()
        assert call(U=1 << 10, W=1 << 10, R=2) != 0 and FN in err() and "utterances*windows*draws" in err() and "2^20" in err()
        assert call(U=1, W=1, R=(1 << 20) + 1) != 0 and "utterances*windows*draws" in err()
        assert call(text=None, txt=p) != 0 and FN in err() and "text_embedding wanted without text" in err()
        assert call(ws_bytes=1024) != 0 and FN in err() and "workspace 1024 <" in err()
        assert call(R=1, ws_bytes=1024) != 0 and FN in err() and "workspace 1024 <" in err()
        for kw in (dict(ws=odd), dict(arena=odd), dict(spec=odd), dict(sampled=odd)):
            assert call(**kw) != 0 and FN in err() and "16-byte alignment" in err(), kw
    finally:
        lib.eg_generator_destroy(h)
    lib9, h9 = _generator(n_layers=9)
    try:
        assert lib9.eg_generator_forward_rollout_draws(h9, p, 2, 2, 2, p, p, p, p, None, p, None, None, None, None, None, p, 1 << 50, None) != 0
        assert FN in err() and "n_layers=9 > 8" in err()
        assert lib9.eg_generator_rollout_draws_workspace_bytes(h9, 2, 2, 2) == 0
    finally:
        lib9.eg_generator_destroy(h9)
    assert lib.eg_launch_count() == n0


# ---- Python surface ---------------------------------------------------------------------------------------------------
def _engine():
    from emotiongestures_amd.engine import GeneratorEngine
    return GeneratorEngine()


def _args(U=2, W=3, Rd=4):
    return dict(spec=torch.zeros(U, W, 128, 124), text=torch.zeros(U, W, 60, dtype=torch.int64), seed_pose=torch.zeros(U, 4, 126),
                sampled=torch.zeros(U, Rd, W, 34, 512), alpha=torch.zeros(4))


@pytest.mark.parametrize("arg,bad,needle", [
    ("sampled", None, "sampled: required, shape (U,R,W,F,d_model)"),
    ("sampled", torch.zeros(2, 3, 34, 512), "!= (U,R,W,F,d_model)"),
    ("sampled", torch.zeros(2, 4, 2, 34, 512), "!= (U,R,W,F,d_model) = (2,4,3,34,512)"),
    ("sampled", torch.zeros(3, 4, 3, 34, 512), "!= (U,R,W,F,d_model) = (2,4,3,34,512)"),
    ("sampled", torch.zeros(2, 4, 3, 34, 256), "!= (U,R,W,F,d_model) = (2,4,3,34,512)"),
    ("sampled", torch.zeros(2, 0, 3, 34, 512), "draws R=0"),
    ("spec", torch.zeros(2, 3, 128, 100), "spec shape"),
    ("spec", torch.zeros(2, 0, 128, 124), "windows W=0"),
    ("spec", torch.zeros(0, 3, 128, 124), "utterances U=0"),
    ("text", torch.zeros(2, 2, 60, dtype=torch.int64), "text shape"),
    ("seed_pose", torch.zeros(2, 5, 126), "seed_pose shape"),
    ("seed_pose", torch.zeros(8, 4, 126), "seed_pose shape"),          # one seed per recording, not per (recording, draw)
    ("alpha", torch.zeros(5), "alpha shape"),
])
def test_forward_rollout_draws_refuses_wrong_shapes_by_name(arg, bad, needle):
    a = _args()
    a[arg] = bad
    with pytest.raises(L.EgError, match=re.escape(needle)):
        _engine().forward_rollout_draws(a["spec"], a["text"], a["seed_pose"], a["sampled"], alpha=a["alpha"])


def test_forward_rollout_draws_needs_loaded_weights():
    a = _args()
    with pytest.raises(L.EgError, match="forward_rollout_draws before load_weights"):
        _engine().forward_rollout_draws(a["spec"], a["text"], a["seed_pose"], a["sampled"])


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_synthesize_draws_is_eval_only_and_checks_its_arguments(variant):
    model = build_mirror(variant, 34, 126, 4, 4, seed=1)
    a = _args()
    model.train()
    with pytest.raises(NotImplementedError, match="eval"):
        model.synthesize(a["spec"], a["text"], a["seed_pose"], a["sampled"], draws=4)
    model.eval()
    with pytest.raises(L.EgError, match=re.escape("(U,R,W,F,d_model) with R=3")):           # shape[1] != draws
        model.synthesize(a["spec"], a["text"], a["seed_pose"], a["sampled"], draws=3)
    with pytest.raises(L.EgError, match=re.escape("(U,R,W,F,d_model) with R=4")):
        model.synthesize(a["spec"], a["text"], a["seed_pose"], None, draws=4)
    with pytest.raises(L.EgError, match="draws=0"):
        model.synthesize(a["spec"], a["text"], a["seed_pose"], a["sampled"], draws=0)
    with pytest.raises(L.EgError, match="draws= with windows_per= is not supported.*rectangular"):
        model.synthesize(a["spec"], a["text"], a["seed_pose"], a["sampled"], draws=4, windows_per=[3, 3])
    with pytest.raises(L.EgError, match="GPU"):             # a CPU module is refused, not computed some other way
        model.synthesize(a["spec"], a["text"], a["seed_pose"], a["sampled"], draws=4)


def test_harness_synthesize_draws_refusals():
    from emotiongestures_amd import harness as H
    model = build_mirror("spatial", 34, 126, 4, 4, seed=1)
    audio, text, seed = torch.zeros(2, 100000), torch.zeros(2, 2, 60, dtype=torch.int64), torch.zeros(2, 4, 126)
    model.train()
    with pytest.raises(NotImplementedError, match="eval"):
        H.synthesize((model, None), audio, text, seed, draws=2)
    model.eval()
    with pytest.raises(L.EgError, match="draws= needs a VAE"):
        H.synthesize((model, None), audio, text, seed, draws=2)
    with pytest.raises(L.EgError, match="draws= with lengths= is not supported.*rectangular"):
        H.synthesize((model, object()), audio, text, seed, draws=2, lengths=[100000, 90000])
    with pytest.raises(L.EgError, match="draws=0"):
        H.synthesize((model, object()), audio, text, seed, draws=0)


def test_stream_refuses_draws_by_name():
    from emotiongestures_amd import harness as H
    model = build_mirror("spatial", 34, 126, 4, 4, seed=1).eval()
    with pytest.raises(L.EgError, match="GestureStream: draws= is not supported.*rectangular synthesize"):
        H.open_stream((model, None), 2, torch.zeros(2, 4, 126), draws=3)
    with pytest.raises(L.EgError, match="GestureStream: draws= is not supported"):
        model.open_stream(2, torch.zeros(2, 4, 126), draws=3)
