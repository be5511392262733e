"""Long-form roll-out, CPU side: the loop restated over the CPU oracle against goldens made from the reference's own Transformer, the
stitch arithmetic, the C ABI's argument checks and the Python surface's refusals.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rollout_np as R
from rollout_np import CASES, load_case
from conftest import ROOT, build_mirror, clip_rel_l2
from emotiongestures_amd import _lib as L
from oracle import emogest_oracle as O

TOL = 2e-5                      # tests/test_oracle_golden.py: the bar the oracle's pose meets against the reference
POSE_TOL_LOOSEST = 1e-3         # tests/test_gpu_generator.py POSE_TOL["bf16x3"]: the loosest bar any roll-out test builds on


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_rollout_matches_reference_golden(name):
    z, m, inp, sampled = load_case(name)
    model = build_mirror(CASES[name], m["frames"], m["pose_dim"], m["prior"], m["chunk"], m["n_words"], m["seed"], m["spec_len"])
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    cfg = O.GenCfg(frames=m["frames"], pose_dim=m["pose_dim"], prior_frames=m["prior"], chunk=m["chunk"], variant=CASES[name])
    with torch.no_grad():
        out = R.rollout(lambda s, t, p, e: O.generator_forward(sd, cfg, s, t, p, e), torch.from_numpy(inp["spec"]), torch.from_numpy(inp["text"]),
                        torch.from_numpy(inp["seed_pose"]), sampled)
    assert out["windows"].shape == z["windows"].shape == (m["U"], m["W"], m["frames"], m["pose_dim"])
    for w in range(m["W"]):
        e = clip_rel_l2(out["windows"][:, w], z["windows"][:, w])
        print(f"{name} window {w}: per-clip rel-L2 {e:.2e}")
        assert e < TOL, (w, e)
    assert out["track"].shape == z["track"].shape == (m["U"], m["W"] * (m["frames"] - m["prior"]) + m["prior"], m["pose_dim"])
    assert clip_rel_l2(out["track"], z["track"]) < TOL
    assert np.abs(out["emotion_prediction"] - z["emotion_prediction"]).max() < TOL * max(1.0, np.abs(z["emotion_prediction"]).max())
    assert np.array_equal(z["alpha"], R.default_alpha(m["prior"]))
    assert np.array_equal(R.stitch(z["windows"], m["prior"]), z["track"])        # the stored track is the stitch of the stored windows


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_can_see_a_wrong_handoff(name):
    """For every window w >= 1 and every utterance, the reference's pose_w seeded with seed_pose instead of the previous window's tail differs
    from the right one by at least 100 x the loosest tolerance any test applies to this fixture (the bf16x3 free-running bar of the last window)."""
    z, m, _inp, _s = load_case(name)
    hg, wg = float(z["handoff_gain"]), float(z["window_gain"])
    loosest = R.free_running_tol(POSE_TOL_LOOSEST, wg, hg, m["W"] - 1)
    sens = z["handoff_sensitivity"]
    assert sens.shape == (m["W"] - 1, m["U"])
    print(f"{name}: handoff_gain {hg:.4f} window_gain {wg:.4f} loosest tol {loosest:.3e} min sensitivity {sens.min():.3e}")
    assert hg > 0 and wg > 0
    assert sens.min() >= 100 * loosest


def test_stitch_is_exact_on_small_integers():
    U, W, F, D, P = 2, 3, 7, 3, 2
    H = F - P
    rng = np.random.RandomState(0)
    win = rng.randint(-8, 9, size=(U, W, F, D)).astype(np.float32)
    alpha = np.asarray([0.25, 0.75], np.float32)            # dyadic: every product and sum below is exact in fp32
    track = R.stitch(win, P, alpha)
    assert track.shape == (U, W * H + P, D)
    assert np.array_equal(track[:, :H], win[:, 0, :H])          # rows [H, F) of window 0 are then blended over by window 1
    assert np.array_equal(R.stitch(win[:, :1], P, alpha), win[:, 0])
    for w in range(1, W):
        for j in range(F if w == W - 1 else H):             # a window's last P rows are blended over by the next one
            want = win[:, w, j] if j >= P else (1 - alpha[j]) * win[:, w - 1, H + j] + alpha[j] * win[:, w, j]
            assert np.array_equal(track[:, w * H + j], want), (w, j)
    assert np.allclose(R.default_alpha(4), [0.2, 0.4, 0.6, 0.8])


def test_rollout_hands_over_the_raw_tail_not_the_blend():
    """The loop's prior for window w is pose_{w-1}[:, H:F] as the generator returned it."""
    calls = []

    def gen(spec, text, prior, sampled):
        calls.append(prior.clone())
        pose = torch.arange(2 * 6 * 3, dtype=torch.float32).reshape(2, 6, 3) + 100 * len(calls)
        return pose, None, None, torch.zeros(2, 8), None
    out = R.rollout(gen, torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 2, dtype=torch.int64), torch.full((2, 2, 3), -1.0))
    assert torch.equal(calls[0], torch.full((2, 2, 3), -1.0))
    for w in (1, 2):
        assert np.array_equal(calls[w].numpy(), out["windows"][:, w - 1, 4:])
    assert out["track"].shape == (2, 3 * 4 + 2, 3) and out["emotion_prediction"].shape == (2, 3, 8)


# ---- C ABI / binding -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("eg_generator_forward_rollout", "eg_generator_rollout_workspace_bytes", "eg_window_gather")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header, re.S)
        assert decl, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
        assert len(decl.group(1).split(",")) == len(L.SIGNATURES[name][1]), name


def _generator():
    lib = L.load()
    cfg = L.EgGeneratorConfig()
    L.check(lib.eg_generator_default_config(C.byref(cfg)))
    h = C.c_void_p()
    L.check(lib.eg_generator_create(C.byref(cfg), C.byref(h)))
    return lib, h


def test_rollout_workspace_grows_with_utterances_and_windows():
    lib, h = _generator()
    try:
        ws = lambda u, w: lib.eg_generator_rollout_workspace_bytes(h, u, w)
        assert ws(1, 1) > lib.eg_generator_workspace_bytes(h, 1)            # the kept K|V on top of a one-clip forward
        assert ws(1, 1) < ws(2, 1) < ws(4, 1)
        assert ws(1, 1) < ws(1, 2) < ws(1, 4)
        assert ws(0, 3) == 0 and ws(2, 0) == 0 and ws(-1, 1) == 0
    finally:
        lib.eg_generator_destroy(h)


def test_c_abi_refuses_bad_counts_by_name():
    lib, h = _generator()
    buf = np.zeros(64, np.float32)                  # never read: the argument checks come before the first launch
    p = C.c_void_p(buf.ctypes.data)
    err = lambda: lib.eg_last_error().decode()
    try:
        def call(U, W, ws_bytes=1 << 40, spec=p):
            return lib.eg_generator_forward_rollout(h, p, U, W, spec, p, p, None, None, p, None, None, None, None, None, p, ws_bytes, None)
        assert call(2, 0) != 0 and "windows=0" in err()
        assert call(0, 2) != 0 and "utterances=0" in err()
        assert call(2, -3) != 0 and "windows=-3" in err()
        assert call(2, 2, ws_bytes=1024) != 0 and "workspace" in err()
        assert call(2, 2, spec=None) != 0 and "null pointer" in err()
        # eg_window_gather: the last window must start inside the track
        assert lib.eg_window_gather(p, 1, 64, 3, 32, 48, p, None) != 0 and "windows=3" in err()
        assert lib.eg_window_gather(p, 1, 64, 0, 32, 48, p, None) != 0 and "windows=0" in err()
        assert lib.eg_window_gather(p, 1, 64, 1, 0, 48, p, None) != 0 and "hop_samples=0" in err()
    finally:
        lib.eg_generator_destroy(h)


# ---- Python surface ---------------------------------------------------------------------------------------------------
def _engine():
    from emotiongestures_amd.engine import GeneratorEngine
    return GeneratorEngine()


def _args(U=2, W=3):
    return dict(spec=torch.zeros(U, W, 128, 124), text=torch.zeros(U, W, 60, dtype=torch.int64), seed_pose=torch.zeros(U, 4, 126),
                sampled=torch.zeros(U, W, 34, 512), alpha=torch.zeros(4))


@pytest.mark.parametrize("arg,bad,needle", [
    ("spec", torch.zeros(2, 3, 128, 100), "spec shape"),
    ("spec", torch.zeros(6, 128, 124), "spec shape"),
    ("spec", torch.zeros(2, 0, 128, 124), "windows W=0"),
    ("spec", torch.zeros(0, 3, 128, 124), "utterances U=0"),
    ("text", torch.zeros(2, 2, 60, dtype=torch.int64), "text shape"),
    ("seed_pose", torch.zeros(2, 5, 126), "seed_pose shape"),
    ("seed_pose", torch.zeros(3, 4, 126), "seed_pose shape"),
    ("sampled", torch.zeros(2, 3, 34, 256), "sampled shape"),
    ("alpha", torch.zeros(5), "alpha shape"),
])
def test_forward_rollout_refuses_wrong_shapes_by_name(arg, bad, needle):
    a = _args()
    a[arg] = bad
    with pytest.raises(L.EgError, match=re.escape(needle)):
        _engine().forward_rollout(a["spec"], a["text"], a["seed_pose"], a["sampled"], alpha=a["alpha"])


def test_forward_rollout_needs_loaded_weights():
    a = _args()
    with pytest.raises(L.EgError, match="before load_weights"):
        _engine().forward_rollout(a["spec"], a["text"], a["seed_pose"])


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_synthesize_is_eval_only(variant):
    model = build_mirror(variant, 34, 126, 4, 4, seed=1)
    a = _args()
    model.train()
    with pytest.raises(NotImplementedError, match="eval"):
        model.synthesize(a["spec"], a["text"], a["seed_pose"])
    model.eval()
    with pytest.raises(L.EgError, match="GPU"):             # a CPU module is refused, not computed some other way
        model.synthesize(a["spec"], a["text"], a["seed_pose"])


def test_harness_synthesize_is_eval_only():
    from emotiongestures_amd import harness as H
    model = build_mirror("spatial", 34, 126, 4, 4, seed=1).train()
    with pytest.raises(NotImplementedError, match="eval"):
        H.synthesize((model, None), torch.zeros(2, 100000), torch.zeros(2, 2, 60, dtype=torch.int64), torch.zeros(2, 4, 126))
