"""Ragged roll-out, CPU side: the plan (host function of the library) against its numpy restatement, the loop over steps restated over the
CPU oracle against the reference goldens of the rectangular roll-out, the C ABI's argument checks and the Python surface's refusals.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rollout_np as R
import rollout_ragged_np as RR
from rollout_np import CASES, load_case
from conftest import ROOT, build_mirror, clip_rel_l2
from emotiongestures_amd import _lib as L
from oracle import emogest_oracle as O

TOL = 2e-5                      # tests/test_rollout.py: the bar the oracle's rectangular loop meets against the reference
POSE_TOL_LOOSEST = 1e-3         # tests/test_gpu_generator.py POSE_TOL["bf16x3"]: the loosest bar any roll-out test builds on
VECTORS = [(4, 2), (1, 4), (3, 4)]          # the fixtures hold U = 2 recordings of W = 4 windows


# ---- the plan ---------------------------------------------------------------------------------------------------------------
PLAN_VECTORS = [(4, 2), (1, 4), (3, 4), (2, 2, 2), (1,), (7,), (1, 1, 1), (2, 5, 2, 1, 5), (1, 30, 2, 2, 1, 3), (3, 1, 4, 1, 5, 9, 2, 6)]


@pytest.mark.parametrize("wp", PLAN_VECTORS)
def test_plan_is_the_stable_sort_and_a_permutation(wp):
    from emotiongestures_amd.engine import ragged_plan
    p, want = ragged_plan(wp), RR.plan(wp)
    U, N, Wmax = len(wp), sum(wp), max(wp)
    order = [int(v) for v in p["order"]]
    assert order == sorted(range(U), key=lambda u: (-wp[u], u))                     # longer first, ties by index
    assert [int(p["inverse"][u]) for u in order] == list(range(U))
    sb = [int(v) for v in p["step_batch"]]
    assert len(sb) == Wmax and sum(sb) == N and sb[0] == U
    assert all(a >= b for a, b in zip(sb, sb[1:])) and sb == [sum(w > s for w in wp) for s in range(Wmax)]
    assert sorted(int(v) for v in p["slot_row"]) == list(range(N))                  # a permutation of the packed rows
    off = np.concatenate([[0], np.cumsum(wp)[:-1]])
    assert np.array_equal(p["offsets"], off)
    slot = 0
    for s in range(Wmax):
        for r in range(sb[s]):
            assert int(p["slot_row"][slot]) == off[order[r]] + s, (s, r)
            slot += 1
    # the device table: slot_row | order | W by rank
    assert p["table"].shape == (N + 2 * U,) and p["table"].dtype == np.int32
    assert np.array_equal(p["table"][N: N + U], p["order"]) and [int(v) for v in p["table"][N + U:]] == [wp[u] for u in order]
    for k in ("order", "inverse", "step_batch", "offsets", "slot_row"):
        assert np.array_equal(np.asarray(p[k], np.int64), want[k]), k


def test_plan_refuses_bad_counts_by_name():
    from emotiongestures_amd.engine import ragged_plan
    lib = L.load()
    with pytest.raises(L.EgError, match=re.escape("windows_per[1]=0")):
        ragged_plan((2, 0, 3))
    with pytest.raises(L.EgError, match=re.escape("windows_per[0]=-2")):
        ragged_plan((-2,))
    with pytest.raises(L.EgError, match="utterances=0"):
        ragged_plan(())
    big = np.full(3, 1 << 19, np.int32)
    assert lib.eg_rollout_ragged_plan(C.c_void_p(big.ctypes.data), 3, None, None, None, None) != 0
    assert "total windows" in lib.eg_last_error().decode()
    assert lib.eg_rollout_ragged_plan_ints(3, 2) == 0 and lib.eg_rollout_ragged_plan_ints(0, 5) == 0
    assert lib.eg_rollout_ragged_plan_ints(3, (1 << 20) + 1) == 0 and lib.eg_rollout_ragged_plan_ints(3, 7) == 7 + 6


# ---- the definition against the reference goldens ------------------------------------------------------------------------------------
def _oracle(name, m):
    model = build_mirror(CASES[name], m["frames"], m["pose_dim"], m["prior"], m["chunk"], m["n_words"], m["seed"], m["spec_len"])
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    cfg = O.GenCfg(frames=m["frames"], pose_dim=m["pose_dim"], prior_frames=m["prior"], chunk=m["chunk"], variant=CASES[name])
    return lambda s, t, p, e: O.generator_forward(sd, cfg, s, t, p, e)


@pytest.mark.parametrize("wp", VECTORS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_ragged_rollout_matches_reference_golden(name, wp):
    """The goldens of the rectangular roll-out hold every window of both recordings; a ragged roll-out over the oracle must reproduce recording
    u's first W_u windows (steps with one active recording included), and its track the stitch of those."""
    z, m, inp, sampled = load_case(name)
    assert m["U"] == len(wp) and max(wp) <= m["W"]
    gen = _oracle(name, m)
    with torch.no_grad():
        out = RR.rollout_ragged(gen, torch.from_numpy(RR.pack(inp["spec"], wp)), torch.from_numpy(RR.pack(inp["text"], wp)),
                                torch.from_numpy(inp["seed_pose"]), wp, None if sampled is None else torch.from_numpy(RR.pack(sampled.numpy(), wp)))
    H, P = m["frames"] - m["prior"], m["prior"]
    off = out["window_offsets"]
    assert out["windows"].shape == (sum(wp), m["frames"], m["pose_dim"]) and out["track"].shape == (len(wp), max(wp) * H + P, m["pose_dim"])
    for u, W_u in enumerate(wp):
        for w in range(W_u):
            e = clip_rel_l2(out["windows"][off[u] + w][None], z["windows"][u, w][None])
            print(f"{name} {wp} recording {u} window {w}: rel-L2 {e:.2e}")
            assert e < TOL, (u, w, e)
        want = R.stitch(z["windows"][u:u + 1, :W_u], P)
        T = W_u * H + P
        assert out["track_frames"][u] == T and want.shape[1] == T
        assert clip_rel_l2(out["track"][u:u + 1, :T], want) < TOL
        assert not out["track"][u, T:].any()
        assert np.abs(out["emotion_prediction"][off[u]: off[u] + W_u] - z["emotion_prediction"][u, :W_u]).max() < \
            TOL * max(1.0, np.abs(z["emotion_prediction"]).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_can_see_a_missing_unpermute(name):
    """(1, 4) is worked on in the order (1, 0): results left in working order would put recording 1's windows where recording 0's belong.  The
    two recordings of the fixture differ, window by window, by at least 100 x the loosest tolerance any test applies to it."""
    z, m, _inp, _s = load_case(name)
    loosest = R.free_running_tol(POSE_TOL_LOOSEST, float(z["window_gain"]), float(z["handoff_gain"]), m["W"] - 1)
    for w in range(m["W"]):
        d = min(clip_rel_l2(z["windows"][0:1, w], z["windows"][1:2, w]), clip_rel_l2(z["windows"][1:2, w], z["windows"][0:1, w]))
        print(f"{name} window {w}: recordings differ by rel-L2 {d:.3e} (loosest tolerance {loosest:.3e})")
        assert d >= 100 * loosest, (w, d)


def test_ragged_loop_runs_only_the_active_recordings_in_working_order():
    calls = []

    def gen(spec, text, prior, sampled):
        calls.append((spec[:, 0, 0].clone(), prior.clone()))
        B = spec.shape[0]
        pose = spec[:, 0, 0][:, None, None] + torch.arange(6 * 3, dtype=torch.float32).reshape(1, 6, 3) / 100
        return pose, None, None, torch.zeros(B, 8), None
    wp = (1, 3, 2)
    N = sum(wp)
    spec = torch.arange(N, dtype=torch.float32)[:, None, None].expand(N, 4, 5).contiguous()        # a clip is marked with its packed row
    seed = torch.stack([torch.full((2, 3), -1.0 - u) for u in range(3)])
    out = RR.rollout_ragged(gen, spec, torch.zeros(N, 2, dtype=torch.int64), seed, wp)
    # order (1, 2, 0): step 0 sees rows off[1], off[2], off[0]; step 1 recordings 1 and 2; step 2 recording 1 alone
    assert [c[0].tolist() for c in calls] == [[1.0, 4.0, 0.0], [2.0, 5.0], [3.0]]
    assert torch.equal(calls[0][1], seed[[1, 2, 0]])
    assert np.array_equal(calls[1][1].numpy(), out["windows"][[1, 4], 4:]) and np.array_equal(calls[2][1].numpy(), out["windows"][[2], 4:])
    assert out["track"].shape == (3, 3 * 4 + 2, 3) and out["track_frames"].tolist() == [6, 14, 10]
    assert not out["track"][0, 6:].any() and not out["track"][2, 10:].any() and out["track"][1, 13].any()


# ---- C ABI / binding -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("eg_generator_forward_rollout_ragged", "eg_generator_rollout_ragged_workspace_bytes", "eg_rollout_ragged_plan",
               "eg_rollout_ragged_plan_ints", "eg_rows_by_table", "eg_window_gather_ragged")


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


def test_ragged_workspace_depends_on_counts_only_and_equals_the_rectangle():
    lib, h = _generator()
    try:
        ws = lambda u, n: lib.eg_generator_rollout_ragged_workspace_bytes(h, u, n)
        assert ws(1, 12) < ws(2, 12) < ws(4, 12)                # grows with U at fixed N (the two prior buffers)
        assert ws(3, 3) < ws(3, 4) < ws(3, 12)                  # grows with N at fixed U
        assert ws(0, 3) == 0 and ws(-1, 3) == 0 and ws(4, 3) == 0 and ws(2, (1 << 20) + 1) == 0
        for U, W in [(1, 1), (1, 5), (2, 4), (5, 3), (8, 30)]:  # the plan table is the caller's buffer: a rectangle needs no more than today
            assert ws(U, U * W) == lib.eg_generator_rollout_workspace_bytes(h, U, W), (U, W)
    finally:
        lib.eg_generator_destroy(h)


def test_c_abi_refuses_bad_arguments_by_name():
    lib, h = _generator()
    buf = np.zeros(64, np.float32)                  # never read: the argument checks come before the first launch
    p = C.c_void_p(buf.ctypes.data)
    err = lambda: lib.eg_last_error().decode()
    try:
        def call(wp, ws_bytes=1 << 40, spec=p, plan=p, U=None, ws=p):
            arr = (C.c_int32 * max(len(wp), 1))(*wp)
            return lib.eg_generator_forward_rollout_ragged(h, p, len(wp) if U is None else U, arr, plan, spec, p, p, None, None, p, None, None, None,
                                                           None, None, ws, ws_bytes, None)
        n0 = lib.eg_launch_count()
        assert call((2, 0)) != 0 and "windows_per[1]=0" in err()
        assert call((-3, 2)) != 0 and "windows_per[0]=-3" in err()
        assert call((), U=0) != 0 and "utterances=0" in err()
        assert call((1 << 19, 1 << 19, 1)) != 0 and "total windows" in err()
        assert call((2, 3), ws_bytes=1024) != 0 and "workspace" in err()
        assert call((2, 3), spec=None) != 0 and "null pointer" in err()
        assert call((2, 3), plan=None) != 0 and "null pointer" in err()
        assert call((2, 3), ws=C.c_void_p(buf.ctypes.data + 4)) != 0 and "alignment" in err()
        # the ragged window gather: lengths are checked on the host against the row width
        lens = lambda *v: (C.c_int64 * len(v))(*v)
        gather = lambda U, stride, l, hop=32, n=48: lib.eg_window_gather_ragged(p, U, stride, l, p, hop, n, p, None)
        assert gather(2, 64, lens(64, 0)) != 0 and "lengths[1]=0" in err()
        assert gather(2, 64, lens(65, 3)) != 0 and "lengths[0]=65" in err()
        assert gather(0, 64, lens(5)) != 0 and "utterances=0" in err()
        assert gather(1, 64, lens(5), hop=0) != 0 and "hop_samples=0" in err()
        assert gather(1, 64, None) != 0 and "null pointer" in err()
        assert lib.eg_rows_by_table(p, p, p, 0, 4, 0, None) != 0 and "rows=0" in err()
        assert lib.eg_rows_by_table(p, None, p, 2, 4, 0, None) != 0 and "null pointer" in err()
        assert lib.eg_launch_count() == n0              # nothing was launched
    finally:
        lib.eg_generator_destroy(h)


def test_n_layers_above_eight_is_refused():
    lib = L.load()
    cfg = L.EgGeneratorConfig()
    L.check(lib.eg_generator_default_config(C.byref(cfg)))
    cfg.n_layers = 9
    h = C.c_void_p()
    L.check(lib.eg_generator_create(C.byref(cfg), C.byref(h)))
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    try:
        assert lib.eg_generator_rollout_ragged_workspace_bytes(h, 2, 5) == 0
        arr = (C.c_int32 * 2)(2, 3)
        assert lib.eg_generator_forward_rollout_ragged(h, p, 2, arr, p, p, p, p, None, None, p, None, None, None, None, None, p, 1 << 40, None) != 0
        assert "n_layers=9" in lib.eg_last_error().decode()
    finally:
        lib.eg_generator_destroy(h)


# ---- Python surface ---------------------------------------------------------------------------------------------------
def _engine():
    from emotiongestures_amd.engine import GeneratorEngine
    return GeneratorEngine()


def _args(wp=(2, 3)):
    N, U = sum(wp), len(wp)
    return dict(spec=torch.zeros(N, 128, 124), text=torch.zeros(N, 60, dtype=torch.int64), seed_pose=torch.zeros(U, 4, 126), windows_per=wp,
                sampled=torch.zeros(N, 34, 512), alpha=torch.zeros(4))


@pytest.mark.parametrize("arg,bad,needle", [
    ("spec", torch.zeros(5, 128, 100), "spec shape"),
    ("spec", torch.zeros(2, 3, 128, 124), "spec shape"),            # the engine takes packed rows; padding is Transformer.synthesize's
    ("spec", torch.zeros(6, 128, 124), "spec shape"),
    ("text", torch.zeros(4, 60, dtype=torch.int64), "text shape"),
    ("seed_pose", torch.zeros(2, 5, 126), "seed_pose shape"),
    ("seed_pose", torch.zeros(3, 4, 126), "seed_pose shape"),
    ("sampled", torch.zeros(5, 34, 256), "sampled shape"),
    ("alpha", torch.zeros(5), "alpha shape"),
    ("windows_per", (2, 0), "windows_per[1]=0"),
    ("windows_per", (), "utterances U=0"),
    ("windows_per", 5, "windows_per: need a sequence"),
])
def test_forward_rollout_ragged_refuses_wrong_shapes_by_name(arg, bad, needle):
    a = _args()
    a[arg] = bad
    with pytest.raises(L.EgError, match=re.escape(needle)):
        _engine().forward_rollout_ragged(a["spec"], a["text"], a["seed_pose"], a["windows_per"], a["sampled"], alpha=a["alpha"])


def test_forward_rollout_ragged_needs_loaded_weights():
    a = _args()
    with pytest.raises(L.EgError, match="before load_weights"):
        _engine().forward_rollout_ragged(a["spec"], a["text"], a["seed_pose"], a["windows_per"])


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_ragged_synthesize_is_eval_only(variant):
    model = build_mirror(variant, 34, 126, 4, 4, seed=1)
    a = _args()
    model.train()
    with pytest.raises(NotImplementedError, match="eval"):
        model.synthesize(a["spec"], a["text"], a["seed_pose"], windows_per=a["windows_per"])
    model.eval()
    with pytest.raises(L.EgError, match="GPU"):             # a CPU module is refused, not computed some other way
        model.synthesize(a["spec"], a["text"], a["seed_pose"], windows_per=a["windows_per"])


def test_harness_ragged_synthesize_is_eval_only_and_gpu_only():
    from emotiongestures_amd import harness as H
    model = build_mirror("spatial", 34, 126, 4, 4, seed=1).train()
    args = (torch.zeros(2, 100000), torch.zeros(2, 4, 60, dtype=torch.int64), torch.zeros(2, 4, 126))
    with pytest.raises(NotImplementedError, match="eval"):
        H.synthesize((model, None), *args, lengths=[100000, 40000])
    with pytest.raises(L.EgError, match="GPU"):
        H.synthesize((model.eval(), None), *args, lengths=[100000, 40000])
