"""Takes roll-out (R draws of recordings with their own window counts), CPU side: the plan with its slot_rank section against its numpy
restatement, the C ABI's argument checks and workspace size, and the Python surface's refusals.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rollout_takes_np as RT
from conftest import ROOT, build_mirror
from emotiongestures_amd import _lib as L

NEW_SYMBOLS = ("eg_generator_forward_rollout_takes", "eg_generator_rollout_takes_workspace_bytes", "eg_rollout_takes_plan",
               "eg_rollout_takes_plan_ints")
FN = "eg_generator_forward_rollout_takes"
PLAN_VECTORS = [(3, 1, 2), (1, 4, 4, 2, 1), (2, 2), (1,), (5,)]


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


def _c_plan(fn, wp, ints):
    lib = L.load()
    U, Wmax = len(wp), max(wp)
    arr = (C.c_int32 * U)(*wp)
    order, inverse, batch, table = (np.zeros(n, np.int32) for n in (U, U, Wmax, ints))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(getattr(lib, fn)(arr, U, ptr(order), ptr(inverse), ptr(batch), ptr(table)), fn)
    return order, inverse, batch, table


@pytest.mark.parametrize("wp", PLAN_VECTORS)
def test_takes_plan_is_the_ragged_table_followed_by_slot_rank(wp):
    lib = L.load()
    U, N = len(wp), sum(wp)
    assert lib.eg_rollout_takes_plan_ints(U, N) == 2 * N + 2 * U
    order, inverse, batch, table = _c_plan("eg_rollout_takes_plan", wp, 2 * N + 2 * U)
    r_order, r_inverse, r_batch, r_table = _c_plan("eg_rollout_ragged_plan", wp, int(lib.eg_rollout_ragged_plan_ints(U, N)))
    assert r_table.size == N + 2 * U and np.array_equal(table[: N + 2 * U], r_table)
    assert np.array_equal(order, r_order) and np.array_equal(inverse, r_inverse) and np.array_equal(batch, r_batch)
    pl = RT.plan(wp)
    assert np.array_equal(table[N + 2 * U:], pl["slot_rank"]) and np.array_equal(table, pl["table"])
    # what the fusion kernel derives from the table: for slot (s, rank) the recording's offset, its count and the step
    slot = 0
    for s in range(max(wp)):
        for rank in range(int(pl["step_batch"][s])):
            u = int(pl["order"][rank])
            assert table[N + 2 * U + slot] == rank and table[rank] == pl["offsets"][u] and table[N + U + rank] == wp[u]
            assert table[slot] - table[rank] == s
            slot += 1
    assert slot == N


def test_takes_plan_refuses_bad_counts_by_name():
    lib = L.load()
    ints = lib.eg_rollout_takes_plan_ints
    assert ints(3, 7) == 20 and ints(1, 1) == 4
    for U, N in ((0, 3), (-1, 3), (4, 3), (2, (1 << 20) + 1)):
        assert ints(U, N) == 0, (U, N)
    err = lambda: lib.eg_last_error().decode()
    call = lambda wp, U=None: lib.eg_rollout_takes_plan((C.c_int32 * max(len(wp), 1))(*wp), len(wp) if U is None else U, None, None, None, None)
    assert call((2, 0)) != 0 and "eg_rollout_takes_plan: windows_per[1]=0" in err()
    assert call((), U=0) != 0 and "eg_rollout_takes_plan: utterances=0" in err()
    assert call((1 << 19, 1 << 19, 1)) != 0 and "eg_rollout_takes_plan: total windows" in err()
    assert lib.eg_rollout_takes_plan(None, 2, None, None, None, None) != 0 and "eg_rollout_takes_plan: null pointer" in err()
    assert call((3, 1, 2)) == 0              # every output is optional


def _generator(**over):
    lib = L.load()
    cfg = L.EgGeneratorConfig()
    L.check(lib.eg_generator_default_config(C.byref(cfg)))
    for k, v in over.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    L.check(lib.eg_generator_create(C.byref(cfg), C.byref(h)))
    return lib, h


def test_workspace_is_the_draws_calls_on_a_rectangle_and_below_the_replicated_ragged_calls():
    lib, h = _generator()
    try:
        ws = lambda u, n, r: lib.eg_generator_rollout_takes_workspace_bytes(h, u, n, r)
        for U, W, R in ((1, 1, 2), (2, 3, 3), (5, 2, 4), (1, 7, 2), (3, 1, 5)):           # (3, 1, 5): U*R > N, the prior buffers taken again
            assert ws(U, U * W, R) == lib.eg_generator_rollout_draws_workspace_bytes(h, U, W, R) > 0, (U, W, R)
        for U, N in ((3, 6), (5, 12), (1, 1), (3, 8)):
            assert ws(U, N, 1) == lib.eg_generator_rollout_ragged_workspace_bytes(h, U, N) > 0
            for R in (2, 3, 4, 5):
                # the tower side is carved once per window: R takes cost less than R times the recordings
                assert ws(U, N, R - 1) < ws(U, N, R) < lib.eg_generator_rollout_ragged_workspace_bytes(h, U * R, N * R), (U, N, R)
        for U, N, R in ((0, 3, 2), (-1, 3, 2), (4, 3, 2), (2, 3, 0), (2, 3, -1), (2, (1 << 20) + 1, 1), (2, 1 << 19, 4), (1, 1, (1 << 20) + 1)):
            assert ws(U, N, R) == 0, (U, N, R)
        assert lib.eg_generator_rollout_takes_workspace_bytes(None, 2, 3, 2) == 0
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

    def call(wp=(2, 3), R=2, U=None, ws_bytes=1 << 50, g=h, arena=p, wpp=True, plan=p, spec=p, text=p, seed=p, sampled=p, track=p, txt=None, ws=p):
        arr = (C.c_int32 * max(len(wp), 1))(*wp) if wpp else None
        return lib.eg_generator_forward_rollout_takes(g, arena, len(wp) if U is None else U, R, arr, plan, spec, text, seed, sampled, None, track,
                                                      None, None, None, None, txt, ws, ws_bytes, None)
    try:
        for kw in (dict(g=None), dict(arena=None), dict(wpp=False), dict(plan=None), dict(spec=None), dict(seed=None), dict(sampled=None),
                   dict(track=None), dict(ws=None)):
            assert call(**kw) != 0 and FN + ": null pointer" in err(), kw
        assert call((), U=0) != 0 and FN in err() and "utterances=0" in err()
        assert call(R=0) != 0 and FN in err() and "draws=0" in err()
        assert call(R=-2) != 0 and "draws=-2" in err()
        assert call((2, 0)) != 0 and FN in err() and "windows_per[1]=0" in err()
        assert call((-3, 2)) != 0 and "windows_per[0]=-3" in err()
        assert call((1 << 19, 1 << 19, 1), R=1) != 0 and FN in err() and "total windows*draws" in err() and "2^20" in err()
        assert call((1 << 18, 1 << 18), R=4) != 0 and FN in err() and "total windows*draws" in err()
        assert call(text=None, txt=p) != 0 and FN in err() and "text_embedding wanted without text" in err()
        assert call(ws_bytes=1024) != 0 and FN in err() and "workspace 1024 <" in err()
        assert call(R=1, ws_bytes=1024) != 0 and FN in err() and "workspace 1024 <" in err()
        for kw in (dict(ws=odd), dict(arena=odd), dict(spec=odd), dict(sampled=odd)):
            assert call(**kw) != 0 and FN in err() and "16-byte alignment" in err(), kw
        assert call(plan=C.c_void_p(p.value + 2)) != 0 and FN in err() and "plan: 4-byte" in err()
    finally:
        lib.eg_generator_destroy(h)
    lib9, h9 = _generator(n_layers=9)
    try:
        assert call(g=h9) != 0 and FN in err() and "n_layers=9 > 8" in err()
        assert lib9.eg_generator_rollout_takes_workspace_bytes(h9, 2, 5, 2) == 0
    finally:
        lib9.eg_generator_destroy(h9)
    assert lib.eg_launch_count() == n0


# ---- the definition's helper ----------------------------------------------------------------------------------------------
def test_replicate_ragged_puts_window_w_of_draw_r_at_row_R_off_plus_r_W_plus_w():
    wp, Rd = (3, 1, 2), 2
    U, N = len(wp), sum(wp)
    spec = torch.arange(N, dtype=torch.float32).reshape(N, 1, 1)
    sampled = torch.arange(N * Rd, dtype=torch.float32).reshape(N * Rd, 1, 1)
    s, t, p, e = RT.replicate_ragged(spec, torch.zeros(N, 1, dtype=torch.int64), torch.arange(U, dtype=torch.float32).reshape(U, 1, 1), wp, sampled)
    assert s.shape == (N * Rd, 1, 1) and t.shape == (N * Rd, 1) and p.shape == (U * Rd, 1, 1) and e is sampled
    off, tr = [0, 3, 4], RT.take_rows(wp, Rd)
    assert tr.tolist() == [[0, 3], [6, 7], [8, 10]] and RT.repeat(wp, Rd) == (3, 3, 1, 1, 2, 2)
    for u in range(U):
        for r in range(Rd):
            assert float(p[u * Rd + r]) == u
            for w in range(wp[u]):
                assert float(s[tr[u, r] + w]) == off[u] + w
    assert RT.first_take_rows(wp, Rd).tolist() == [0, 1, 2, 6, 8, 9]


# ---- Python surface ---------------------------------------------------------------------------------------------------
def _engine():
    from emotiongestures_amd.engine import GeneratorEngine
    return GeneratorEngine()


def _args(wp=(2, 3), Rd=4):
    N, U = sum(wp), len(wp)
    return dict(spec=torch.zeros(N, 128, 124), text=torch.zeros(N, 60, dtype=torch.int64), seed_pose=torch.zeros(U, 4, 126), windows_per=wp,
                sampled=torch.zeros(N * Rd, 34, 512), alpha=torch.zeros(4))


@pytest.mark.parametrize("arg,bad,needle", [
    ("sampled", None, "sampled: required, shape (N*R,F,d_model)"),
    ("sampled", torch.zeros(2, 4, 3, 34, 512), "sampled shape (2, 4, 3, 34, 512) != (N*R,F,d_model) = (5*R,34,512)"),   # padding is synthesize_takes'
    ("sampled", torch.zeros(12, 34, 512), "!= (N*R,F,d_model) = (5*R,34,512)"),          # not a multiple of N
    ("sampled", torch.zeros(0, 34, 512), "!= (N*R,F,d_model)"),
    ("sampled", torch.zeros(20, 34, 256), "!= (N*R,F,d_model)"),
    ("spec", torch.zeros(5, 128, 100), "spec shape"),
    ("spec", torch.zeros(2, 3, 128, 124), "spec shape"),
    ("text", torch.zeros(4, 60, dtype=torch.int64), "text shape"),
    ("seed_pose", torch.zeros(2, 5, 126), "seed_pose shape"),
    ("seed_pose", torch.zeros(8, 4, 126), "seed_pose shape"),          # one seed per recording, not per (recording, draw)
    ("alpha", torch.zeros(5), "alpha shape"),
    ("windows_per", (2, 0), "windows_per[1]=0"),
    ("windows_per", (), "utterances U=0"),
    ("windows_per", 5, "windows_per: need a sequence"),
])
def test_forward_rollout_takes_refuses_wrong_shapes_by_name(arg, bad, needle):
    a = _args()
    a[arg] = bad
    with pytest.raises(L.EgError, match=re.escape(needle)):
        _engine().forward_rollout_takes(a["spec"], a["text"], a["seed_pose"], a["windows_per"], a["sampled"], alpha=a["alpha"])


def test_forward_rollout_takes_checks_a_caller_owned_track_and_needs_loaded_weights():
    a = _args()
    with pytest.raises(L.EgError, match=re.escape("track: need a contiguous float32 GPU tensor [2,4,94,126]")):
        _engine().forward_rollout_takes(a["spec"], a["text"], a["seed_pose"], a["windows_per"], a["sampled"], track=torch.zeros(2, 4, 94, 126))
    with pytest.raises(L.EgError, match="forward_rollout_takes before load_weights"):
        _engine().forward_rollout_takes(a["spec"], a["text"], a["seed_pose"], a["windows_per"], a["sampled"])


@pytest.mark.parametrize("variant", ["spatial", "memory"])
def test_synthesize_takes_is_eval_only_and_checks_its_arguments(variant):
    model = build_mirror(variant, 34, 126, 4, 4, seed=1)
    a = _args()
    run = lambda sampled, **kw: model.synthesize_takes(a["spec"], a["text"], a["seed_pose"], sampled, **{"windows_per": a["windows_per"], **kw})
    padded = torch.zeros(2, 4, 3, 34, 512)
    model.train()
    with pytest.raises(NotImplementedError, match="eval"):
        run(a["sampled"], draws=4)
    model.eval()
    with pytest.raises(L.EgError, match=re.escape("!= (U,R,Wmax,F,d_model) with U=2, R=3")):         # shape[1] != draws
        run(padded, draws=3)
    with pytest.raises(L.EgError, match=re.escape("!= (U,R,Wmax,F,d_model) with U=2, R=4")):         # shape[0] != U
        run(torch.zeros(3, 4, 3, 34, 512), draws=4)
    with pytest.raises(L.EgError, match=re.escape("!= (N*R,F,d_model) with N*R=5*3")):                # packed rows != N * draws
        run(a["sampled"], draws=3)
    with pytest.raises(L.EgError, match=re.escape("need padded (U,R,Wmax,F,d_model) or packed (N*R,F,d_model) with R=4")):
        run(None, draws=4)
    with pytest.raises(L.EgError, match=re.escape("need padded (U,R,Wmax,F,d_model) or packed")):
        run(torch.zeros(2, 3, 34, 512), draws=4)
    with pytest.raises(L.EgError, match="synthesize_takes: draws=0"):
        run(a["sampled"], draws=0)
    with pytest.raises(L.EgError, match="windows_per: need a sequence"):
        run(a["sampled"], draws=4, windows_per=5)
    with pytest.raises(TypeError):              # both are required keywords
        model.synthesize_takes(a["spec"], a["text"], a["seed_pose"], a["sampled"], draws=4)
    for s in (a["sampled"], padded):
        with pytest.raises(L.EgError, match="GPU"):             # a CPU module is refused, not computed some other way
            run(s, draws=4)


def test_harness_synthesize_takes_refusals():
    from emotiongestures_amd import harness as H
    assert "synthesize_takes" in H.__all__
    model = build_mirror("spatial", 34, 126, 4, 4, seed=1)
    audio, text, seed = torch.zeros(2, 100000), torch.zeros(2, 4, 60, dtype=torch.int64), torch.zeros(2, 4, 126)
    model.train()
    with pytest.raises(NotImplementedError, match="eval"):
        H.synthesize_takes((model, object()), audio, text, seed, lengths=[100000, 40000], draws=2)
    model.eval()
    with pytest.raises(L.EgError, match="synthesize_takes: draws= needs a VAE"):
        H.synthesize_takes((model, None), audio, text, seed, lengths=[100000, 40000], draws=2)
    with pytest.raises(L.EgError, match="synthesize_takes: draws=0"):
        H.synthesize_takes((model, object()), audio, text, seed, lengths=[100000, 40000], draws=0)
    with pytest.raises(L.EgError, match="synthesize_takes: diversity= needs draws >= 2"):
        H.synthesize_takes((model, object()), audio, text, seed, lengths=[100000, 40000], draws=1, diversity=object())
    with pytest.raises(L.EgError, match="synthesize_takes: beat=True: pose_dim=126"):
        H.synthesize_takes((model, object()), audio, text, seed, lengths=None, draws=2, beat=True)
    with pytest.raises(L.EgError, match="GPU"):             # lengths=None is accepted: the call gets as far as the engine
        H.synthesize_takes((model, object()), audio, text, seed, lengths=None, draws=2)


def test_the_old_refusals_still_raise_and_name_synthesize_takes():
    from emotiongestures_amd import harness as H
    model = build_mirror("spatial", 34, 126, 4, 4, seed=1).eval()
    with pytest.raises(L.EgError, match="draws= with windows_per= is not supported.*rectangular") as e:
        model.synthesize(torch.zeros(2, 3, 128, 124), torch.zeros(2, 3, 60, dtype=torch.int64), torch.zeros(2, 4, 126), torch.zeros(2, 4, 3, 34, 512),
                         draws=4, windows_per=[3, 3])
    assert "synthesize_takes" in str(e.value)
    with pytest.raises(L.EgError, match="draws= with lengths= is not supported.*rectangular") as e:
        H.synthesize((model, object()), torch.zeros(2, 100000), torch.zeros(2, 2, 60, dtype=torch.int64), torch.zeros(2, 4, 126), draws=2,
                     lengths=[100000, 90000])
    assert "synthesize_takes" in str(e.value)
