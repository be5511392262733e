"""The smoothing filter without a GPU: eg_smooth_design against scipy and against the numpy restatement tests/smooth_np.py over every allowed
(window, polyorder, deriv), the float64 path of smooth.smooth_tracks, and the refusals by name of the design, the Python front end and
eg_smooth_tracks itself (which refuses before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.signal import savgol_coeffs, savgol_filter

import smooth_np as SN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import smooth as SM

DELTA = 1.0 / 15.0


def design(K, p, d, delta=DELTA):
    t64, t32 = np.zeros((K, K), np.float64), np.zeros((K, K), np.float32)
    rc = L.load().eg_smooth_design(K, p, d, delta, t64.ctypes.data_as(C.c_void_p), t32.ctypes.data_as(C.c_void_p))
    return rc, t64, t32


def test_design_against_scipy_for_every_allowed_filter():
    rng = np.random.default_rng(3)
    worst = [0.0, 0.0, 0.0]
    cases = SN.allowed()
    assert (3, 2, 2) in cases and (31, 5, 2) in cases and (3, 3, 0) not in cases and (9, 1, 2) not in cases and (5, 5, 0) not in cases
    for K, p, d in cases:
        rc, t64, t32 = design(K, p, d)
        assert rc == 0, (K, p, d, L.load().eg_last_error())
        assert np.array_equal(t32, t64.astype(np.float32))
        ref = savgol_coeffs(K, p, deriv=d, delta=DELTA, use="dot")
        e_row = np.abs(t64[K // 2] - ref).max() / np.abs(ref).max()
        x = rng.standard_normal((K + 7, 4))
        want = savgol_filter(x, K, p, deriv=d, delta=DELTA, axis=0, mode="interp")
        got, _mag = SN.smooth(x[None], SN.design(K, p, d, DELTA))
        e_np = np.abs(got[0] - want).max() / np.abs(want).max()
        lib, _mag = SN.smooth(x[None], t64)
        e_lib = np.abs(lib[0] - want).max() / np.abs(want).max()
        worst = [max(a, b) for a, b in zip(worst, (e_row, e_np, e_lib))]
        assert e_row <= 1e-9 and e_np <= 1e-9 and e_lib <= 1e-9, (K, p, d, e_row, e_np, e_lib)
    print(f"centre row vs savgol_coeffs {worst[0]:.2e}; restatement vs savgol_filter {worst[1]:.2e}; library table vs savgol_filter {worst[2]:.2e}")


def test_smoother_and_the_float64_path_of_smooth_tracks():
    sm = SM.Smoother(9, 3)
    assert (sm.window, sm.polyorder, sm.deriv, sm.half) == (9, 3, 0, 4) and sm.table.dtype == np.float64 and sm.table.shape == (9, 9)
    assert np.array_equal(sm.table32, sm.table.astype(np.float32))
    assert np.abs(sm.table - SN.design(9, 3, 0, DELTA)).max() <= 1e-12
    assert np.abs(sm.table.sum(1) - 1.0).max() <= 1e-12                      # a constant passes through every row
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3, 40, 5))
    frames = [9, 33]
    x[0, :, 9:] = np.nan
    x[1, :, 33:] = np.nan
    got = SM.smooth_tracks(x, sm, frames=frames)
    want, _mag = SN.smooth(x.reshape(6, 40, 5), sm.table, [9, 9, 9, 33, 33, 33])
    assert got.dtype == np.float64 and got.shape == x.shape and np.abs(got.reshape(6, 40, 5) - want).max() <= 1e-12
    assert not got[0, :, 9:].any() and not got[1, :, 33:].any()
    for u, n in enumerate(frames):
        ref = savgol_filter(x[u, 1, :n], 9, 3, axis=0, mode="interp")
        assert np.abs(got[u, 1, :n] - ref).max() <= 1e-9 * np.abs(ref).max()
    # [T, D] with a pair instead of a Smoother; a CPU tensor gives a float64 tensor; a derivative
    one = SM.smooth_tracks(x[1, 0, :33], (9, 3))
    assert np.array_equal(one, got[1, 0, :33])
    t = SM.smooth_tracks(torch.from_numpy(x[1, 0, :33].astype(np.float32)), SM.Smoother(9, 3, deriv=1, fps=15))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == (33, 5)
    ref = savgol_filter(x[1, 0, :33].astype(np.float32).astype(np.float64), 9, 3, deriv=1, delta=DELTA, axis=0, mode="interp")
    assert np.abs(t.numpy() - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("args,match", [
    ((8, 3), "window=8 is even"), ((33, 3), r"window=33 \(odd, 3\.\.31\)"), ((1, 1), "window=1"), ((5, 5), "polyorder=5"), ((9, 6), "polyorder=6"),
    ((9, 0), "polyorder=0"), ((9, 3, 3), "deriv=3"), ((9, 1, 2), "deriv=2 > polyorder=1"), ((9, 3, -1), "deriv=-1")])
def test_design_refusals_by_name(args, match):
    with pytest.raises(L.EgError, match=match):
        SM.Smoother(*args)
    K, p = args[:2]
    d = args[2] if len(args) == 3 else 0
    rc, t64, _t32 = design(K, p, d)
    assert rc != 0 and not t64.any()


def test_delta_and_argument_refusals_by_name():
    for fps in (0, -15, float("inf"), float("nan")):
        with pytest.raises(L.EgError, match="fps|delta"):
            SM.Smoother(9, 3, fps=fps)
    for delta in (0.0, -1.0, float("inf"), float("nan")):
        rc, _a, _b = design(9, 3, 1, delta)
        assert rc != 0 and b"delta" in L.load().eg_last_error()
    assert L.load().eg_smooth_design(9, 3, 0, DELTA, None, None) != 0 and b"null" in L.load().eg_last_error()
    with pytest.raises(L.EgError, match="Smoother or"):
        SM.smooth_tracks(np.zeros((20, 3)), 9)
    with pytest.raises(L.EgError, match="recording 1 has 8 valid frames < window=9"):
        SM.smooth_tracks(np.zeros((2, 20, 3)), (9, 3), frames=[20, 8])
    with pytest.raises(L.EgError, match="recording 0 has 8 valid frames < window=9"):
        SM.smooth_tracks(torch.zeros(8, 3), (9, 3))
    with pytest.raises(L.EgError, match="frames has 1 entries for 2"):
        SM.smooth_tracks(np.zeros((2, 20, 3)), (9, 3), frames=[20])
    with pytest.raises(L.EgError, match="at most two leading axes"):
        SM.smooth_tracks(np.zeros((1, 1, 1, 20, 3)), (9, 3))


def test_eg_smooth_tracks_refuses_before_any_launch():
    """No GPU here and none needed: every refusal returns before the launch (the addresses are never touched)."""
    lib = L.load()
    P = C.c_void_p
    frames = (C.c_int32 * 2)(20, 8)
    ok = dict(track=P(1 << 20), rows=2, T=20, D=5, K=9, table=P(1 << 16), frames=None, d_frames=None, draws=1, unit=1, out=P(1 << 22))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.eg_smooth_tracks(a["track"], a["rows"], a["T"], a["D"], a["K"], a["table"], a["frames"], a["d_frames"], a["draws"], a["unit"],
                                  a["out"], None)
        return rc, lib.eg_last_error().decode()

    for kw, word in [(dict(K=8), "even"), (dict(K=33), "window=33"), (dict(K=1), "window=1"), (dict(track=None), "null track"),
                     (dict(out=None), "null out"), (dict(table=None), "null d_table"), (dict(track=P((1 << 20) + 4)), "16-byte"),
                     (dict(table=P((1 << 16) + 8)), "16-byte"), (dict(out=P((1 << 20) + 16)), "overlaps"), (dict(rows=0), "rows=0"),
                     (dict(T=0), "frames=0"), (dict(D=0), "columns=0"), (dict(rows=3, draws=2), "multiple of draws"), (dict(unit=0), "frame_unit"),
                     (dict(T=8), "frames=8 < window=9"), (dict(frames=frames, d_frames=P(1 << 12)), "recording 1 has 8 valid frames"),
                     (dict(frames=frames), "go together"), (dict(d_frames=P(1 << 12)), "go together"),
                     (dict(rows=1 << 20, T=1 << 20, D=4), "index range")]:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert lib.eg_smooth_stream_state_bytes(3, 126, 9) == 4 * (3 * 8 * 126 + 3)
    assert lib.eg_smooth_stream_state_bytes(3, 126, 8) == 0 and lib.eg_smooth_stream_state_bytes(0, 126, 9) == 0
    rc = lib.eg_smooth_stream_push(P(1 << 20), 3, 30, 126, 31, P(1 << 16), P(1 << 22), None, P(1 << 24), None)
    assert rc != 0 and "window=31 > H=30" in lib.eg_last_error().decode()
    assert (lib.eg_smooth_tile_frames(), lib.eg_smooth_tile_cols()) == (SM.TILE_FRAMES, SM.TILE_COLS) == (L.EG_SMOOTH_TILE_FRAMES, L.EG_SMOOTH_TILE_COLS)


def test_callers_refuse_by_name_without_a_gpu():
    from emotiongestures_amd import harness as Hs
    with pytest.raises(L.EgError, match="smooth= together with joints="):
        from emotiongestures_amd import skeleton as SK
        Hs.open_stream((None, None), 2, torch.zeros(2, 4, 126), joints=SK.ted_expressive(), smooth=(9, 3))
    with pytest.raises(L.EgError, match="synthesize: smooth=: deriv=1"):
        Hs.synthesize((None, None), torch.zeros(2, 1000), torch.zeros(2, 1, 60), torch.zeros(2, 4, 126), smooth=SM.Smoother(9, 3, deriv=1))
    with pytest.raises(L.EgError, match="window=8 is even"):
        Hs.synthesize_takes((None, None), torch.zeros(2, 1000), torch.zeros(2, 1, 60), torch.zeros(2, 4, 126), draws=2, smooth=(8, 3))
