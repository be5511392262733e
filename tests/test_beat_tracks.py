"""Beat alignment of whole recordings, CPU side: the meta table (a host function of the library) against its numpy restatement, the
workspace size (0 for every refused shape), the C ABI's refusals by name before any device use, and the Python surface's refusals.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from conftest import build_mirror
from emotiongestures_amd import _lib as L

HOUR = 3600 * 16000                    # one hour at 16 kHz: 112 501 onset frames, 54 000 poses at 15 fps
NEW_SYMBOLS = ("eg_beat_tracks_meta_ints", "eg_beat_tracks_meta", "eg_beat_tracks_workspace_bytes", "eg_beat_align_tracks",
               "eg_beat_tracks_scan")


def _i32(v):
    a = np.ascontiguousarray(v, np.int32)
    return a, C.c_void_p(a.ctypes.data)


def meta_np(lengths, frames, t_end, fps):
    """The table restated: head {U, sum T, max T, max frames}, rows {length, T, frames, offset, t_end, 0, 0, 0}."""
    lengths = np.asarray(lengths, np.int64)
    U = lengths.size
    T = 1 + lengths // 512
    fr = np.zeros(U, np.int64) if frames is None else np.asarray(frames, np.int64)
    te = np.zeros(U, np.int64) if frames is None else (fr // fps if t_end is None else np.asarray(t_end, np.int64))
    rows = np.zeros((U, 8), np.int64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4] = lengths, T, fr, te
    rows[:, 3] = np.concatenate([[0], np.cumsum(T)[:-1]])
    return np.concatenate([[U, T.sum(), T.max(), fr.max()], rows.reshape(-1)]).astype(np.int32)


META_VECTORS = [
    ([64000], [60], None),                                                        # U = 1
    ([160000, 160000, 160000], [150, 150, 150], None),                            # equal lengths
    ([524287, 300000, 64000, 48123, 2048], [1025, 281, 60, 45, 2], None),
    ([HOUR, 2048, 9600000], [54000, 2, 9000], None),                              # a 1-hour entry
    ([1200000, 700123], [1125, 656], [70, 40]),                                   # explicit t_end
    ([64000, 2049, 511 * 512 + 511], None, None),                                 # audio half only
]


@pytest.mark.parametrize("lengths,frames,t_end", META_VECTORS)
def test_meta_table_equals_numpy_restatement(lengths, frames, t_end):
    lib = L.load()
    U = len(lengths)
    n = lib.eg_beat_tracks_meta_ints(U)
    assert n == 4 + 8 * U
    meta = np.full(n, -7, np.int32)
    _l, pl = _i32(lengths)
    _f, pf = _i32(frames) if frames is not None else (None, None)
    _t, pt = _i32(t_end) if t_end is not None else (None, None)
    L.check(lib.eg_beat_tracks_meta(pl, pf, pt, 15, U, C.c_void_p(meta.ctypes.data)), "eg_beat_tracks_meta")
    assert np.array_equal(meta, meta_np(lengths, frames, t_end, 15))
    if HOUR in lengths:
        assert meta[2] == 112501 and meta[3] == 54000
        assert lib.eg_beat_tracks_workspace_bytes(pl, pf, U, 1, 54000) > 0         # an hour per recording is accepted


def test_meta_ints_and_meta_refusals():
    lib = L.load()
    assert lib.eg_beat_tracks_meta_ints(0) == 0 and lib.eg_beat_tracks_meta_ints(-3) == 0
    meta = np.zeros(64, np.int32)
    pm = C.c_void_p(meta.ctypes.data)
    _l, pl = _i32([64000, 2047])
    assert lib.eg_beat_tracks_meta(pl, None, None, 15, 2, pm) != 0 and "lengths[1]=2047" in lib.eg_last_error().decode()
    _l2, pl2 = _i32([64000, 64000])
    _f, pf = _i32([60, 1])
    assert lib.eg_beat_tracks_meta(pl2, pf, None, 15, 2, pm) != 0 and "frames[1]=1" in lib.eg_last_error().decode()
    assert lib.eg_beat_tracks_meta(pl2, None, None, 15, 0, pm) != 0 and "U=0" in lib.eg_last_error().decode()
    assert lib.eg_beat_tracks_meta(pl2, None, None, 15, 2, None) != 0 and "null meta" in lib.eg_last_error().decode()


def test_workspace_is_zero_for_every_refused_shape_and_grows_with_the_work():
    lib = L.load()
    _l, pl = _i32([64000, 48123])
    _f, pf = _i32([60, 45])
    ok = lib.eg_beat_tracks_workspace_bytes(pl, pf, 2, 1, 60)
    assert ok > 129 * (126 + 94) * 4                                            # holds at least the mel dB and rms arrays
    assert lib.eg_beat_tracks_workspace_bytes(pl, pf, 2, 3, 60) > ok             # more draws: more pose rows
    assert 0 < lib.eg_beat_tracks_workspace_bytes(pl, None, 2, 1, 0) < ok        # audio half only
    bad = [
        (None, pf, 2, 1, 60),                                                     # null lengths
        (pl, pf, 0, 1, 60), (pl, pf, -1, 1, 60), (pl, pf, 70000, 1, 60),          # U
        (pl, pf, 2, 0, 60), (pl, pf, 2, -2, 60),                                  # draws
        (pl, pf, 2, 1, 59),                                                       # frames[0] > Tmax
        (pl, pf, 2, 1, 1),                                                        # Tmax
        (pl, pf, 2, 40000, 60),                                                   # U * draws beyond the grid range
        (_i32([2047, 64000])[1], pf, 2, 1, 60),                                   # a length below one FFT
        (pl, _i32([60, 1])[1], 2, 1, 60),                                         # a single pose
        (pl, _i32([60, 0])[1], 2, 1, 60),
    ]
    for args in bad:
        assert lib.eg_beat_tracks_workspace_bytes(*args) == 0, args
    # sizes beyond the index types: 2^24 onset frames in all, 2^31 pose-beat slots
    many = np.full(200, HOUR, np.int32)
    assert lib.eg_beat_tracks_workspace_bytes(C.c_void_p(many.ctypes.data), None, 200, 1, 0) == 0
    assert "index range" in lib.eg_last_error().decode()
    assert lib.eg_beat_tracks_workspace_bytes(pl, _i32([60, 45])[1], 2, 4000, 60000) == 0
    assert "index range" in lib.eg_last_error().decode()


def _call(lib, **over):
    """eg_beat_align_tracks with dummy non-null pointers: every refusal comes before the first launch, so nothing is dereferenced."""
    lengths, frames = over.pop("lengths", [64000, 48123]), over.pop("frames", [60, 45])
    lengths, frames = [(None, None) if v is None else _i32(v) for v in (lengths, frames)]
    dummy = C.c_void_p(256)
    a = dict(audio=dummy, U=2, stride=64000, lengths=lengths[1], d_meta=dummy, pose=dummy, draws=1, Tmax=60, pose_dim=282, frames=frames[1],
             fps=15, t_start=0, t_end=None, sigma=0.3, order=2, fb=dummy, win=dummy, tw=dummy, band=dummy, ws=dummy, ws_bytes=1 << 40,
             score=dummy, nab=None, oenv=None, rms=None, am=None, pm=None, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    if isinstance(a["t_end"], list):
        keep = _i32(a["t_end"])
        a["t_end"] = keep[1]
    rc = lib.eg_beat_align_tracks(*a.values())
    return rc, lib.eg_last_error().decode()


REFUSALS = [
    (dict(audio=None), "null pointer"), (dict(d_meta=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(fb=None), "null pointer"),
    (dict(band=None), "null pointer"), (dict(lengths=None), "null"), (dict(score=None), "null frames / score"),
    (dict(frames=None), "null frames / score"),
    (dict(U=0), "U=0"), (dict(U=-1), "U=-1"), (dict(draws=0), "draws=0"), (dict(draws=-4), "draws=-4"),
    (dict(lengths=[64000, 2047]), "lengths[1]=2047"), (dict(lengths=[64001, 48123]), "lengths[0]=64001 exceeds stride=64000"),
    (dict(frames=[60, 1]), "frames[1]=1"), (dict(frames=[61, 45]), "frames[0]=61 (2..Tmax=60)"),
    (dict(pose_dim=173), "pose_dim=173"), (dict(pose_dim=126), "the beat joints are columns 18:42 and 150:174"),
    (dict(fps=0), "pose_fps=0"), (dict(order=0), "order=0"), (dict(sigma=0.0), "sigma=0"), (dict(sigma=-1.0), "sigma=-1"),
    (dict(t_start=-1), "t_start=-1"), (dict(t_start=4), "t_start=4 t_end[0]=4"), (dict(t_end=[4, 0]), "t_end[1]=0"),
    (dict(ws_bytes=1024), "workspace too small"), (dict(stride=2047), "stride=2047"),
    (dict(draws=40000), "grid range"), (dict(Tmax=60000, draws=4000), "index range"),
]


@pytest.mark.parametrize("over,needle", REFUSALS, ids=[n for _o, n in REFUSALS])
def test_call_refuses_by_name_before_any_device_use(over, needle):
    lib = L.load()
    before = lib.eg_launch_count()
    rc, msg = _call(lib, **over)
    assert rc != 0 and "eg_beat_align_tracks" in msg and needle in msg, (rc, msg)
    assert lib.eg_launch_count() == before


def test_scan_entry_refuses_null_and_short_workspace():
    lib = L.load()
    _l, pl = _i32([64000])
    dummy = C.c_void_p(256)
    assert lib.eg_beat_tracks_scan(None, pl, 1, dummy, dummy, 1 << 40, dummy, dummy, None) != 0
    assert "null pointer" in lib.eg_last_error().decode()
    assert lib.eg_beat_tracks_scan(dummy, pl, 1, dummy, dummy, 16, dummy, dummy, None) != 0
    assert "workspace too small" in lib.eg_last_error().decode()


def test_python_surface_refuses_cpu_tensors_and_ted_generators():
    from emotiongestures_amd import harness as H
    from emotiongestures_amd.beat import beat_alignment_tracks
    audio, track = torch.zeros(2, 64000), torch.zeros(2, 60, 282)
    with pytest.raises(RuntimeError, match="audio must be a CUDA tensor"):
        beat_alignment_tracks(audio, track)
    gen = build_mirror("spatial", 34, 126, 4, 4, seed=3).eval()                  # TED: 126 pose columns, no beat joints
    with pytest.raises(L.EgError, match=re.escape("the beat joints are columns 18:42 and 150:174")):
        H.synthesize((gen, None), torch.zeros(1, 64000), torch.zeros(1, 2, 60, dtype=torch.long), torch.zeros(1, 4, 126), beat=True)


def test_new_symbols_are_declared_and_bound():
    import os
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.SIGNATURES and getattr(lib, name) is not None
