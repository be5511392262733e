"""BVH text of whole takes, the part that needs no GPU: the host export of the device's decimal routine (eg_bvh_text_decimal) against Python's
``"%.6f"`` and the integer restatement tests/bvh_text_np.py; ``BvhFile.format_tracks`` on the host against ``format`` per take; the refusals of
the C ABI (they return before the first launch, so the fake device addresses are never touched) and of the Python surface; and ``format``
itself, whose channel logic moved into a helper, against the text built the way it was built before."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bvh_text_np as TN
import test_euler_bvh as TEB
from conftest import ROOT
from emotiongestures_amd import _lib as L
from emotiongestures_amd import bvh as BVH

NEW_SYMBOLS = ("eg_bvh_text_decimal", "eg_bvh_text_tile_frames", "eg_bvh_text_table_bytes", "eg_bvh_text_workspace_bytes", "eg_bvh_text_measure",
               "eg_bvh_text_write")
P = C.c_void_p
EG_ERR_BAD_ARG, EG_ERR_WORKSPACE, EG_ERR_ALIGN = -1, -3, -5

SMALL = TN.SMALL


def decimal(lib, v, buf=C.create_string_buffer(20)):
    n = lib.eg_bvh_text_decimal(float(v), buf)
    return None if n < 0 else buf.raw[:n].decode("ascii")


special_values = TN.special_values


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header, re.S)
        assert decl and name in L.SIGNATURES and getattr(lib, name) is not None, name
        n_args = 0 if decl.group(1).strip() == "void" else len(decl.group(1).split(","))
        assert n_args == len(L.SIGNATURES[name][1]), name
    for macro, value in (("MAX_CHANNELS", 512), ("MAX_WIDTH", 18), ("TILE_FRAMES", TN.TILE_FRAMES)):
        assert int(re.search(r"#define EG_BVH_TEXT_%s (\d+)" % macro, header).group(1)) == value == getattr(L, "EG_BVH_TEXT_" + macro)
    assert lib.eg_bvh_text_tile_frames() == BVH.TEXT_TILE_FRAMES == TN.TILE_FRAMES
    body = re.search(r"typedef\s+struct\s+EgBvhTextArgs\s*\{(.*?)\}\s*EgBvhTextArgs\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    names = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            first, *rest = [p.strip() for p in decl.split(",")]
            names += [re.search(r"(\w+)$", first).group(1)] + rest
    assert names == [n for n, _t in L.EgBvhTextArgs._fields_]


def test_decimal_equals_percent_f_and_the_restatement():
    lib = L.load()
    rng = np.random.default_rng(5)
    scales = (1e-7, 1e-5, 1e-3, 1.0, 180.0, 1e4, 1e7, 2.0e9)
    vals = np.concatenate([(rng.standard_normal(16000) * s).astype(np.float32) for s in scales] + [special_values()])
    vals = vals[np.isfinite(vals) & (np.abs(vals) < 2.0 ** 31)]
    assert len(vals) >= 10 ** 5
    for v in vals:
        want = "%.6f" % float(v)
        got = decimal(lib, v)
        assert got == want == TN.decimal6(v), (float(v).hex(), got, want, TN.decimal6(v))
        assert 8 <= len(got) <= TN.MAX_WIDTH
    assert max(len(decimal(lib, v)) for v in vals) == 18 and min(len(decimal(lib, v)) for v in special_values()) == 8


def test_decimal_on_exact_ties():
    """k * 2^-m: the sixth decimal is decided by a tie exactly when the value is an odd multiple of 2^-7 (k * 15625 / 2): the 200 odd k
    below 400 at m = 7, and the k at m > 7 that reduce to one.  Ties go to the even neighbour."""
    lib = L.load()
    ties = 0
    for m in range(1, 12):
        for k in list(range(1, 400)) + [2 ** 20 + 1, 2 ** 22 + 3, 2 ** 23 - 1]:
            v = np.float32(k * 2.0 ** -m)
            for s in (v, -v):
                assert decimal(lib, s) == "%.6f" % float(s) == TN.decimal6(s), float(s).hex()
            ties += TN.is_tie(v)
    assert ties >= 200
    assert decimal(lib, 0.0078125) == "0.007812" and decimal(lib, 3 * 0.0078125) == "0.023438"


def test_decimal_special_values_and_refusals():
    lib = L.load()
    want = [(0.0, "0.000000"), (-0.0, "-0.000000"), (1e-9, "0.000000"), (-1e-9, "-0.000000"),
            # fp32 has no value in [10 - 5e-7, 10): 9.9999995 and 999.9999995 round to their fp32 neighbours first; a carry into the integer
            # part exists below 4 only, where the spacing is under 5e-7
            (9.9999995, "9.999999"), (999.9999995, "1000.000000"), (np.nextafter(np.float32(4), np.float32(0)), "4.000000"),
            (np.nextafter(np.float32(1), np.float32(0)), "1.000000"), (2147483520.0, "2147483520.000000"), (-2147483520.0, "-2147483520.000000")]
    for v, text in want:
        assert decimal(lib, np.float32(v)) == text == TN.decimal6(np.float32(v)) == "%.6f" % float(np.float32(v))
    for v in special_values():
        assert decimal(lib, v) == "%.6f" % float(v) == TN.decimal6(v)
    for v in (float("nan"), float("inf"), float("-inf"), 2.0 ** 31, -2.0 ** 31, 3e38):
        assert decimal(lib, v) is None and not TN.writable(v)
    assert lib.eg_bvh_text_decimal(1.0, None) == -1


def _file(root_channels="Xposition Yposition Zposition Zrotation Xrotation Yrotation"):
    n = len(root_channels.split())
    return BVH.parse(SMALL.replace("CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation", f"CHANNELS {n} {root_channels}"))


@pytest.mark.parametrize("as_tensor", [False, True])
def test_format_tracks_on_the_host_equals_format_per_take(as_tensor):
    f = _file()
    rng = np.random.default_rng(11)
    U, R, T = 2, 2, 7
    frames = [T, 3]
    rp = rng.standard_normal((U, T, 3)) * 50
    for joints in (None, ["Hips", "Arm"]):
        J = 4 if joints is None else 2
        e = rng.standard_normal((U, R, T, J, 3)) * 120
        e[1, :, 3:] = np.nan                                                       # behind the valid frames: never read
        x = torch.from_numpy(e).float() if as_tensor else e
        for root in (None, rp):
            bt = f.format_tracks(x, frames, joints=joints, frame_time=1 / 30, root_position=root)
            assert bt.lead == (U, R) and bt.frames == frames and bt.offsets.dtype == np.int64 and len(bt.offsets) == U * R + 1
            assert bt.body.dtype == torch.uint8 and not bt.body.is_cuda and bt.offsets[-1] == bt.body.numel()
            for u in range(U):
                for r in range(R):
                    n = frames[u]
                    take = np.asarray(x[u, r, :n])
                    want = f.format(take, joints, 1 / 30, None if root is None else root[u, :n].astype(np.float32))
                    assert bt.text(u, r) == want and bt.tobytes(u, r) == want.encode() and want.startswith(bt.head(u, r))
                    assert BVH.parse(bt.text(u, r)).frames == n
    e = rng.standard_normal((U, R, T, 4, 3)) * 120
    one = f.format_tracks(e[0, 0], frame_time=0.04)                                 # no leading axes
    assert one.lead == () and one.text() == f.format(e[0, 0], frame_time=0.04)
    rows = f.format_tracks(e[:, 0], [T, 1], frame_time=0.04, root_position=rp)
    assert rows.lead == (U,) and rows.text(1) == f.format(e[1, 0, :1], frame_time=0.04, root_position=rp[1, :1].astype(np.float32))


def test_restatement_equals_format():
    for f in (_file(), _file("Yposition Xposition Zrotation Xrotation Yrotation")):
        rng = np.random.default_rng(12)
        e = (rng.standard_normal((2, 5, 4, 3)) * 100).astype(np.float32)
        rp = (rng.standard_normal((2, 5, 3)) * 10).astype(np.float32)
        for root in (None, rp):
            src = f._channel_sources(f._rotating(None, "test"), root is not None)
            data, offsets, _lines = TN.body(src, e.reshape(2, 5, 12), [5, 2], root)
            for b, n in enumerate([5, 2]):
                want = f.format(e[b, :n], frame_time=0.04, root_position=None if root is None else root[b, :n])
                assert want.endswith(data[offsets[b]:offsets[b + 1]].decode()) and data[offsets[b]:offsets[b + 1]].count(b"\n") == n


def test_write_tracks(tmp_path):
    f = _file()
    e = np.random.default_rng(13).standard_normal((2, 2, 4, 4, 3)) * 90
    paths = f.write_tracks(str(tmp_path / "takes"), e, [4, 2], frame_time=0.05)
    assert [os.path.basename(p) for p in paths] == ["take_000_00.bvh", "take_000_01.bvh", "take_001_00.bvh", "take_001_01.bvh"]
    for b, p in enumerate(paths):
        assert open(p).read() == f.format(e[b // 2, b % 2, :[4, 2][b // 2]], frame_time=0.05)
    named = [str(tmp_path / f"t{i}.bvh") for i in range(4)]
    assert f.format_tracks(e, [4, 2], frame_time=0.05).write(named) == named and open(named[3]).read() == open(paths[3]).read()
    with pytest.raises(L.EgError, match="BvhText.write: 3 paths for 4 takes"):
        f.format_tracks(e, [4, 2], frame_time=0.05).write(named[:3])


def test_python_refusals_by_name():
    f = _file()
    e = np.zeros((2, 3, 4, 3))
    with pytest.raises(L.EgError, match=r"BvhFile.format_tracks: euler shape \(2, 3, 5, 3\): need \[T, 4, 3\]"):
        f.format_tracks(np.zeros((2, 3, 5, 3)), frame_time=0.1)
    with pytest.raises(L.EgError, match="BvhFile.format_tracks: recording 1 has 0 valid frames < 1"):
        f.format_tracks(e, [3, 0], frame_time=0.1)
    with pytest.raises(L.EgError, match="BvhFile.format_tracks: frames has 1 entries for 2 recordings"):
        f.format_tracks(e, [3], frame_time=0.1)
    with pytest.raises(L.EgError, match="BvhFile.format_tracks: frame_time=None"):
        f.format_tracks(e)
    with pytest.raises(L.EgError, match=r"BvhFile.format_tracks: root_position shape \(1, 3, 3\): need \[3, 3\] or \[2, 3, 3\]"):
        f.format_tracks(e, frame_time=0.1, root_position=np.zeros((1, 3, 3)))
    with pytest.raises(L.EgError, match="BvhFile.format_tracks: joints: unknown joint name 'Tail'"):
        f.format_tracks(e, joints=["Tail"], frame_time=0.1)
    with pytest.raises(L.EgError, match=r"euler shape \(1, 1, 1, 3, 4, 3\): need \[T, 4, 3\], \[U, T, 4, 3\] or \[U, R, T, 4, 3\]"):
        f.format_tracks(np.zeros((1, 1, 1, 3, 4, 3)), frame_time=0.1)
    wide = BVH.parse(SMALL.replace("OFFSET -8.0 0.0 0.0\n    CHANNELS 3 Xrotation Yrotation Zrotation",
                                   "OFFSET -8.0 1e13 0.0\n    CHANNELS 6 Xposition Yposition Zposition Xrotation Yrotation Zrotation"))
    with pytest.raises(L.EgError, match=r"channel 16: OFFSET 10000000000000.0 is written as 21 bytes \(need 8 .. 18\)"):
        wide.text_table()


def test_text_table_layout():
    f = _file("Yposition Xposition Zrotation Xrotation Yrotation")                   # a root with two position channels
    C_ = f.channels
    assert C_ == 5 + 3 + 6 + 3
    for root in (False, True):
        blob = f.text_table(["Hips", "Leg"], root)
        assert blob.dtype == np.uint8 and len(blob) == 28 * C_ == L.load().eg_bvh_text_table_bytes(C_)
        src, clen = blob[:4 * C_].view(np.int32), blob[4 * C_:8 * C_].view(np.int32)
        text = blob[8 * C_:].reshape(C_, 20)
        const = lambda c: bytes(text[c, :clen[c]]).decode()
        assert list(src[:5]) == ([-2, -1] if root else [-4, -4]) + [0, 1, 2] and list(src[5:8]) == [-4] * 3 and list(src[-3:]) == [3, 4, 5]
        assert [const(c) for c in range(5, 8)] == ["0.000000"] * 3                   # Spine is not kept
        assert [const(c) for c in range(8, 11)] == ["12345.678000", "-3.000000", "0.000000"] and list(src[11:14]) == [-4] * 3
        if not root:
            assert [const(0), const(1)] == ["91.500000", "0.250000"]
    assert bytes(_file().text_table()[8 * 18:].reshape(18, 20)[2, :9]).decode() == "-0.000000"          # the OFFSET of -0.0


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------------------
EULER, ROOTP, D_TABLE, D_FRAMES, WS, LINES, SUMMARY, TEXT = (P(1 << 20), P(1 << 21), P(1 << 14), P(1 << 12), P(1 << 24), P(1 << 25), P(1 << 26),
                                                              P(1 << 27))


def _args(table, **kw):
    base = dict(euler=EULER, root_position=None, table=table.ctypes.data_as(P), d_table=D_TABLE, frames=None, d_frames=None, rows=2, T=20,
                J3=12, C=len(table) // 28, draws=1, frame_unit=1)
    base.update(kw)
    return L.EgBvhTextArgs(**base)


@pytest.mark.parametrize("name", ["eg_bvh_text_measure", "eg_bvh_text_write"])
def test_c_abi_refuses_by_name_before_any_launch(name):
    lib = L.load()
    table = _file().text_table()
    need = lib.eg_bvh_text_workspace_bytes(2, 20, 18)
    assert need > 0 and need % 256 == 0

    def call(args, ws=WS, ws_bytes=need, lines=LINES, summary=SUMMARY, text=TEXT, text_bytes=1 << 20):
        a = args if args is None else C.byref(args)
        rc = lib.eg_bvh_text_measure(a, ws, ws_bytes, lines, summary, None) if name.endswith("measure") else \
            lib.eg_bvh_text_write(a, lines, text, text_bytes, None)
        return rc, lib.eg_last_error().decode()

    full, short = (C.c_int32 * 2)(20, 20), (C.c_int32 * 2)(20, 0)
    rooted = _file().text_table(None, True)
    bad_src, bad_len = table.copy(), table.copy()
    bad_src[:4].view(np.int32)[0] = 12
    bad_len[4 * 18:4 * 18 + 4].view(np.int32)[0] = 19                                # channel 0 is a constant (no root_position)
    cases = [
        (None, EG_ERR_BAD_ARG, "null argument block"),
        (_args(table, euler=None), EG_ERR_BAD_ARG, "null euler, table or d_table"),
        (_args(table, d_table=None), EG_ERR_BAD_ARG, "null euler, table or d_table"),
        (_args(table, euler=P(EULER.value + 2)), EG_ERR_ALIGN, "euler, root_position, table or d_table not 4-byte aligned"),
        (_args(table, rows=0), EG_ERR_BAD_ARG, "rows=0 frames=20 channels=18 (need rows, frames >= 1 and channels in 1..512)"),
        (_args(table, T=0), EG_ERR_BAD_ARG, "rows=2 frames=0 channels=18 (need rows, frames >= 1 and channels in 1..512)"),
        (_args(table, C=513), EG_ERR_BAD_ARG, "rows=2 frames=20 channels=513 (need rows, frames >= 1 and channels in 1..512)"),
        (_args(table, rows=1 << 30, T=1 << 10), EG_ERR_BAD_ARG, f"rows={1 << 30} x frames=1024: grid / index range"),
        (_args(table, J3=0), EG_ERR_BAD_ARG, "J3=0 (need >= 1)"),
        (_args(table, rows=3, draws=2), EG_ERR_BAD_ARG, "rows=3 is not a multiple of draws=2"),
        (_args(table, draws=0), EG_ERR_BAD_ARG, "rows=2 is not a multiple of draws=0"),
        (_args(table, frame_unit=0), EG_ERR_BAD_ARG, "frame_unit=0 (need >= 1)"),
        (_args(table, d_frames=P(D_FRAMES.value + 2), frames=C.cast(full, P)), EG_ERR_ALIGN, "d_frames not 4-byte aligned"),
        (_args(table, frames=C.cast(full, P)), EG_ERR_BAD_ARG, "frames (host) and d_frames (device) go together: the counts are checked on the host copy"),
        (_args(table, d_frames=D_FRAMES), EG_ERR_BAD_ARG, "frames (host) and d_frames (device) go together: the counts are checked on the host copy"),
        (_args(table, d_frames=D_FRAMES, frames=C.cast(short, P)), EG_ERR_BAD_ARG, "recording 1 has 0 valid frames < 1"),
        (_args(bad_src), EG_ERR_BAD_ARG, "src[0]=12 (need -4 .. J3 - 1 = 11)"),
        (_args(rooted), EG_ERR_BAD_ARG, "src[0]=-1 names root_position, which is null"),
        (_args(bad_len), EG_ERR_BAD_ARG, "const_len[0]=19 (need 8 .. 18)"),
    ]
    for args, code, words in cases:
        rc, msg = call(args)
        assert rc == code and msg == f"{name}: {words}", (words, rc, msg)
    ok = _args(table)
    if name.endswith("measure"):
        own = [(dict(ws=None), EG_ERR_BAD_ARG, "null workspace, line_off or summary"), (dict(summary=None), EG_ERR_BAD_ARG, "null workspace, line_off or summary"),
               (dict(lines=P(LINES.value + 4)), EG_ERR_ALIGN, "workspace, line_off or summary not 8-byte aligned"),
               (dict(ws_bytes=need - 1), EG_ERR_WORKSPACE, f"workspace too small ({need - 1} < {need} bytes)")]
    else:
        own = [(dict(text=None), EG_ERR_BAD_ARG, "null line_off or text"), (dict(lines=P(LINES.value + 4)), EG_ERR_ALIGN, "line_off not 8-byte aligned"),
               (dict(text=P(TEXT.value + 8)), EG_ERR_ALIGN, "text not 16-byte aligned"), (dict(text_bytes=0), EG_ERR_BAD_ARG, "text_bytes=0 (need >= 1)")]
    for kw, code, words in own:
        rc, msg = call(ok, **kw)
        assert rc == code and msg == f"{name}: {words}", (words, rc, msg)
    assert lib.eg_bvh_text_workspace_bytes(0, 20, 18) == 0 and lib.eg_bvh_text_workspace_bytes(2, 20, 513) == 0
    assert lib.eg_bvh_text_table_bytes(0) == 0 and lib.eg_bvh_text_table_bytes(513) == 0 and lib.eg_bvh_text_table_bytes(512) == 28 * 512


# ---- format itself -----------------------------------------------------------------------------------------------------------------------------
def _format_as_before(f, euler, joints=None, frame_time=None, root_position=None):
    """BvhFile.format's body as it stood before its channel logic moved into BvhFile._channel_sources."""
    kept = f._rotating(joints, "format")
    e = np.asarray(euler, np.float64)
    T = len(e)
    motion = np.zeros((T, f.channels))
    for nd in f.nodes:
        for i, w in enumerate(nd.channels):
            if w.endswith("position"):
                motion[:, nd.first + i] = nd.offset["XYZ".index(w[0])]
    for jt, nd in enumerate(kept):
        motion[:, nd.rotation_columns] = e[:, jt]
    if root_position is not None:
        rp = np.asarray(root_position, np.float64)
        for axis, c in enumerate(f._root_columns()):
            if c is not None:
                motion[:, c] = rp[:, axis]
    fmt = " ".join(["%.6f"] * f.channels)
    head = f.hierarchy if f.hierarchy.endswith("\n") else f.hierarchy + "\n"
    return head + "MOTION\nFrames: %d\nFrame Time: %.6f\n" % (T, float(frame_time)) + "\n".join(fmt % tuple(row) for row in motion) + "\n"


def test_format_is_unchanged_by_the_shared_channel_helper():
    rng = np.random.default_rng(14)
    for f in (BVH.parse(TEB._motion_text()[0]), BVH.parse(TEB.HIERARCHY), _file(), _file("Yposition Xposition Zrotation Xrotation Yrotation")):
        J = len(f.names)
        for joints in (None, TEB.SUBSET if "Spine1" in f.names or set(TEB.SUBSET) <= set(f.names) else f.names[::2]):
            n = J if joints is None else len(joints)
            for T in (0, 1, 6):
                e = rng.standard_normal((T, n, 3)) * 200
                rp = rng.standard_normal((T, 3)) * 30
                for root in (None, rp):
                    assert f.format(e, joints, 0.0125, root) == _format_as_before(f, e, joints, 0.0125, root)
