"""The rows contract of the whole-track stages (include/emogest.h, "Rows of whole tracks"; csrc/rows.h), over every entry point that takes
(d_frames, draws, frame_unit): the same refusals in the same words.  No GPU here and none needed: every refusal returns before the first
launch, so the fake (aligned) addresses are never touched."""
import ctypes as C

import pytest

from emotiongestures_amd import _lib as L

P = C.c_void_p
ROWS, T = 2, 20
X, OUT, OUT2, TABLE, D_FRAMES, WS = (P(1 << 20), P(1 << 22), P(1 << 23), P(1 << 14), P(1 << 12), P(1 << 24))
K_SMOOTH = 5
EG_ERR_BAD_ARG, EG_ERR_ALIGN = -1, -5         # include/emogest.h: EgStatus

# a three-bone chain, a two-joint body and their host tables (checked on the host before the rows are)
PARENTS, CHILDREN = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 3)(1, 2, 3)
LENGTHS = (C.c_float * 3)(1.0, 1.0, 1.0)
REST = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
BODY_PARENTS, BODY_OFFSETS, ORDERS = (C.c_int32 * 2)(-1, 0), (C.c_float * 6)(), (C.c_int32 * 2)(0, 0)


def _calls(lib):
    """name -> (call(rows, frames, d_frames, draws, frame_unit) -> rc, the minimum of valid frames or None without a host copy, its words)"""
    return {
        "eg_skeleton_joints": (lambda rows, fr, d, draws, unit: lib.eg_skeleton_joints(
            X, rows, T, PARENTS, CHILDREN, LENGTHS, 3, TABLE, d, draws, unit, None, 0, 1, 1, OUT, T, None), None, None),
        "eg_skeleton_dir_vec": (lambda rows, fr, d, draws, unit: lib.eg_skeleton_dir_vec(
            X, rows, T, PARENTS, CHILDREN, LENGTHS, 3, TABLE, d, draws, unit, None, OUT, None), None, None),
        "eg_skeleton_rotations": (lambda rows, fr, d, draws, unit: lib.eg_skeleton_rotations(
            X, rows, T, PARENTS, CHILDREN, LENGTHS, 3, REST, TABLE, d, draws, unit, None, 0, 1, 1, OUT, T, None), None, None),
        "eg_articulate_forward": (lambda rows, fr, d, draws, unit: lib.eg_articulate_forward(
            X, rows, T, BODY_PARENTS, BODY_OFFSETS, 2, TABLE, d, draws, unit, None, 0, 0, 1, 1, OUT, OUT2, T, None), None, None),
        "eg_articulate_rot6d": (lambda rows, fr, d, draws, unit: lib.eg_articulate_rot6d(X, rows, T, 2, d, draws, unit, None, 0, OUT, None),
                                None, None),
        "eg_articulate_euler": (lambda rows, fr, d, draws, unit: lib.eg_articulate_euler(
            X, rows, T, 2, ORDERS, TABLE, d, draws, unit, None, 0, 1, 1, 1, OUT, T, None), None, None),
        "eg_articulate_rot6d_euler": (lambda rows, fr, d, draws, unit: lib.eg_articulate_rot6d_euler(
            X, rows, T, 2, ORDERS, TABLE, d, draws, unit, None, 0, 1, OUT, None), None, None),
        "eg_angle_unwrap": (lambda rows, fr, d, draws, unit: lib.eg_angle_unwrap(X, rows, T, 6, d, draws, unit, 360.0, None, 0, None), None, None),
        "eg_smooth_tracks": (lambda rows, fr, d, draws, unit: lib.eg_smooth_tracks(X, rows, T, 5, K_SMOOTH, TABLE, fr, d, draws, unit, OUT, None),
                             K_SMOOTH, f"window={K_SMOOTH} (there is no shrinking window)"),
        "eg_kin_stats": (lambda rows, fr, d, draws, unit: lib.eg_kin_stats(
            X, rows, T, 3, fr, d, draws, unit, 15.0, TABLE, 4, WS, 1 << 20, OUT, OUT2, None), 4, "4 (the jerk reads four positions)"),
        "eg_srgr_tracks": (lambda rows, fr, d, draws, unit: lib.eg_srgr_tracks(
            X, OUT, None, rows, T, 3, fr, d, draws, unit, 0.1, 1.0, WS, 1 << 20, P(1 << 26), P(1 << 27), P(1 << 28), None), 1, "1"),
        "eg_l1div_tracks": (lambda rows, fr, d, draws, unit: lib.eg_l1div_tracks(
            X, rows, T, 9, fr, d, draws, unit, WS, 1 << 20, P(1 << 26), P(1 << 27), P(1 << 28), None), 1, "1"),
    }


NAMES = sorted(_calls(None))


@pytest.mark.parametrize("name", NAMES)
def test_rows_refusals_same_words_everywhere(name):
    lib = L.load()
    call, min_frames, why = _calls(lib)[name]
    full = (C.c_int32 * 1)(T)

    def refused(rows=ROWS, fr=None, d=None, draws=1, unit=1):
        rc = call(rows, fr, d, draws, unit)
        return rc, lib.eg_last_error().decode()

    off_by_2 = dict(d=P(D_FRAMES.value + 2), fr=full if min_frames is not None else None, draws=2)
    for kw, code, text in [(dict(rows=3, draws=2), EG_ERR_BAD_ARG, f"{name}: rows=3 is not a multiple of draws=2"),
                           (dict(draws=0), EG_ERR_BAD_ARG, f"{name}: rows=2 is not a multiple of draws=0"),
                           (dict(unit=0), EG_ERR_BAD_ARG, f"{name}: frame_unit=0 (need >= 1)"),
                           (off_by_2, EG_ERR_ALIGN, f"{name}: d_frames not 4-byte aligned")]:
        rc, msg = refused(**kw)
        assert rc == code and msg == text, (kw, rc, msg)
    if min_frames is None:
        return
    together = f"{name}: frames (host) and d_frames (device) go together: the counts are checked on the host copy"
    short = (C.c_int32 * 2)(T, min_frames - 1)
    for kw, text in [(dict(fr=short), together), (dict(d=D_FRAMES), together),
                     (dict(fr=short, d=D_FRAMES), f"{name}: recording 1 has {min_frames - 1} valid frames < {why}")]:
        rc, msg = refused(**kw)
        assert rc == EG_ERR_BAD_ARG and msg == text, (kw, rc, msg)
    # the count is frames[u] * frame_unit clamped to [0, T]: a stream's 0 / 1 flags with frame_unit = T
    flags = (C.c_int32 * 2)(1, 0)
    rc, msg = refused(fr=flags, d=D_FRAMES, unit=T)
    assert rc == EG_ERR_BAD_ARG and msg == f"{name}: recording 1 has 0 valid frames < {why}", (rc, msg)


def test_every_entry_point_with_rows_arguments_is_in_the_table():
    """The header is the list: a prototype that takes (d_frames, draws, frame_unit) belongs in the table above."""
    import os
    import re
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "emogest.h")).read()
    protos = re.findall(r"^int (eg_\w+)\(([^;]*)\);", header, re.M | re.S)
    have = sorted(n for n, args in protos if re.search(r"d_frames,\s*int32_t draws,\s*int32_t frame_unit", args))
    assert have == NAMES
