#!/usr/bin/env python3
"""Generate tests/golden/jointscore.npz by running the REFERENCE's SRGR and L1div (model/Beat_score_v2.py) on hashed inputs, in float64.

Build container only (needs /root/reference):   python tests/golden/make_golden_jointscore.py

What runs from the reference, in place: SRGR.run / SRGR.avg and L1div.run / L1div.avg.  Stand-ins for modules that file imports and these
classes never touch: librosa, librosa.display, matplotlib, matplotlib.pyplot.  The file holds inputs and outputs only.

The mask.  SRGR.run returns a rate, not its mask, so the mask is taken from the reference one cell at a time: SRGR(threshold, joints=1).run on
frame t, joint j alone with the weight 0.165 returns 1 (rounded) for a hit and 0 for a miss.  The reference subtracts in float64, the library
in fp32: with coordinates within +-1.1 the three fp32 subtractions differ from the float64 ones by less than 3 * 2^-23 ~ 3.6e-7 in all, so
with every |d - threshold| > 1e-6 -- asserted here over every input -- the two masks must be identical, no cell left out.

One SRGR object pools the four shapes as a data set is pooled upstream; its joint count (`pose_dimes`) is set to each shape's J before the
run.  The archive is written with fixed zip time stamps, so the script regenerates it byte for byte.
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"

from emotiongestures_amd.synth import hash_unit  # noqa: E402

SHAPES = ((37, 47), (5, 1), (70, 43), (9, 64))
THRESHOLD = 0.1


def inputs(n, J):
    """target, result [n, J, 3] and semantic [n], fp32."""
    h = lambda tag, count, seed: hash_unit(tag, count, seed).astype(np.float64)
    target = ((h("jointscore.target", n * J * 3, 11) - 0.5) * 2).astype(np.float32)
    result = (target.astype(np.float64) + (h("jointscore.offset", n * J * 3, 12) - 0.5) * 0.14).astype(np.float32)
    semantic = hash_unit("jointscore.sem", n, 13).astype(np.float32)
    semantic[::3] = 0
    return target.reshape(n, J, 3), result.reshape(n, J, 3), semantic


def save(path, arrays):
    """An .npz with fixed time stamps (np.savez stamps every member with the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            z.writestr(info, buf.getvalue())


def main():
    for name in ("librosa", "librosa.display", "matplotlib", "matplotlib.pyplot"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["librosa"].display = sys.modules["librosa.display"]
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["matplotlib.pyplot"].figure = None
    spec = importlib.util.spec_from_file_location("reference_beat_score_v2", os.path.join(REF, "model", "Beat_score_v2.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)

    out = {"shapes": np.asarray(SHAPES, np.int64), "threshold": np.float64(THRESHOLD)}
    pool_s, pool_l = B.SRGR(threshold=THRESHOLD), B.L1div()
    margin, share = np.inf, []
    for n, J in SHAPES:
        target, result, semantic = inputs(n, J)
        tag = f"{n}x{J}"
        assert np.abs(target).max() <= 1.1 and np.abs(result).max() <= 1.1
        r64, g64, s64 = result.astype(np.float64), target.astype(np.float64), semantic.astype(np.float64)
        margin = min(margin, float(np.abs(np.abs(r64 - g64).sum(2) - THRESHOLD).min()))
        cell = B.SRGR(threshold=THRESHOLD, joints=1)
        mask = np.zeros((n, J), np.uint8)
        for t in range(n):
            for j in range(J):
                mask[t, j] = round(cell.run(r64[t, j].copy(), g64[t, j].copy(), np.array([0.165])))
        one = B.SRGR(threshold=THRESHOLD, joints=J)
        rate = one.run(r64.reshape(n, J * 3).copy(), g64.reshape(n, J * 3).copy(), s64.copy())
        pool_s.pose_dimes = J
        assert pool_s.run(r64.reshape(n, J * 3).copy(), g64.reshape(n, J * 3).copy(), s64.copy()) == rate
        l1 = B.L1div()
        l1.run(r64.reshape(n, J * 3).copy())
        pool_l.run(r64.reshape(n, J * 3).copy())
        assert l1.counter == n
        share.append(float(mask.mean()))
        out.update({f"{tag}/target": target, f"{tag}/result": result, f"{tag}/semantic": semantic, f"{tag}/mask": mask,
                    f"{tag}/rate": np.float64(rate), f"{tag}/l1_sum": np.float64(l1.sum), f"{tag}/l1div": np.float64(l1.avg())})
    assert margin > 1e-6, margin
    out.update({"pool/srgr_sum": np.float64(pool_s.sum), "pool/srgr_counter": np.int64(pool_s.counter), "pool/srgr_avg": np.float64(pool_s.avg()),
                "pool/l1_sum": np.float64(pool_l.sum), "pool/l1_counter": np.int64(pool_l.counter), "pool/l1_avg": np.float64(pool_l.avg()),
                "margin": np.float64(margin)})
    path = os.path.join(ROOT, "tests", "golden", "jointscore.npz")
    save(path, out)
    print("wrote", path, os.path.getsize(path), f"bytes; smallest |d - threshold| {margin:.3e}; share of hits per shape", share)


if __name__ == "__main__":
    main()
