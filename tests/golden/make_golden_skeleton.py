#!/usr/bin/env python3
"""Generate tests/golden/skeleton.npz by running the REFERENCE's skeleton conversions on hashed inputs.

Build container only (needs /root/reference):   python tests/golden/make_golden_skeleton.py

What runs from the reference, in place: utils.data_utils_expressive.convert_dir_vec_to_pose and convert_pose_seq_to_dir_vec.  Stand-ins for
modules that are absent here and unused by those functions: librosa, librosa.display.  The file holds inputs and outputs only -- no table of the
reference: the 42 one-bone inputs (bone k = (1, 0, 0), every other bone zero) pin the topology and every length of
emotiongestures_amd.skeleton.ted_expressive() through behaviour.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"

from emotiongestures_amd.synth import hash_unit  # noqa: E402


def main():
    for name in ("librosa", "librosa.display"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["librosa"].display = sys.modules["librosa.display"]
    sys.path.insert(0, REF)
    os.chdir(REF)
    import utils.data_utils_expressive as U

    out = {}
    v4 = hash_unit("skeleton.vec4", 2 * 5 * 126, 5).reshape(2, 5, 126) - 0.5
    v3 = hash_unit("skeleton.vec3", 5 * 126, 6).reshape(5, 126) - 0.5
    v2 = hash_unit("skeleton.vec2", 126, 7) - 0.5
    for tag, v in (("4d", v4), ("3d", v3), ("2d", v2)):
        out[f"vec_{tag}"] = v
        out[f"pose_{tag}"] = U.convert_dir_vec_to_pose(v)
        assert out[f"pose_{tag}"].dtype == np.float64
    one = np.zeros((42, 126))
    one[np.arange(42), 3 * np.arange(42)] = 1.0
    out["vec_one_bone"] = one
    out["pose_one_bone"] = U.convert_dir_vec_to_pose(one)
    # the inverse, from the 3-D and 4-D poses above: a torch fp32 tensor upstream
    out["dir_vec_3d"] = U.convert_pose_seq_to_dir_vec(out["pose_3d"]).numpy()
    out["dir_vec_4d"] = U.convert_pose_seq_to_dir_vec(out["pose_4d"]).numpy()
    assert out["dir_vec_3d"].dtype == np.float32 and out["dir_vec_4d"].shape == (2, 5, 42, 3)
    path = os.path.join(ROOT, "tests", "golden", "skeleton.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; pose_4d", out["pose_4d"].shape, out["pose_4d"].dtype)


if __name__ == "__main__":
    main()
