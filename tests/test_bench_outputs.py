"""bench.py's plain run (headline only; everything else behind --full) and --dump-outputs (the last timed step's 5-tuple as .npy files)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_switches_every_extra_off(monkeypatch):
    a = _args(monkeypatch, "--steps", "7", "--warmup", "2")
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert a.no_extra_legs and a.no_roofline and a.no_cpu_baseline and a.no_train_legs
    f = _args(monkeypatch, "--full")
    assert f.full and not (f.no_extra_legs or f.no_roofline or f.no_cpu_baseline or f.no_train_legs)
    assert _args(monkeypatch, "--full", "--no-roofline").no_roofline


def test_dump_outputs_writes_float32_and_samples_past_the_limit(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(0)
    outs = [torch.rand(10, 3, 5, generator=g), torch.rand(10, 4, generator=g), torch.rand(10, 2, generator=g, dtype=torch.float64),
            torch.rand(10, 8, generator=g), torch.rand(10, 6, generator=g)]
    bench.dump_outputs(str(tmp_path / "all"), outs)
    for name, o in zip(bench.OUTPUT_NAMES, outs):
        a = np.load(tmp_path / "all" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, o.float().numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)      # 4 * 10 * 35 = 1400 bytes in all -> 7 of the 10 clips
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), outs)
    got = [np.load(tmp_path / "s1" / f"{n}.npy") for n in bench.OUTPUT_NAMES]
    assert sum(a.nbytes for a in got) <= 1000 and got[0].shape == (7, 3, 5)
    rows = [i for i in range(10) if any(np.array_equal(outs[0][i].numpy(), r) for r in got[0])]
    assert len(rows) == 7
    for o, a in zip(outs, got):                               # the same clips from every array
        assert np.array_equal(a, o[rows].float().numpy())
    for n in bench.OUTPUT_NAMES:                              # the sample is fixed
        assert np.array_equal(np.load(tmp_path / "s1" / f"{n}.npy"), np.load(tmp_path / "s2" / f"{n}.npy"))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs_match_the_oracle(tmp_path):
    """A plain run prints the headline alone (no parity, legs, roofline or CPU baseline) and --dump-outputs writes what the timed step returned:
    its pose agrees with the CPU oracle on the same seeded clips."""
    from emotiongestures_amd.builders import build_mirror, clip_rel_l2
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.synth import load_synth_weights
    from oracle import emogest_oracle as O
    B = 4
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--batch", str(B), "--steps", "3", "--warmup", "1", "--in-flight", "2",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "bf16x3" and line["higher_is_better"] is True
    for k in ("pose_rel_l2_vs_cpu_oracle", "fgd_vs_cpu_oracle", "sustained", "f32", "train", "roofline", "cpu_baseline"):
        assert line[k] is None, k
    assert line["extra_legs"] == {}
    outs = {n: np.load(tmp_path / f"{n}.npy") for n in bench.OUTPUT_NAMES}
    assert outs["pose"].shape == (B, 34, 126) and outs["emo_pred"].shape == (B, 8)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in outs.values())
    sd_g = build_mirror("spatial", 34, 126, 4, 4, seed=0, precision="bf16x3").state_dict()           # bench.build_models' weights
    sd_v = load_synth_weights(MLP_Reconstruct_v3(frames=34), 0).eval().state_dict()
    inp = bench.make_inputs(B, seed=1000)
    with torch.no_grad():
        t = {k: torch.from_numpy(v) for k, v in inp.items() if k != "audio"}
        spec = torch.from_numpy(O.melspectrogram(inp["audio"], out_frames=124))
        ref = O.generator_forward(sd_g, O.GenCfg(), spec, t["text"], t["pre_pose"], O.cvae_sample(sd_v, t["label"], t["z"]))[0]
    assert clip_rel_l2(outs["pose"], ref.numpy()) < 1e-3
