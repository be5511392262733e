"""Text branch end to end (TextEncoderTCN: embedding -> 3 TCN levels -> fc1 over time -> decoder) in bf16x3: the one-launch causal products on images
(default) and the two-launch fp32-input path (EG_TEXT_TAPS=2, read per call) against a float64 evaluation of the same module on the CPU."""
import numpy as np
import pytest
import torch

from conftest import build_mirror, rel_l2
from emotiongestures_amd.synth import synth_inputs

pytestmark = pytest.mark.gpu


def test_text_embedding_one_launch_vs_two_launches_vs_fp64(monkeypatch):
    """B = 3 clips of 60 words (180 rows: partial last tile, tile boundaries inside clips), 200 words, 3 levels.  Only `text_embedding` depends on
    the text branch.  The new path's error against float64 may be at most twice the old path's (the K chain is reordered, not lengthened)."""
    from oracle import emogest_oracle as O
    dev = torch.device("cuda:0")
    B = 3
    inp = synth_inputs(B, 34, 126, 4, seed=11)
    gen = build_mirror("spatial", 34, 126, 4, 4, n_words=200, seed=11, precision="bf16x3")
    sd64 = {k: v.detach().clone().double() for k, v in gen.state_dict().items() if k.startswith("text_encoder.")}
    with torch.no_grad():
        ref = O.text_encoder_tcn(sd64, "text_encoder", torch.from_numpy(inp["text"]), O.GenCfg()).numpy()
    gen.to(dev)
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    outs = {}
    for taps in ("1", "2"):
        monkeypatch.setenv("EG_TEXT_TAPS", taps)
        with torch.no_grad():
            res = gen(t["spec"], t["text"], t["pre_pose"], t["sampled"])
        torch.cuda.synchronize()
        outs[taps] = [r.cpu().numpy() for r in res]
    monkeypatch.delenv("EG_TEXT_TAPS")
    assert ref.shape == outs["1"][4].shape
    e_new, e_old = rel_l2(outs["1"][4], ref), rel_l2(outs["2"][4], ref)
    print(f"text_embedding rel-L2 vs float64: one launch per conv {e_new:.3e}, two launches {e_old:.3e}; "
          f"max|d| {np.abs(outs['1'][4] - ref).max():.3e} / {np.abs(outs['2'][4] - ref).max():.3e}")
    assert np.isfinite(outs["1"][4]).all()
    assert e_new <= 2 * e_old
    for i in range(4):          # pose, emotion / semantic feature, emotion prediction: nothing downstream of the text branch
        assert np.array_equal(outs["1"][i], outs["2"][i])
