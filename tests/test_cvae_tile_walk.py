"""The halo index arithmetic of the fused CVAE sample kernel, checked without a GPU: tools/cvae_tile_walk.py restates the kernel's tiled walk
(buffer extents, start positions, zero padding outside the axis) in float64 numpy, and it must reproduce the layer-by-layer evaluation,
which in turn is oracle.cvae_sample.  This checks the arithmetic of the walk as restated there (extents n0..n4, start
positions, zero padding), not the kernel: what binds the kernel to it is tests/test_gpu_cvae_fused.py, bit for bit against the launch chain."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("cvae_tile_walk", os.path.join(ROOT, "tools", "cvae_tile_walk.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

TOL = 1e-12         # float64, a few hundred terms of size <= 1 per element, only their grouping differs


@pytest.mark.parametrize("n,F,D,T,big_bias", [
    (1, 34, 512, 128, False),       # four full tiles: l0 = 0, interior, last
    (1, 60, 192, 128, False),       # the last tile is partial
    (2, 34, 64, 64, False),         # one tile, z0 only 16 positions long
    (1, 34, 64, 128, False),        # the tile is longer than the axis
    (1, 34, 192, 64, False),        # three short tiles
    (1, 34, 192, 128, True),        # large biases: a halo position outside the axis that is not stored as zero shows
])
def test_tiled_walk_equals_the_layered_evaluation(n, F, D, T, big_bias):
    layered, tiled = W.case(n, F, D, T, big_bias=big_bias)
    assert np.isfinite(tiled).all()
    assert np.abs(tiled - layered).max() <= TOL * max(1.0, np.abs(layered).max())


def test_layered_evaluation_is_the_oracle():
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.synth import load_synth_weights, synth_inputs
    from oracle import emogest_oracle as O
    vae = load_synth_weights(MLP_Reconstruct_v3(frames=34), 4).eval()
    sd = {k: v.detach().double() for k, v in vae.state_dict().items()}
    inp = synth_inputs(2, 34, seed=4)
    y, z = torch.from_numpy(inp["label"]).double(), torch.from_numpy(inp["z"]).double()
    with torch.no_grad():
        want = O.cvae_sample(sd, y, z).numpy()
    got = W.layered({k: v.numpy() for k, v in sd.items()}, y.numpy(), z.numpy())
    assert np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max())
