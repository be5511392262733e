"""What tests/test_gpu_skeleton.py and tests/test_gpu_rotations.py share: the frame rates and lengths around the tile height, the skeletons by
name, seeded means, and the TED-shaped models and inputs of the caller tests."""
import numpy as np
import torch

import rollout_np as RO
import skeleton_np as SN
from conftest import build_mirror
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.synth import load_synth_weights

TF = SK.TILE_FRAMES
RATES = [(1, 1), (2, 1), (5, 3), (2, 3)]                 # L / M
FPS = {(1, 1): None, (2, 1): (15, 30), (5, 3): (15, 25), (2, 3): (15, 10)}
LENGTHS = [1, 2, TF - 1, TF, TF + 1, 2 * TF + 3]
RAGGED = [1, TF + 1, 2 * TF + 3]
NAMES = ["ted", "chain", "star", "random63"]
F_, D_, P_ = 34, 126, 4
H_ = F_ - P_
HOP, N = 32000, (124 - 1) * 512
_SK = {}
_MODELS = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def skeleton(name):
    if name not in _SK:
        _SK[name] = {"ted": SK.ted_expressive, "chain": lambda: SK.Skeleton(*SN.chain_table()), "star": lambda: SK.Skeleton(*SN.star_table()),
                     "random63": lambda: SK.Skeleton(*SN.random_table())}[name]()
    return _SK[name]


def table_of(sk):
    return sk.parents.tolist(), sk.children.tolist(), sk.lengths.tolist()


def mean_of(K, seed):
    return (np.random.default_rng(seed).standard_normal(3 * K) * 0.2).astype(np.float32)


def ted_models():
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    if "ted" not in _MODELS:
        _MODELS["ted"] = (build_mirror("spatial", F_, D_, P_, 4, seed=7, precision="bf16x3").to(dev()),
                          load_synth_weights(MLP_Reconstruct_v3(frames=F_), 7).eval().to(dev()))
    return _MODELS["ted"]


def inputs(U, W, seed):
    inp = RO.rollout_inputs(U, W, F_, D_, P_, seed=seed)
    return {k: torch.from_numpy(inp[k]).to(dev()) for k in ("text", "seed_pose", "label", "z")}
