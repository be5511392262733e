"""CPU side of the audio tower's site tests: the float64 restatement of tests/tower_f64.py against the golden the reference's own modules wrote
(tests/golden/make_golden_tower_grad.py), and the comparison helper against deliberate mutations of a float64 gradient.  No GPU."""
import os

import numpy as np
import pytest
import torch

import tower_f64 as T64
from conftest import GOLDEN
from emotiongestures_amd.builders import build_mirror

SITES = ["stem"] + [f"layer1.{i}" for i in range(3)] + [f"layer2.{i}" for i in range(4)] + [f"layer3.{i}" for i in range(6)] + ["final"]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "tower_grads.npz"))
    _batch, seed = [int(v) for v in z["meta"]]
    sd = {k: v.detach().clone() for k, v in build_mirror("spatial", 34, 126, 4, 4, seed=seed).state_dict().items()}
    return z, sd


def _site(z, sd, site, masks=None):
    x = torch.from_numpy(z[f"{site}/x"].astype(np.float64))
    g = torch.from_numpy(z[f"{site}/g"].astype(np.float64)) / float(z[f"{site}/g_scale"])
    params, running = T64.site_state(sd, site)
    stride = 1 if site in ("stem", "final") else int(z[f"{site}/stride"])
    return T64.run_site(site, params, running, x, g, stride, masks)


def _fingerprint_errors(z, key, t):
    """(sample, norm, sum) errors of t against the golden fingerprint; the sum relative to ||ref|| sqrt(n), the bound of |sum| by Cauchy-Schwarz."""
    v = t.detach().reshape(-1).double().numpy()
    stride = max(1, v.size // 64)
    ref_s, ref_n, ref_sum = z[key + "/sample"], float(z[key + "/norm"]), float(z[key + "/sum"])
    assert v[::stride][:64].shape == ref_s.shape, key
    e_s = np.linalg.norm(v[::stride][:64] - ref_s) / max(np.linalg.norm(ref_s), 1e-300)
    e_n = abs(np.linalg.norm(v) - ref_n) / max(ref_n, 1e-300)
    e_sum = abs(v.sum() - ref_sum) / max(ref_n * np.sqrt(v.size), 1e-300)
    return e_s, e_n, e_sum


@pytest.mark.parametrize("site", SITES)
def test_float64_restatement_reproduces_the_reference_golden(golden, site):
    """Every fingerprint the golden holds for the site (output, input gradient, every parameter gradient: 64-value sample, L2 norm AND sum) to
    1e-10, and the ReLU masks (conv1's and the block's last) bit for bit: ties tower_f64.run_site to the reference's own modules."""
    z, sd = golden
    r = _site(z, sd, site)
    keys = {"out": r["out"], "dx": r["dx"]}
    keys.update({f"p/{k}": t for k, t in r["grads"].items()})
    seen = 0
    for k, t in keys.items():
        key = f"{site}/{k}"
        if key + "/norm" not in z.files:
            continue
        seen += 1
        if k == "p/final_conv1.bias":               # exactly zero in exact arithmetic (a bias in front of a train-mode BatchNorm): round-off on both sides
            assert float(t.norm()) < 1e-12 * float(z[f"{site}/p/final_conv1.weight/norm"]) and float(z[key + "/norm"]) < 1e-12 * float(z[f"{site}/p/final_conv1.weight/norm"])
            continue
        e = _fingerprint_errors(z, key, t)
        assert max(e) <= 1e-10, f"{key}: sample {e[0]:.1e}, norm {e[1]:.1e}, sum {e[2]:.1e}"
    assert seen == len(keys), f"{site}: {len(keys) - seen} tensors without a golden fingerprint"
    for k in ("r1", "out"):
        if f"{site}/mask/{k}" in z.files:
            mine = r["masks"][k].numpy().reshape(-1)
            ref = np.unpackbits(z[f"{site}/mask/{k}"])[:mine.size].astype(bool)
            assert np.array_equal(mine, ref), f"{site}: {int((mine != ref).sum())} elements of the {k} mask differ"
    assert len(r["masks"]) == sum(f"{site}/mask/{k}" in z.files for k in ("r1", "out"))


def test_running_statistics_follow_nn_batchnorm(golden):
    """The running buffers run_site returns are nn.BatchNorm2d's update (momentum 0.1, unbiased batch variance)."""
    z, sd = golden
    r = _site(z, sd, "layer2.0")
    params, running = T64.site_state(sd, "layer2.0")
    x = torch.from_numpy(z["layer2.0/x"].astype(np.float64))
    c1 = torch.relu(torch.nn.functional.conv2d(x, params["conv1.weight"].detach(), None, stride=2, padding=1))
    bn = torch.nn.BatchNorm2d(c1.shape[1], momentum=0.1).double().train()
    bn.running_mean.copy_(running["bn1"][0])
    bn.running_var.copy_(running["bn1"][1])
    bn(c1)
    assert torch.allclose(r["running"]["bn1"][0], bn.running_mean, rtol=1e-12, atol=1e-15)
    assert torch.allclose(r["running"]["bn1"][1], bn.running_var, rtol=1e-12, atol=1e-15)
    assert set(r["running"]) == {"bn1", "bn2", "downsample.1"}


def test_comparison_helper_rejects_localised_errors_the_fingerprint_accepts(golden):
    """Each mutation of a float64 gradient fails tower_f64.compare under the loosest (split-bf16) bounds: a kh <-> kw transposition of a 3x3
    weight gradient, a 1 % error on one output channel, a 1 % error on the last column of a map, one 32-column tile scaled by 1.01.  The golden
    fingerprint check accepts the transposition: its 64-value sample sees tap (0, 0) only and the norm is unchanged."""
    z, sd = golden
    site = "layer2.1"
    r = _site(z, sd, site)
    B = T64.BOUNDS["bf16x3"]
    dw, dx = r["grads"]["conv1.weight"], r["dx"]
    T64.compare(dw, dw, B, "unmutated weight gradient")
    T64.compare(dx, dx, B, "unmutated input gradient")
    tr = dw.transpose(2, 3).contiguous()
    assert not torch.equal(tr, dw)
    T64.fp_check(z, f"{site}/p/conv1.weight", tr, 1e-4, "transposed dconv1 (fingerprint)")          # accepted
    ch = dw.clone()
    ch[dw.shape[0] // 2] *= 1.01
    col = dx.clone()
    col[..., -1] *= 1.01
    tile = dx.clone()
    tile[..., T64.TILE_W:2 * T64.TILE_W] *= 1.01
    assert dx.shape[-1] > T64.TILE_W
    for what, got, ref in (("kh <-> kw transposition", tr, dw), ("1 % on one output channel", ch, dw), ("1 % on the last column", col, dx),
                           ("one 32-column tile x 1.01", tile, dx)):
        with pytest.raises(AssertionError):
            T64.compare(got, ref, B, what)
        whole, (sl, where), elem = T64.errors(got, ref)
        assert sl > B["slice"], (what, whole, sl, where, elem)                                       # the slice check alone catches it


def test_forced_masks_follow_the_given_decisions(golden):
    """run_site(masks=...) applies the given ReLU decisions (a GPU forward's) instead of its own; check_flips counts the difference and holds the
    flipped pre-activations to rounding size."""
    z, sd = golden
    site = "layer1.1"
    r = _site(z, sd, site)
    m = {k: v.clone() for k, v in r["masks"].items()}
    pre = r["pre"]["r1"]
    i = int(pre.abs().reshape(-1).argmin())                      # the element nearest to zero: flip it
    m["r1"].view(-1)[i] = ~m["r1"].view(-1)[i]
    f = _site(z, sd, site, masks=m)
    assert torch.equal(f["masks"]["r1"], m["r1"]) and torch.equal(f["masks"]["out"], m["out"])
    assert T64.check_flips(f["pre"]["r1"], m["r1"], 1e-5, site) == 1
    far = m["r1"].clone()
    j = int(pre.abs().reshape(-1).argmax())
    far.view(-1)[j] = ~far.view(-1)[j]
    with pytest.raises(AssertionError):
        T64.check_flips(pre, far, 1e-5, site)
