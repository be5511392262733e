#!/usr/bin/env python3
"""The tiled halo walk of cvae_sample_fused_kernel (csrc/misc.hip), restated in numpy float64 with the kernel's buffer extents and
index arithmetic, so that the walk can be checked on a CPU against the plain layer-by-layer evaluation (tests/test_cvae_tile_walk.py).

    python3 tools/cvae_tile_walk.py            # the shapes of tests/test_gpu_cvae_fused.py, a few tiles each
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _post(s, sd, p):
    """LeakyReLU(0.2), then the BatchNorm affine of eval mode."""
    s = np.where(s > 0, s, 0.2 * s)
    scale = sd[p + ".weight"] / np.sqrt(sd[p + ".running_var"] + 1e-5)
    return s * scale[:, None] + (sd[p + ".bias"] - sd[p + ".running_mean"] * scale)[:, None]


def _lin(sd, p, x):
    return x @ sd[p + ".weight"].T + sd[p + ".bias"]


def layered(sd, y, z):
    """sample() layer by layer on whole rows (the launch chain's data flow), any d_model."""
    n = y.shape[0]
    zy = np.concatenate([z, _lin(sd, "Posterior_Y_embedding.2", _lin(sd, "Posterior_Y_embedding.0", y))], 1)
    x = _lin(sd, "fusion_z_posterior.2", _lin(sd, "fusion_z_posterior.0", zy)).reshape(n, 4, -1)
    for idx in (0, 3):
        w, b = sd[f"Decoder.{idx}.weight"], sd[f"Decoder.{idx}.bias"]          # [Cin][Cout][3]
        lin = x.shape[2]
        out = np.tile(b[None, :, None], (n, 1, 2 * lin))
        for lo in range(2 * lin):
            for k in range(3):
                t = lo + 1 - k
                if t >= 0 and t % 2 == 0 and t // 2 < lin:
                    out[:, :, lo] += x[:, :, t // 2] @ w[:, :, k]
        x = np.stack([_post(o, sd, f"Decoder.{idx + 2}") for o in out])
    for idx in (6, 9, 12):
        w, b = sd[f"Decoder.{idx}.weight"], sd[f"Decoder.{idx}.bias"]          # [Cout][Cin][3]
        xp = np.pad(x, ((0, 0), (0, 0), (1, 1)))
        out = b[None, :, None] + sum(np.einsum("oc,ncl->nol", w[:, :, k], xp[:, :, k:k + x.shape[2]]) for k in range(3))
        x = out if idx == 12 else np.stack([_post(o, sd, f"Decoder.{idx + 2}") for o in out])
    return x


def _convt_stage(xin, w, b, sd, bn, nout, pos0, lout):
    """xin [Cin][nin] at positions p.., yout [Cout][nout] at 2p..: a 'lane' j owns input j and outputs 2j, 2j + 1."""
    cout = w.shape[1]
    y = np.zeros((cout, nout))
    for j in range(nout // 2):
        e = b + xin[:, j] @ w[:, :, 1]
        o = b + xin[:, j + 1] @ w[:, :, 0] + xin[:, j] @ w[:, :, 2]
        pair = _post(np.stack([e, o], 1), sd, bn)
        for r in range(2):
            pos = pos0 + 2 * j + r
            y[:, 2 * j + r] = pair[:, r] if 0 <= pos < lout else 0.0
    return y


def _conv_stage(xin, xoff, w, b, sd, bn, nout, pos0, L):
    y = np.zeros((w.shape[0], nout))
    for p in range(nout):
        s = b + sum(w[:, :, k] @ xin[:, xoff + p + k] for k in range(3))
        if bn is not None:
            s = _post(s[:, None], sd, bn)[:, 0]
            s = s if 0 <= pos0 + p < L else 0.0
        y[:, p] = s
    return y


def tiled(sd, y, z, T, tiles=None):
    """sample() by the kernel's walk: one (sample, tile) at a time through buffers of the kernel's extents.  `tiles`: tile indices to
    evaluate (default all); columns of tiles left out stay NaN."""
    n, L = y.shape[0], sd["fusion_z_posterior.2.weight"].shape[0]
    F = sd["Decoder.12.bias"].shape[0]
    assert T % 4 == 0 and L % 4 == 0
    Q = L // 4
    n0, n1, n2, n3, n4 = T // 4 + 4, T // 2 + 6, T + 8, T + 4, T + 2
    out = np.full((n, F, L), np.nan)
    for s in range(n):
        zy = np.concatenate([z[s], _lin(sd, "Posterior_Y_embedding.2", _lin(sd, "Posterior_Y_embedding.0", y[s]))])
        fz_h = _lin(sd, "fusion_z_posterior.0", zy)
        for tile in (range(-(-L // T)) if tiles is None else tiles):
            l0 = tile * T
            q0 = l0 // 4 - 1
            z0 = np.zeros((4, n0))
            for c in range(4):
                for j in range(n0):
                    q = q0 + j
                    if 0 <= q < Q:
                        row = c * Q + q
                        z0[c, j] = sd["fusion_z_posterior.2.weight"][row] @ fz_h + sd["fusion_z_posterior.2.bias"][row]
            d1 = _convt_stage(z0, sd["Decoder.0.weight"], sd["Decoder.0.bias"], sd, "Decoder.2", n1, l0 // 2 - 2, L // 2)
            d2 = _convt_stage(d1, sd["Decoder.3.weight"], sd["Decoder.3.bias"], sd, "Decoder.5", n2, l0 - 4, L)
            d3 = _conv_stage(d2, 1, sd["Decoder.6.weight"], sd["Decoder.6.bias"], sd, "Decoder.8", n3, l0 - 2, L)
            d4 = _conv_stage(d3, 0, sd["Decoder.9.weight"], sd["Decoder.9.bias"], sd, "Decoder.11", n4, l0 - 1, L)
            o = _conv_stage(d4, 0, sd["Decoder.12.weight"], sd["Decoder.12.bias"], sd, None, T, l0, L)
            hi = min(l0 + T, L)
            out[s, :, l0:hi] = o[:, :hi - l0]
    return out


def case(n, F, D, T, seed=3, big_bias=False):
    """(layered, tiled) float64 results for synthetic weights and inputs."""
    from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
    from emotiongestures_amd.synth import load_synth_weights, synth_inputs
    vae = load_synth_weights(MLP_Reconstruct_v3(frames=F, d_model=D), seed).eval()
    sd = {k: v.detach().double().numpy() for k, v in vae.state_dict().items()}
    if big_bias:
        for k in sd:
            if k.endswith(".bias") and k.split(".")[0] in ("Decoder", "fusion_z_posterior", "Posterior_Y_embedding"):
                sd[k] = np.full_like(sd[k], 1e3)
    inp = synth_inputs(n, F, d_model=D, seed=seed)
    y, z = inp["label"].astype(np.float64), inp["z"].astype(np.float64)
    return layered(sd, y, z), tiled(sd, y, z, T)


if __name__ == "__main__":
    for n, F, D, T in ((1, 34, 512, 128), (1, 60, 192, 128), (2, 34, 64, 64), (1, 34, 192, 64), (1, 34, 64, 128)):
        a, b = case(n, F, D, T)
        print(f"n={n} F={F} D={D} T={T}: max |tiled - layered| = {np.abs(a - b).max():.3e} (max |layered| {np.abs(a).max():.3e})")
