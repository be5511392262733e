"""CPU restatement of the long-form roll-out (include/emogest.h: eg_generator_forward_rollout) for the tests and the golden script:
the generator called window after window, every window seeded with the RAW last prior_frames poses of the one before it, and the
per-window poses stitched into one track by a linear cross-fade over the overlap.  The generator itself is passed in (the CPU oracle's
generator_forward in the tests, the reference's own Transformer in tests/golden/make_golden_rollout.py), so this file only states
the loop, the hand-off and the stitch."""
import os

import numpy as np
import torch

from emotiongestures_amd.synth import load_synth_weights, synth_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"rollout_ted_spatial": "spatial", "rollout_ted_memory": "memory"}       # fixture -> generator variant


def default_alpha(prior_frames: int) -> np.ndarray:
    """alpha[j] = (j + 1) / (P + 1): the weight of the NEW window on overlap frame j."""
    return (np.arange(1, prior_frames + 1, dtype=np.float32) / np.float32(prior_frames + 1)).astype(np.float32)


def stitch(windows: np.ndarray, prior_frames: int, alpha=None) -> np.ndarray:
    """windows [U, W, F, D] raw per-window poses -> track [U, W*H + P, D], H = F - P, in fp32 (two rounded products, one rounded sum):
    track[:, w*H + j] = (1 - alpha[j]) * pose_{w-1}[:, H + j] + alpha[j] * pose_w[:, j] for j < P and w >= 1, pose_w[:, j] otherwise."""
    windows = np.asarray(windows, np.float32)
    U, W, F, D = windows.shape
    P, H = prior_frames, F - prior_frames
    a = default_alpha(P) if alpha is None else np.asarray(alpha, np.float32)
    assert a.shape == (P,)
    track = np.zeros((U, W * H + P, D), np.float32)
    track[:, :F] = windows[:, 0]
    for w in range(1, W):
        old = (np.float32(1) - a)[None, :, None] * windows[:, w - 1, H:]
        new = a[None, :, None] * windows[:, w, :P]
        track[:, w * H: w * H + P] = old + new
        track[:, w * H + P: w * H + F] = windows[:, w, P:]
    return track


def rollout(generator, spec, text, seed_pose, sampled=None, alpha=None):
    """generator(spec [U,...], text [U,...], prior [U,P,D], sampled [U,F,d] | None) -> (pose [U,F,D], emo, sem, pred [U,8], txt), torch
    tensors.  spec [U,W,...], text [U,W,...], seed_pose [U,P,D], sampled [U,W,F,d] | None.  Every call sees the U windows of one index."""
    U, W = spec.shape[0], spec.shape[1]
    P = seed_pose.shape[1]
    prior, poses, preds, priors = seed_pose, [], [], []
    for w in range(W):
        priors.append(prior)
        out = generator(spec[:, w].contiguous(), text[:, w].contiguous(), prior.contiguous(), None if sampled is None else sampled[:, w].contiguous())
        poses.append(out[0])
        preds.append(out[3])
        prior = out[0][:, out[0].shape[1] - P:, :]
    windows = torch.stack(poses, 1).numpy()
    return {"windows": windows, "track": stitch(windows, P, alpha), "emotion_prediction": torch.stack(preds, 1).numpy(),
            "priors": torch.stack(priors, 1).numpy()}


def rollout_inputs(U, W, frames=34, pose_dim=126, prior_frames=4, spec_len=124, n_words=200, seed=0, seed_pose_scale=1.0):
    """The fixtures' inputs, regenerated from the seed: synth_inputs for U*W clips taken as [U, W, ...] (utterance-major); the seed pose is
    window 0's pre_pose times seed_pose_scale; label / z [U, W, ...] feed the CVAE where a fixture uses it."""
    inp = synth_inputs(U * W, frames, pose_dim, prior_frames, spec_len=spec_len, n_words=n_words, seed=seed)
    r = lambda a: a.reshape((U, W) + a.shape[1:])
    return {"spec": r(inp["spec"]), "text": r(inp["text"]), "label": r(inp["label"]), "z": r(inp["z"]),
            "seed_pose": (r(inp["pre_pose"])[:, 0] * np.float32(seed_pose_scale)).astype(np.float32)}


def free_running_tol(pose_tol: float, window_gain: float, handoff_gain: float, w: int) -> float:
    """Tolerance of window w of a free-running roll-out: POSE_TOL * (1 + window_gain * sum_{i<w} handoff_gain^i), both gains measured
    on the reference by the golden script (stored in the fixture)."""
    return pose_tol * (1.0 + window_gain * sum(handoff_gain ** i for i in range(w)))


def load_case(name):
    """The fixture, its meta as a dict, its inputs regenerated from the seed, and the per-window CVAE sample where the fixture uses one."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    U, W, frames, pose_dim, prior, chunk, spec_len, n_words, seed, use_sampled = [int(v) for v in z["meta"]]
    m = dict(U=U, W=W, frames=frames, pose_dim=pose_dim, prior=prior, chunk=chunk, spec_len=spec_len, n_words=n_words, seed=seed,
             use_sampled=bool(use_sampled), scale=float(z["seed_pose_scale"]))
    inp = rollout_inputs(U, W, frames, pose_dim, prior, spec_len, n_words, seed, m["scale"])
    sampled = None
    if use_sampled:
        from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
        from oracle import emogest_oracle as O         # from the CPU oracle with a `frames`-frame CVAE (the fixture's own construction)
        vae = load_synth_weights(MLP_Reconstruct_v3(frames=frames), seed).eval()
        sd_v = {k: v.detach() for k, v in vae.state_dict().items()}
        with torch.no_grad():
            sampled = O.cvae_sample(sd_v, torch.from_numpy(inp["label"].reshape(U * W, 8)), torch.from_numpy(inp["z"].reshape(U * W, 32)))
        sampled = sampled.reshape(U, W, frames, 512)
    return z, m, inp, sampled
