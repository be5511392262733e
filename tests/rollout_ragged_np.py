"""CPU restatement of the ragged roll-out (include/emogest.h: eg_generator_forward_rollout_ragged) for the tests: U recordings with their own
window counts W_u.  Step s is the generator on the ACTIVE recordings {u : W_u > s} in the order "longer first, ties by index"; a recording's
window w >= 1 is seeded with the raw last prior_frames poses of its own window w - 1; its track is rollout_np.stitch of its own windows.
The generator is passed in, as for rollout_np.rollout, so this file states only the plan, the loop over steps and the packing."""
import numpy as np
import torch

from rollout_np import stitch


def plan(windows_per):
    """The plan in numpy: order (rank -> recording, stable sort by (-W_u, u)), inverse, step_batch [Wmax], offsets [U] (exclusive prefix sum of
    W_u in caller order) and slot_row [N]: step-major slot (s, rank) -> packed recording-major row offsets[order[rank]] + s."""
    wp = np.asarray(windows_per, np.int64)
    assert wp.ndim == 1 and wp.size >= 1 and (wp >= 1).all()
    order = np.asarray(sorted(range(wp.size), key=lambda u: (-wp[u], u)), np.int64)
    inverse = np.empty_like(order)
    inverse[order] = np.arange(wp.size)
    offsets = np.concatenate([[0], np.cumsum(wp)[:-1]]).astype(np.int64)
    step_batch = np.asarray([(wp > s).sum() for s in range(int(wp.max()))], np.int64)
    slot_row = np.asarray([offsets[order[r]] + s for s in range(int(wp.max())) for r in range(step_batch[s])], np.int64)
    return {"order": order, "inverse": inverse, "offsets": offsets, "step_batch": step_batch, "slot_row": slot_row}


def pack(padded, windows_per):
    """[U, Wmax, ...] -> packed [N, ...]: recording u's first W_u entries, recording-major."""
    return np.concatenate([np.asarray(padded)[u, :w] for u, w in enumerate(windows_per)], 0)


def rollout_ragged(generator, spec, text, seed_pose, windows_per, sampled=None, alpha=None):
    """generator(spec [B,...], text [B,...], prior [B,P,D], sampled [B,F,d] | None) -> (pose [B,F,D], emo, sem, pred [B,8], txt), torch tensors.
    spec / text / sampled PACKED [N, ...] torch tensors, seed_pose [U,P,D].  Returns numpy: windows [N,F,D] and emotion_prediction [N,8] packed,
    track [U, Wmax*H + P, D] zero past track_frames[u], track_frames, window_offsets, and priors [N,P,D] (what every window was seeded with)."""
    pl = plan(windows_per)
    wp, order, off = [int(v) for v in windows_per], pl["order"], pl["offsets"]
    U, N, Wmax, P = len(wp), sum(wp), max(wp), seed_pose.shape[1]
    prior = {int(u): seed_pose[int(u)] for u in order}
    windows, preds, priors = [None] * N, [None] * N, [None] * N
    for s in range(Wmax):
        act = [int(u) for u in order[:pl["step_batch"][s]]]                 # nothing of an inactive recording enters the step
        rows = torch.as_tensor([int(off[u]) + s for u in act])
        out = generator(spec[rows].contiguous(), text[rows].contiguous(), torch.stack([prior[u] for u in act]).contiguous(),
                        None if sampled is None else sampled[rows].contiguous())
        for i, u in enumerate(act):
            row = int(off[u]) + s
            priors[row], windows[row], preds[row] = prior[u].numpy(), out[0][i].numpy(), out[3][i].numpy()
            prior[u] = out[0][i, out[0].shape[1] - P:, :]
    windows = np.stack(windows).astype(np.float32)
    F, D = windows.shape[1:]
    H = F - P
    track = np.zeros((U, Wmax * H + P, D), np.float32)
    for u in range(U):
        track[u, : wp[u] * H + P] = stitch(windows[None, off[u]: off[u] + wp[u]], P, alpha)[0]
    return {"windows": windows, "track": track, "track_frames": np.asarray([w * H + P for w in wp], np.int64), "window_offsets": off,
            "emotion_prediction": np.stack(preds), "priors": np.stack(priors)}
