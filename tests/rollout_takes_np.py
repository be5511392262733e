"""CPU restatement of the takes roll-out (include/emogest.h: eg_generator_forward_rollout_takes): by definition the ragged roll-out of
tests/rollout_ragged_np.py on U*R recordings, recording u*R + r having recording u's windows, text, seed pose and W_u and its own sampled
maps.  This file only states the replication, the packed take order, the fold back and the plan with its slot_rank section; the loop, the
hand-off and the stitch stay rollout_ragged_np's and rollout_np's."""
import numpy as np
import torch

import rollout_ragged_np as RR


def repeat(windows_per, draws):
    """W_u of the U*R replicated recordings: every count R times."""
    return tuple(int(w) for w in windows_per for _ in range(draws))


def take_rows(windows_per, draws):
    """take_window_offsets [U, R]: the first packed row R*off[u] + r*W_u of draw r of recording u."""
    wp = np.asarray(windows_per, np.int64)
    off = np.concatenate([[0], np.cumsum(wp)[:-1]])
    return draws * off[:, None] + np.arange(draws)[None, :] * wp[:, None]


def replicate_ragged(spec, text, seed_pose, windows_per, sampled):
    """Packed spec [N, ...] / text [N, ...], seed_pose [U, ...] and sampled [N*R, ...] in the packed take order -> the arguments of the
    ragged call on the U*R recordings of the definition (torch tensors): spec, text, seed_pose, sampled.  `sampled` is in that call's packed
    order already; the windows of recording u are repeated R times in place."""
    wp = [int(w) for w in windows_per]
    N = sum(wp)
    assert sampled.shape[0] % N == 0
    Rd = sampled.shape[0] // N
    off = np.concatenate([[0], np.cumsum(wp)[:-1]])
    rows = torch.as_tensor([int(off[u]) + w for u in range(len(wp)) for _ in range(Rd) for w in range(wp[u])], device=spec.device)
    rep = lambda x: x[:, None].expand((len(wp), Rd) + tuple(x.shape[1:])).reshape((len(wp) * Rd,) + tuple(x.shape[1:])).contiguous()
    return spec[rows].contiguous(), text[rows].contiguous(), rep(seed_pose), sampled


def first_take_rows(windows_per, draws):
    """For every packed window row of the U recordings [N], its row in draw 0 of the replicated call's packed order [N*R]."""
    wp = [int(w) for w in windows_per]
    tr = take_rows(wp, draws)
    return np.asarray([tr[u, 0] + w for u in range(len(wp)) for w in range(wp[u])], np.int64)


def plan(windows_per):
    """rollout_ragged_np.plan plus slot_rank [N] (the rank of step-major slot (s, rank)) and the device table of the takes plan:
    slot_row [N] | order [U] | W by rank [U] | slot_rank [N]."""
    pl = RR.plan(windows_per)
    wp = np.asarray(windows_per, np.int64)
    pl["slot_rank"] = np.asarray([r for s in range(int(wp.max())) for r in range(pl["step_batch"][s])], np.int64)
    pl["table"] = np.concatenate([pl["slot_row"], pl["order"], wp[pl["order"]], pl["slot_rank"]]).astype(np.int32)
    return pl
