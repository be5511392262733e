"""Emotion recognition of whole tracks: does a generated take show the emotion it was asked for?

The eval loop's ``Emotion_ACC`` (test_emotion_gesture_diversity_iterative.py:216-221; ``harness.evaluate``) runs the skeleton emotion
classifier on clips of exactly ``n_position`` frames.  This module is its whole-track counterpart, on the device (csrc/emotion.hip), for
tracks of any and unequal length with R takes each:

``window_plan(frames, window, stride=None, tail=True)``          host-only counts and starts of the classifier windows
``window_logits(classifier, track, frames=None, ...)``           the classifier on every window -> ``(logits [N, C], plan)``
``emotion_votes(logits, plan_or_counts, draws, labels=None)``    one decision per take, accuracy and confusion matrices -> the dict below
``emotion_of_tracks(classifier, track, frames, labels, ...)``    the two in one call
``EmotionAccuracy()``                                            ``push(dict)`` / ``avg()``: pools the figures over calls

Definition (include/emogest.h).  A classifier window is ``F = n_position`` consecutive poses of one take, never padded or resampled.
Recording u with ``frames[u]`` valid poses has windows at ``0, S, 2S, ...`` while ``start + F <= frames[u]`` (``S`` defaults to ``F``) and,
with ``tail=True``, one more at ``frames[u] - F`` when ``(frames[u] - F) % S != 0``, so that every valid pose is seen; ``C_u`` windows in
all, ``frames[u] < F`` is refused by name.  Clip order: recording-major, then take, then window (clip ``R * coff[u] + r * C_u + j``, ``coff``
the exclusive prefix sum of ``C``); ``N = R * sum(C_u)``.  Poses at or beyond ``frames[u]`` are never read.

A window is valid when all its logits are finite; its class is the lowest index among the maxima (``harness.compute_acc``'s ``topk(1)``
where the maximum is unique), ``-1`` when not valid.  Per take: ``votes [U, R, C]`` and ``invalid [U, R]`` int32, ``mean_logit [U, R, C]``
float64 (the valid windows' widened logits added in ascending order inside chunks of ``CHUNK_WINDOWS`` windows, then the chunks in ascending
order, over the valid count; NaN without a valid window) and ``pred [U, R]``: most votes, then the larger mean logit, then the lowest index;
``-1`` without a valid window.  ``unscored``: the takes with ``pred == -1``.  With labels ``y [U, R]``: ``hit = pred == y``,
``window_hits = votes[u, r, y]``, ``accuracy = 100 * sum hit / (U R)`` and ``window_accuracy = 100 * sum window_hits / N`` (float64, percent),
``confusion [C, C]`` (row = label, column = ``pred``, takes with ``pred >= 0``) and ``window_confusion [C, C]`` (column = window class, valid
windows).  One label per take is what is scored.

CUDA tensors go through the kernels (no eager-PyTorch fallback).  numpy arrays and CPU tensors of logits take the same definition in numpy,
as the other score modules do: every integer is equal and ``mean_logit`` is added in the kernel's order.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._host import BoundedCache, host_ptr, int_list, ptr as _ptr, sized, stream as _stream

__all__ = ["window_plan", "window_logits", "emotion_votes", "emotion_of_tracks", "EmotionAccuracy", "vote_workspace_bytes", "CHUNK_WINDOWS",
           "MAX_CLASSES"]

CHUNK_WINDOWS = L.EG_EMOTION_CHUNK_WINDOWS          # windows of one partial sum: the unit of mean_logit's summation order
MAX_CLASSES = L.EG_EMOTION_MAX_CLASSES
LABEL_KEYS = ("hit", "window_hits", "accuracy", "window_accuracy", "confusion", "window_confusion")


# ---- the window plan -----------------------------------------------------------------------------------------------------------------------
class WindowPlan:
    """The classifier windows of U recordings (eg_emotion_meta: host only): ``frames``, ``off``, ``counts`` (C_u) and ``coff`` as int32 numpy
    ``[U]``, ``total = sum(C_u)`` (N / R), ``window``, ``stride``, ``tail``; ``starts(u)`` the first pose of every window of recording u."""

    def __init__(self, lib, frames, window, stride, tail):
        U = len(frames)
        self.U, self.window, self.stride, self.tail = U, int(window), int(stride), bool(tail)
        self.frames = np.ascontiguousarray(frames, np.int32)
        self.h_frames = host_ptr(self.frames)
        meta = np.zeros(max(int(lib.eg_emotion_meta_ints(U)), 4), np.int32)
        total = int(lib.eg_emotion_meta(self.h_frames, U, self.window, self.stride, int(self.tail), host_ptr(meta)))
        if total <= 0:
            raise L.EgError(f"eg_emotion_meta: refused ({lib.eg_last_error().decode()})")
        self.meta = meta
        self.off, self.counts, self.coff = meta[U:2 * U].copy(), meta[2 * U:3 * U].copy(), meta[3 * U:4 * U].copy()
        self.h_counts = host_ptr(self.counts)
        self.total = total
        self.sum_frames = int(self.frames.astype(np.int64).sum())
        self._tables: dict = {}

    def table(self, device) -> torch.Tensor:
        """The uploaded ``frames | off | C | coff`` table on `device` (once per device)."""
        key = str(device)
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self.meta).to(device)
        return self._tables[key]

    def starts(self, u: int) -> np.ndarray:
        f, F, S = int(self.frames[u]), self.window, self.stride
        s = np.arange(0, f - F + 1, S, dtype=np.int64)
        return np.append(s, f - F) if self.tail and (f - F) % S else s


_PLANS = BoundedCache(16)
_COUNT_TABLES = BoundedCache(16)


def window_plan(frames, window: int, stride: Optional[int] = None, tail: bool = True) -> WindowPlan:
    """Counts and starts of the classifier windows of recordings with ``frames[u]`` valid poses (host only; cached per argument set)."""
    frames = tuple(int_list(frames))
    stride = int(window) if stride is None else int(stride)
    key = (frames, int(window), stride, bool(tail))
    return _PLANS.get(key, lambda: WindowPlan(L.load(), frames, window, stride, tail))


def _counts_of(plan_or_counts, device):
    """-> (counts int32 numpy [U], its host pointer, the device ``C | coff`` table or None without a device, what keeps them alive)."""
    if isinstance(plan_or_counts, WindowPlan):
        p = plan_or_counts
        return p.counts, p.h_counts, None if device is None else p.table(device)[2 * p.U:], p
    counts = tuple(int_list(plan_or_counts))
    if device is None:
        a = np.ascontiguousarray(counts, np.int32)
        return a, host_ptr(a), None, a

    def build():
        a = np.ascontiguousarray(counts, np.int32)
        coff = np.concatenate([[0], np.cumsum(a.astype(np.int64))[:-1]]).astype(np.int32) if len(a) else a
        return a, torch.from_numpy(np.concatenate([a, coff])).to(device)
    a, tab = _COUNT_TABLES.get((counts, str(device)), build)
    return a, host_ptr(a), tab, (a, tab)


# ---- the classifier on every window --------------------------------------------------------------------------------------------------------
def _geometry(classifier, who):
    """(F, d_model, pose_dim, classes) of a SkeletonTransformer; anything else is refused by name."""
    try:
        fc1, head0, last = classifier.prior_seq_encoder.fc1, classifier.post_projector[0], classifier.post_projector[8]
        table = classifier.encoder.position_enc.pos_table
        d_model = int(classifier.d_model)
    except AttributeError:
        raise L.EgError(f"{who}: the classifier must be a harness.SkeletonTransformer, got {type(classifier).__name__}") from None
    for layer in classifier.encoder.layer_stack:                                  # eg_multi_head_attention reads heads * 64 weight rows
        if layer.slf_attn.d_k != 64 or layer.slf_attn.d_v != 64:
            raise L.EgError(f"{who}: the classifier's heads are {layer.slf_attn.d_k} / {layer.slf_attn.d_v} wide; the library's attention "
                            "has d_k = d_v = 64 only")
    F = head0.weight.shape[1] // d_model
    if F < 1 or F * d_model != head0.weight.shape[1] or table.shape[1] < F:
        raise L.EgError(f"{who}: the classifier's head takes {head0.weight.shape[1]} inputs, not n_position * d_model with d_model={d_model}")
    return F, d_model, int(fc1.weight.shape[1]), int(last.weight.shape[0])


def _encoder_layers(classifier, x: torch.Tensor) -> torch.Tensor:
    """The encoder's layer stack on x [n, F, d_model] as ``Encoder.forward`` runs it after the positional addition, without the attention maps."""
    prec = classifier.precision
    for layer in classifier.encoder.layer_stack:
        a = layer.slf_attn
        layer.slf_attn.precision = layer.pos_ffn.precision = prec
        x, _ = ops.multi_head_attention(x, x, a.w_qs.weight, a.w_ks.weight, a.w_vs.weight, a.fc.weight, a.layer_norm.weight, a.layer_norm.bias,
                                        a.n_head, prec, want_attn=False, packed=a.packed(x.device))
        x = layer.pos_ffn(x)
    return x


def window_logits(classifier, track: torch.Tensor, frames=None, stride: Optional[int] = None, tail: bool = True, chunk_clips: int = 1024):
    """The emotion classifier (an eval-mode ``harness.SkeletonTransformer``) on every window of ``track [U, Tmax, D]`` or ``[U, R, Tmax, D]``
    (fp32, CUDA; there is no CPU fallback), ``frames[u]`` valid poses per recording (default Tmax; poses beyond them are never read and may
    hold NaN) -> ``(logits [N, C] fp32 in clip order, plan)``.

    The per-pose embedding (``prior_seq_encoder.fc1``, ``fc2``) runs once per valid pose on ``takes.pack_rows``' packed rows.  Then, for every
    range of at most ``chunk_clips`` clips: eg_emotion_window_embed (the windows and the positional addition in one pass), the encoder layers
    and the head, into the range's rows of ``logits`` -- the FFN hidden map alone is 8 KB per pose row at ``d_inner = 2048``, so the range
    bounds the workspace.  ``classifier``'s own packed weights and ``classifier.precision`` are used.  The products choose their tiles by row
    count, so logits may differ in rounding between values of ``chunk_clips``; everything downstream is defined on the logits the call
    produced.  Not capturable (the loop allocates)."""
    from .harness import _affine_chain
    from .modules import _eval_only
    from .takes import _track4, pack_rows
    who = "window_logits"
    F, Dm, D, C = _geometry(classifier, who)
    _eval_only(classifier)
    trk = _track4(track, who)
    U, R, Tmax, Dt = trk.shape
    if Dt != D:
        raise L.EgError(f"{who}: track has {Dt} pose columns, the classifier takes pose_dim={D}")
    if int(chunk_clips) < 1:
        raise L.EgError(f"{who}: chunk_clips={chunk_clips} (need >= 1)")
    frames = [Tmax] * U if frames is None else int_list(frames)
    if len(frames) != U:
        raise ValueError(f"{who}: frames has {len(frames)} entries for {U} recordings")
    plan = window_plan(frames, F, stride, tail)                                   # refuses frames[u] < F by name
    lib = L.load()
    dev = trk.device
    prec = classifier.precision
    cache = classifier._cache
    with torch.no_grad():
        x, _fr, _off = pack_rows(trk, frames)                                     # [R * sum(frames), Dpad], zero pad columns
        pad = x.shape[1] - D
        for i, lin in enumerate((classifier.prior_seq_encoder.fc1, classifier.prior_seq_encoder.fc2)):
            pk = pad if i == 0 else 0
            packed = cache.get(lin, dev, pad_k=pk)
            x = ops.linear(x, cache.padded_weight(lin) if pk else lin.weight, lin.bias, precision=prec, packed=packed)
        emb = x
        pos = classifier.encoder.position_enc.pos_table[0, :F].to(dev, torch.float32).contiguous()
        head = [classifier.post_projector[i] for i in (0, 2, 4, 6, 8)]
        N = R * plan.total
        logits = torch.empty(N, C, dtype=torch.float32, device=dev)
        table = plan.table(dev)
        step = int(chunk_clips)
        for c0 in range(0, N, step):
            c1 = min(N, c0 + step)
            xin = torch.empty((c1 - c0) * F, Dm, dtype=torch.float32, device=dev)
            L.check(lib.eg_emotion_window_embed(_ptr(emb), _ptr(pos), U, R, F, plan.stride, int(plan.tail), Dm, plan.h_frames, _ptr(table), c0, c1,
                                                _ptr(xin), _stream(dev)), "eg_emotion_window_embed")
            enc = _encoder_layers(classifier, xin.view(c1 - c0, F, Dm))
            logits[c0:c1].copy_(_affine_chain(cache, enc.reshape(c1 - c0, F * Dm), head, True, prec))
    return logits, plan


# ---- the definition in numpy ---------------------------------------------------------------------------------------------------------------
def _votes_host(logits: np.ndarray, counts, R: int, labels: Optional[np.ndarray]) -> dict:
    """logits [N, C] float32, counts [U], labels [U, R] ints in [0, C) or None -> the dict of emotion_votes in numpy."""
    N, C = logits.shape
    U = len(counts)
    finite = np.isfinite(logits).all(1)
    wclass = np.where(finite, np.argmax(np.where(np.isnan(logits), -np.inf, logits), 1), -1).astype(np.int32)
    votes, invalid = np.zeros((U, R, C), np.int32), np.zeros((U, R), np.int32)
    mean, pred = np.full((U, R, C), np.nan, np.float64), np.full((U, R), -1, np.int32)
    wide = logits.astype(np.float64)
    c = 0
    for u, n in enumerate(counts):
        for r in range(R):
            k, ok = wclass[c:c + n], finite[c:c + n]
            votes[u, r] = np.bincount(k[ok], minlength=C)
            invalid[u, r] = n - int(ok.sum())
            if ok.any():
                total = np.zeros(C, np.float64)
                for w0 in range(0, n, CHUNK_WINDOWS):
                    part = np.zeros(C, np.float64)
                    for w in np.flatnonzero(ok[w0:w0 + CHUNK_WINDOWS]):
                        part += wide[c + w0 + w]
                    total += part
                mean[u, r] = total / float(ok.sum())
                best = max(range(C), key=lambda j: (votes[u, r, j], mean[u, r, j], -j))
                pred[u, r] = best
            c += n
    out = {"window_class": wclass, "votes": votes, "invalid": invalid, "mean_logit": mean, "pred": pred,
           "unscored": np.int32((pred < 0).sum())}
    if labels is not None:
        y = labels.astype(np.int64)
        scored = pred >= 0
        out["hit"] = (scored & (pred == y)).astype(np.int32)
        out["window_hits"] = np.take_along_axis(votes, y[..., None], 2)[..., 0].astype(np.int32)
        out["accuracy"] = np.float64(100.0 * float(out["hit"].sum()) / float(U * R))
        out["window_accuracy"] = np.float64(100.0 * float(out["window_hits"].sum(dtype=np.int64)) / float(N))
        conf, wconf = np.zeros((C, C), np.int32), np.zeros((C, C), np.int32)
        np.add.at(conf, (y[scored], pred[scored]), 1)
        for u in range(U):
            for r in range(R):
                wconf[y[u, r]] += votes[u, r]
        out["confusion"], out["window_confusion"] = conf, wconf
    return out


# ---- labels --------------------------------------------------------------------------------------------------------------------------------
def _label_index(labels, U: int, R: int, C: int, who: str):
    """Class indices ``[U]`` / ``[U, R]`` or one-hot ``[U, C]`` / ``[U, R, C]`` -> indices ``[U, R]``: a CUDA tensor stays on its device and is
    trusted; host data come back as int64 numpy, checked against [0, C).  Floating data are one-hot (their argmax is the label, as the eval
    loop's ``torch.max(label, 1)[1]``); integers are indices, except ``[U, R, C]`` and a ``[U, C]`` that cannot be ``[U, R]``."""
    if labels is None:
        return None
    on_dev = isinstance(labels, torch.Tensor) and labels.is_cuda
    lab = labels.detach() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if not on_dev and isinstance(lab, torch.Tensor):
        lab = lab.numpy()
    shape = tuple(lab.shape)
    floating = lab.dtype.is_floating_point if on_dev else np.issubdtype(lab.dtype, np.floating)
    one_hot = (len(shape) == 3 and shape == (U, R, C)) or (len(shape) == 2 and shape == (U, C) and (floating or shape != (U, R)))
    if one_hot:
        lab = lab.argmax(-1)
    elif floating:
        raise L.EgError(f"{who}: labels shape {shape} of floating type: one-hot labels are ({U},{C}) or ({U},{R},{C})")
    if tuple(lab.shape) == (U,):
        lab = lab[:, None].expand(U, R) if on_dev else np.broadcast_to(lab[:, None], (U, R))
    if tuple(lab.shape) != (U, R):
        raise L.EgError(f"{who}: labels shape {shape}: need class indices ({U},) or ({U},{R}), or one-hot ({U},{C}) or ({U},{R},{C})")
    if on_dev:
        return lab
    lab = np.ascontiguousarray(lab, np.int64)
    if lab.size and (lab.min() < 0 or lab.max() >= C):
        bad = np.argwhere((lab < 0) | (lab >= C))[0]
        raise L.EgError(f"{who}: labels[{bad[0]}, {bad[1]}]={lab[bad[0], bad[1]]} outside [0, {C})")
    return lab


# ---- votes ---------------------------------------------------------------------------------------------------------------------------------
def vote_workspace_bytes(plan_or_counts, draws: int, classes: int) -> int:
    """Bytes of ``emotion_votes``' workspace (eg_emotion_vote_workspace_bytes; host only)."""
    _a, h, _t, _keep = _counts_of(plan_or_counts, None)
    return sized("eg_emotion_vote_workspace_bytes", h, len(_a), int(draws), int(classes))


def _new_out(U, R, C, N, dev, with_labels):
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    out = {"window_class": i32(N), "votes": i32(U, R, C), "invalid": i32(U, R),
           "mean_logit": torch.empty(U, R, C, dtype=torch.float64, device=dev), "pred": i32(U, R), "unscored": i32(())}
    if with_labels:
        out.update({"hit": i32(U, R), "window_hits": i32(U, R), "accuracy": torch.empty((), dtype=torch.float64, device=dev),
                    "window_accuracy": torch.empty((), dtype=torch.float64, device=dev), "confusion": i32(C, C), "window_confusion": i32(C, C)})
    return out


def emotion_votes(logits, plan_or_counts, draws: int, labels=None, workspace: Optional[torch.Tensor] = None,
                  out: Optional[dict] = None) -> Dict[str, object]:
    """One decision per take from window ``logits [N, C]`` (fp32, clip order), the windows per recording (a ``WindowPlan`` or the counts
    ``[U]``) and ``draws`` = R: the dict of the module docstring -- ``"window_class" [N]``, ``"votes"``, ``"invalid"``, ``"mean_logit"``,
    ``"pred"``, ``"unscored"`` and, with ``labels``, ``"hit"``, ``"window_hits"``, ``"accuracy"``, ``"window_accuracy"``, ``"confusion"``,
    ``"window_confusion"``.  ``labels``: class indices ``[U]`` or ``[U, R]``, or one-hot ``[U, C]`` or ``[U, R, C]``.

    CUDA logits: eg_emotion_vote, two launches, results on the device (scalars as 0-d tensors).  Labels that arrive on the host are checked
    against ``[0, C)`` and refused by name; labels already on the device are trusted -- a take whose label is out of range has ``hit = 0``,
    enters no matrix cell and counts in ``"unscored"``.  ``workspace`` (uint8, ``vote_workspace_bytes``) and ``out`` (the dict of an earlier
    call of the same shapes) make the call allocation-free for graph capture (with int32 ``[U, R]`` device labels); whoever captures it keeps
    the plan, whose uploaded table the launches read.  numpy or CPU logits: the definition in numpy (numpy in: numpy out; tensor in: tensors)."""
    who = "emotion_votes"
    R = int(draws)
    if not 1 <= R <= 64:
        raise L.EgError(f"{who}: draws={R} (1..64)")
    if len(logits.shape) != 2:
        raise ValueError(f"{who}: logits must be [N, C], got {tuple(logits.shape)}")
    N, C = (int(v) for v in logits.shape)
    if not 2 <= C <= MAX_CLASSES:
        raise L.EgError(f"{who}: classes={C} (2..{MAX_CLASSES})")
    on_dev = isinstance(logits, torch.Tensor) and logits.is_cuda
    dev = logits.device if on_dev else None
    counts, h_counts, d_counts, _keep = _counts_of(plan_or_counts, dev)
    U = len(counts)
    if U < 1 or int(counts.min()) < 1:
        raise L.EgError(f"{who}: counts {counts.tolist()}: every recording needs at least one window")
    if N != R * int(counts.astype(np.int64).sum()):
        raise ValueError(f"{who}: logits has {N} rows, draws * sum(counts) = {R} * {int(counts.sum())}")
    y = _label_index(labels, U, R, C, who)
    if not on_dev:
        as_tensor = isinstance(logits, torch.Tensor)
        if isinstance(y, torch.Tensor):                                           # device labels with host logits: checked like host labels
            y = _label_index(y.cpu(), U, R, C, who)
        res = _votes_host(np.asarray(logits.detach().numpy() if as_tensor else logits, np.float32), counts.tolist(), R, y)
        return {k: torch.as_tensor(v) for k, v in res.items()} if as_tensor else res
    lib = L.load()
    x = logits.detach().to(torch.float32).contiguous()
    d_y = None
    if y is not None:
        d_y = (y if isinstance(y, torch.Tensor) else torch.from_numpy(y).to(dev)).to(torch.int32).contiguous()
    if workspace is None:
        workspace = torch.empty(vote_workspace_bytes(plan_or_counts, R, C), dtype=torch.uint8, device=dev)
    if out is None:
        out = _new_out(U, R, C, N, dev, d_y is not None)
    elif d_y is not None and any(k not in out for k in LABEL_KEYS):
        raise L.EgError(f"{who}: out= lacks the label outputs {[k for k in LABEL_KEYS if k not in out]}")
    lp = [_ptr(out[k]) if d_y is not None else None for k in LABEL_KEYS]
    L.check(lib.eg_emotion_vote(_ptr(x), U, R, C, h_counts, _ptr(d_counts), _ptr(d_y), _ptr(workspace), int(workspace.numel()),
                                _ptr(out["window_class"]), _ptr(out["votes"]), _ptr(out["invalid"]), _ptr(out["mean_logit"]), _ptr(out["pred"]),
                                *lp, _ptr(out["unscored"]), _stream(dev)), "eg_emotion_vote")
    return out


def emotion_of_tracks(classifier, track: torch.Tensor, frames=None, labels=None, stride: Optional[int] = None, tail: bool = True,
                      chunk_clips: int = 1024) -> Dict[str, object]:
    """``emotion_votes(*window_logits(classifier, track, frames, stride, tail, chunk_clips), labels)``: which emotion the classifier
    recognises in every take of ``track [U, Tmax, D]`` (R = 1) or ``[U, R, Tmax, D]``, and how often it is the one asked for.  The dict of
    ``emotion_votes`` (per-take entries ``[U, R, ...]``) plus ``"logits" [N, C]``, ``"windows_per"`` (C_u, U host ints) and
    ``"window_start"`` (per recording the first pose of every window, int64 numpy).  Host labels are checked before anything runs."""
    who = "emotion_of_tracks"
    if not isinstance(track, torch.Tensor) or track.dim() not in (3, 4):
        raise ValueError(f"{who}: track must be [U, Tmax, D] or [U, R, Tmax, D], got "
                         f"{tuple(track.shape) if isinstance(track, torch.Tensor) else type(track).__name__}")
    U, R = int(track.shape[0]), (int(track.shape[1]) if track.dim() == 4 else 1)
    y = _label_index(labels, U, R, _geometry(classifier, who)[3], who)
    logits, plan = window_logits(classifier, track, frames, stride, tail, chunk_clips)
    out = dict(emotion_votes(logits, plan, R, y))
    out["logits"] = logits
    out["windows_per"] = plan.counts.tolist()
    out["window_start"] = [plan.starts(u) for u in range(plan.U)]
    return out


class EmotionAccuracy:
    """Pools the figures of ``emotion_votes`` / ``emotion_of_tracks`` dicts (with labels) over calls, as ``jointscore.SRGR.push`` pools rates:
    ``push(res)`` adds the hits, takes, window hits, windows, unscored takes and both confusion matrices; ``avg()`` is the take accuracy
    ``100 * hits / takes`` so far, ``window_avg()`` the window accuracy, in host float64."""

    def __init__(self):
        self.hits = self.takes = self.window_hits = self.windows = self.unscored = 0
        self.confusion = self.window_confusion = None

    def push(self, res: dict) -> None:
        if "hit" not in res:
            raise L.EgError("EmotionAccuracy.push: the dict has no label figures (emotion_votes was called without labels)")
        host = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
        hit, votes, invalid = host(res["hit"]), host(res["votes"]), host(res["invalid"])
        self.hits += int(hit.sum(dtype=np.int64))
        self.takes += int(hit.size)
        self.window_hits += int(host(res["window_hits"]).sum(dtype=np.int64))
        self.windows += int(votes.sum(dtype=np.int64)) + int(invalid.sum(dtype=np.int64))
        self.unscored += int(host(res["unscored"]))
        conf, wconf = host(res["confusion"]).astype(np.int64), host(res["window_confusion"]).astype(np.int64)
        if self.confusion is None:
            self.confusion, self.window_confusion = conf.copy(), wconf.copy()
        else:
            if conf.shape != self.confusion.shape:
                raise L.EgError(f"EmotionAccuracy.push: {conf.shape[0]} classes after {self.confusion.shape[0]}")
            self.confusion += conf
            self.window_confusion += wconf

    def avg(self) -> float:
        return 100.0 * float(self.hits) / float(self.takes)

    def window_avg(self) -> float:
        return 100.0 * float(self.window_hits) / float(self.windows)
