"""The rows of a whole-track stage on the Python side (include/emogest.h, "Rows of whole tracks"; csrc/rows.h): data ``[..., T, *]`` with
up to two leading axes -- ``()``, ``(U,)`` recordings or ``(U, R)`` draws of recordings -- is ``U * R`` rows of T frames, and ``frames [U]``
gives the valid frames of a recording, shared by its R rows.  The helpers every such stage uses, and ``front``, the one front end of the
stages whose output is per row.  Nothing here depends on a stage."""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from ._host import int_list


def frames_list(frames, U: int, T: int, who: str) -> Optional[List[int]]:
    if frames is None:
        return None
    fr = int_list([frames] if isinstance(frames, int) else frames)          # a bare int means one recording
    if len(fr) != U:
        raise L.EgError(f"{who}: frames has {len(fr)} entries for {U} recordings")
    if any(v < 0 or v > T for v in fr):
        raise L.EgError(f"{who}: frames {fr}: every value must be in [0, {T}]")
    return fr


def frames_dev(fr: Optional[List[int]], device) -> Optional[torch.Tensor]:
    return None if fr is None else torch.tensor(fr, dtype=torch.int32, device=device)


def counts32(frames) -> Optional[np.ndarray]:
    """Host counts as the C ABI takes them: contiguous int32, or None.  The caller keeps the array alive over the call."""
    return None if frames is None else np.ascontiguousarray(frames, np.int32)


def count_list(v, n: int, who: str, name: str = "frames") -> List[int]:
    """One integer per recording of the packed-rows calls (beat, takes); a wrong length is a ValueError there."""
    v = int_list(v)
    if len(v) != n:
        raise ValueError(f"{who}: {name} has {len(v)} entries for {n} recordings")
    return v


def lead_axes(shape, n_tail: int, who: str):
    """Leading axes ``()``, ``(U,)`` or ``(U, R)`` -> (lead, U, R)."""
    lead = tuple(shape[:-n_tail])
    if len(lead) > 2:
        raise L.EgError(f"{who}: shape {tuple(shape)}: at most two leading axes ([U, R, ...])")
    U = lead[0] if lead else 1
    R = lead[1] if len(lead) == 2 else 1
    return lead, int(U), int(R)


def per_row(fr: Optional[List[int]], U: int, R: int, T: int) -> List[int]:
    return [n for n in (fr if fr is not None else [T] * U) for _ in range(R)]


def is_cuda(x) -> bool:
    return isinstance(x, torch.Tensor) and x.is_cuda


def host64(x, who: str = "") -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, np.float64)


def host32(x) -> np.ndarray:
    return np.asarray(x.detach().numpy() if isinstance(x, torch.Tensor) else x, np.float32)


def dev32(x: torch.Tensor) -> torch.Tensor:
    x = x.detach().to(torch.float32).contiguous()
    return x.clone() if x.data_ptr() % 16 else x                # a slice of a larger tensor may start anywhere


def front(x, n_tail: int, frames, who: str, on_device, on_host, min_frames: int = 0, why: str = "", host=host64) -> SimpleNamespace:
    """The front end of a stage whose output is per row: ``x [..., T, *]`` with ``n_tail`` axes from T on.  Takes the leading axes, checks
    ``frames`` and refuses the first recording with fewer than ``min_frames`` valid frames (``why``: the bound in the message's words), then
    ``on_device(x [U * R, T, *] fp32, fr, d_frames, R)`` for a CUDA tensor or ``on_host(host(x) [U * R, T, *], per_row)`` for anything else
    (numpy in: numpy out; tensor in: tensors out).  Returns ``lead``, ``U``, ``R``, ``T``, ``fr`` (the checked list or None), ``per_row``
    and ``res``, what the callback returned: the caller shapes its result under ``lead``."""
    shape = tuple(x.shape)
    lead, U, R = lead_axes(shape, n_tail, who)
    T = shape[-n_tail]
    fr = frames_list(frames, U, T, who)
    for u, n in enumerate(fr if fr is not None else [T] * U):
        if n < min_frames:
            raise L.EgError(f"{who}: recording {u} has {n} valid frames < {why}")
    rows = (U * R,) + shape[-n_tail:]
    pr = per_row(fr, U, R, T)
    if is_cuda(x):
        xd = dev32(x).reshape(rows)
        res = on_device(xd, fr, frames_dev(fr, xd.device), R)
    else:
        res = on_host(host(x).reshape(rows), pr)
        if isinstance(x, torch.Tensor):
            res = tuple(torch.from_numpy(r) for r in res) if isinstance(res, tuple) else torch.from_numpy(res)
    return SimpleNamespace(lead=lead, U=U, R=R, T=T, fr=fr, per_row=pr, res=res)
