"""Host plumbing between torch tensors and the C ABI of libemogest_hip.so: pointer and stream casts, the GPU-tensor check, host integer
vectors, the "size a buffer or raise" call and the bounded "build once per key" cache.  Every wrapper module takes these from here; nothing here depends on one of them."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def host_ptr(a):
    """The address of a contiguous numpy array (None stays None).  The caller keeps the array alive for as long as the pointer is used."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def need_cuda(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not t.is_cuda:
        raise L.EgError(f"{name}: the HIP path needs a GPU tensor (got {t.device}); there is no CPU fallback")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def int_list(v) -> list:
    """A torch tensor (any device; a GPU tensor synchronises), an ndarray or any iterable of integer-likes -> a list of Python ints.  Nothing
    about length or range is checked here: every caller has its own check and wording.  A bare int is not iterable: TypeError."""
    return [int(a) for a in (v.tolist() if hasattr(v, "tolist") else v)]


def sized(fn_name: str, *args) -> int:
    """The bytes a ``*_bytes`` sizer of the library asks for; a refusal (<= 0) raises with the library's last error."""
    lib = L.load()
    nbytes = int(getattr(lib, fn_name)(*args))
    if nbytes <= 0:
        raise L.EgError(f"{fn_name}: refused ({lib.eg_last_error().decode()})")
    return nbytes


def device_bytes(fn_name: str, device, *args) -> torch.Tensor:
    """A uint8 tensor of ``sized(fn_name, *args)`` bytes on ``device`` (uninitialised)."""
    return torch.empty(sized(fn_name, *args), dtype=torch.uint8, device=device)


class BoundedCache:
    """`get(key, build)`: `build()` once per missing key, the result kept in insertion order.  With `limit` entries present the oldest
    insertion is dropped first (FIFO: a hit does not refresh an entry); `limit=None` keeps everything.

    An entry may own device memory (a plan's uploaded table).  A caller who bakes such an address into a captured graph must hold the entry
    itself: `limit` later distinct keys evict it from here, and with the last reference gone the allocator hands the memory out again."""

    def __init__(self, limit: Optional[int] = None):
        self.limit = limit
        self._d: dict = {}

    def get(self, key, build):
        ent = self._d.get(key)
        if ent is None:
            ent = build()
            if self.limit is not None and len(self._d) >= self.limit:
                self._d.pop(next(iter(self._d)))
            self._d[key] = ent
        return ent

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d
