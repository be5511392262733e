"""Device-side plumbing shared by the test_gpu_*_f64.py modules of tests/train_tail_f64.py (a helper, not collected): canary-guarded buffers, uploads at
a chosen float offset from a 16-byte boundary, and the FRACTION report.  Every output of a C-ABI call sits in a buffer filled with one NaN bit
pattern, GUARD slots before and behind it; after the call the guards must still hold it (a store past the result lands there), and a refused call
must leave the whole buffer untouched."""
import torch

import train_tail_f64 as S

SENTINEL = 0x7FC5A5A5
GUARD = 256                 # 4-byte slots on each side: 1 KB, so the result itself starts on a 16-byte boundary (+ 4 * offset)
BAD_ARG, UNSUPPORTED = -1, -2
FRACTIONS = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, _stream(dev())


class Guarded:
    """A float32 (or int16 / int32 through .buf views) result of `shape` in the middle of a sentinel-filled buffer, `offset` floats past a 16-byte
    boundary.  init: values to hold before the call (in / out operands)."""

    def __init__(self, shape, offset=0, init=None):
        self.n = 1
        for v in shape:
            self.n *= int(v)
        self.lo = GUARD + offset
        self.buf = torch.full((self.lo + self.n + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
        self.t = self.buf.view(torch.float32)[self.lo:self.lo + self.n].view(tuple(shape))
        if init is not None:
            self.t.copy_(init.to(torch.float32).reshape(tuple(shape)))

    def intact(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[:self.lo] == SENTINEL).all()), f"{what}: a store in front of the result"
        assert bool((b[self.lo + self.n:] == SENTINEL).all()), f"{what}: a store behind the result"
        return self.t.cpu().clone()

    def untouched(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf == SENTINEL).all()), f"{what}: written although the call was refused or the output is optional"


def up(t, offset=0):
    """A CPU tensor on the device, `offset` elements past a 16-byte boundary (offset 1 of a float tensor: misaligned for every float4 access)."""
    if t is None:
        return None
    t = t.contiguous()
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev())
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def workspace(floats, offset=0):
    """A guarded workspace of exactly `floats` floats."""
    return Guarded((max(int(floats), 1),), offset)


def frac(op, got, ref, bound, what, axes=None, channels=None):
    """compare_sliced on the whole tensor, every slice and every element; prints and records the worst element as a FRACTION of its bound.
    channels: a boolean mask over the last axis -- only those columns are held (the others' bound is not finite)."""
    got, ref, bound = torch.as_tensor(got).cpu(), torch.as_tensor(ref), torch.as_tensor(bound)
    if channels is not None:
        bound = bound.expand(ref.shape)
        got, ref, bound = got.reshape(ref.shape)[..., channels], ref[..., channels], bound[..., channels]
    if ref.numel() == 0:
        return 0.0
    if ref.dim() == 0:
        got, ref, bound = got.reshape(1), ref.reshape(1), bound.reshape(1)
    el = S.compare_sliced(got, ref, bound, what, axes)[2]
    FRACTIONS[op] = max(FRACTIONS.get(op, 0.0), el)
    return el


def report(*ops):
    for op in ops:
        if op in FRACTIONS:
            print(f"FRACTION {op}: {FRACTIONS[op]:.3f}")
