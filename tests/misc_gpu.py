"""Device-side plumbing of the test_gpu_*_f64.py modules of tests/misc_f64.py (a helper, not collected), on top of tests/train_tail_gpu.py: inputs
uploaded into NaN-filled buffers, so that whatever a kernel reads outside its operands poisons the result."""
import ctypes as C

import torch

import train_tail_gpu as D

NAN_PAD = 64


def up_nan(t, ld=None):
    """A CPU float tensor on the device with NAN_PAD NaNs in front of and behind it.  ld: the rows of a 2-D tensor are laid ld >= columns apart and
    the gap columns are NaN as well.  -> the device view of t's shape."""
    t = t.contiguous()
    if ld is None:
        buf = torch.full((t.numel() + 2 * NAN_PAD,), float("nan"), dtype=t.dtype, device=D.dev())
        v = buf[NAN_PAD:NAN_PAD + t.numel()].view(t.shape)
    else:
        rows, cols = t.shape
        buf = torch.full((rows * ld + 2 * NAN_PAD,), float("nan"), dtype=t.dtype, device=D.dev())
        v = buf[NAN_PAD:NAN_PAD + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(t)
    return v


def pointer_array(tensors, n):
    """A host array of n device pointers (NULL where a tensor is None), as eg_prior_encoder takes its weights."""
    return (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tensors])


def bits(t):
    return t.contiguous().view(torch.int32)
