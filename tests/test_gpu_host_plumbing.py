"""The host plumbing every C-ABI wrapper shares (emotiongestures_amd._host) on the GPU: device pointers, the current stream's handle and
the GPU-tensor check."""
import pytest
import torch

from emotiongestures_amd import _host as H
from emotiongestures_amd import _lib as L

pytestmark = pytest.mark.gpu


def test_ptr_stream_and_need_cuda():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    t = torch.arange(8, dtype=torch.int32, device=dev)
    assert H.ptr(t).value == t.data_ptr() and H.ptr(None) is None
    assert (H.stream(dev).value or 0) == torch.cuda.current_stream(dev).cuda_stream     # the default stream's handle 0 reads back as None
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(dev) == side
        assert (H.stream(dev).value or 0) == side.cuda_stream
    with pytest.raises(L.EgError, match="needs a GPU tensor"):
        H.need_cuda(t.cpu(), "t")
    f = H.need_cuda(t, "t")
    assert f.dtype == torch.float32 and f.is_cuda and torch.equal(f, t.float())
    v = t.float().view(2, 4).t()
    c = H.need_cuda(v, "v")
    assert not v.is_contiguous() and c.is_contiguous() and torch.equal(c, v)
