"""CPU-only: the two host-side route queries of csrc/conv.hip against a restatement of their rules.  Callers size the pooling-partial buffers from
eg_conv3x3_gap_tiles before they know whether a shape has a kernel, so it must answer for every shape, served or not."""
import itertools

import pytest

CHANNELS = (32, 34, 48, 60, 64, 120, 128, 256)
MAPS = ((1, 1), (5, 7), (16, 64), (17, 65), (128, 124), (9, 33))
F32, BF16X3, BF16 = 0, 1, 2


def _cdiv(a, b):
    return -(-a // b)


def _tile_rows(cin, cout, stride):
    if stride == 2 or cout >= 256:
        return 2
    if cin == 32 and cout == 32:
        return 4
    return 4 if (cin >= 128 or cout >= 128) else 8


def _gap_tiles(h, w, cin, cout, stride):
    ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
    return _cdiv(ho, _tile_rows(cin, cout, stride)) * _cdiv(wo, 32)


@pytest.fixture(scope="module")
def lib():
    from emotiongestures_amd import _lib
    return _lib.load()


def test_gap_tiles_is_total_and_follows_the_tile_height_rule(lib):
    for cin, cout, stride, (h, w) in itertools.product(CHANNELS, CHANNELS, (1, 2), MAPS):
        assert int(lib.eg_conv3x3_gap_tiles(h, w, cin, cout, stride)) == _gap_tiles(h, w, cin, cout, stride), (h, w, cin, cout, stride)


def test_channel_split_follows_the_workgroup_count_rule(lib, monkeypatch):
    monkeypatch.delenv("EG_CONV_SPLIT", raising=False)
    for c, batch, (h, w) in itertools.product(CHANNELS, (1, 2, 8, 64), MAPS):
        wgs = _gap_tiles(h, w, c, c, 1) * batch
        want, cap = 1, {64: 2, 128: 4}.get(c, 1)
        while want < cap and wgs * want * 2 <= 512:
            want *= 2
        assert int(lib.eg_conv3x3_channel_split(batch, h, w, c, c, 1, BF16X3)) == want, (batch, h, w, c)
        for stride, prec in ((1, F32), (1, BF16), (2, BF16X3)):
            assert int(lib.eg_conv3x3_channel_split(batch, h, w, c, c, stride, prec)) == 1, (batch, h, w, c, stride, prec)
    for cin, cout in ((32, 64), (64, 128), (128, 64), (128, 34)):
        assert int(lib.eg_conv3x3_channel_split(1, 16, 64, cin, cout, 1, BF16X3)) == 1, (cin, cout)

