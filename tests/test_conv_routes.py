"""CPU-only: the three host-side route queries of csrc/conv.hip against a restatement of their rules.  Callers size the pooling-partial buffers from
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



# csrc/conv.hip ROUTES restated: (cin, stride, cout_lo, cout_hi); the padded width of a route is its widest count rounded up to the 16-channel tile
ROUTES = ((32, 1, 32, 32), (32, 1, 17, 31), (32, 2, 49, 64), (64, 1, 49, 64), (64, 2, 113, 128), (64, 1, 128, 128), (128, 1, 65, 128), (128, 1, 49, 64),
          (128, 1, 1, 48), (128, 2, 241, 256), (256, 1, 256, 256))


def _cout_pad(cin, cout, stride):
    for rc, rs, lo, hi in ROUTES:
        if (rc, rs) == (cin, stride) and lo <= cout <= hi:
            return _cdiv(hi, 16) * 16
    return 0


def test_cout_pad_is_the_width_of_the_serving_route_and_zero_elsewhere(lib):
    served = 0
    for cin, stride, cout in itertools.product((16, 32, 48, 64, 96, 128, 256), (1, 2, 3), range(0, 260)):
        got = int(lib.eg_conv3x3_cout_pad(cin, cout, stride))
        assert got == _cout_pad(cin, cout, stride), (cin, stride, cout)
        if got:
            served += 1
            assert got % 16 == 0 and got >= cout, (cin, stride, cout, got)
    assert served == 1 + 15 + 16 + 16 + 16 + 1 + 128 + 16 + 1
    # the widths that are NOT round_up(cout, 16): what a caller packing by the 16-channel granule gets wrong
    assert [int(lib.eg_conv3x3_cout_pad(128, c, 1)) for c in (1, 20, 32, 33, 48, 49, 64, 65, 100, 112, 113, 128)] == [48, 48, 48, 48, 48, 64, 64, 128, 128, 128, 128, 128]


def test_the_host_packers_pack_at_the_route_width(lib):
    import torch
    from emotiongestures_amd import ops
    for cin, cout, want in ((128, 20, 48), (128, 34, 48), (128, 60, 64), (128, 68, 128), (32, 20, 32), (64, 52, 64), (48, 20, 32)):
        assert ops.conv3x3_cout_pad(cin, cout, 1) == want
        if cin % 8 == 0:
            wp, bp, sp, tp = ops.conv3x3_pack(torch.ones(cout, cin, 3, 3), torch.ones(cout), torch.ones(cout), torch.ones(cout), "cpu")
            assert wp.numel() == int(lib.eg_conv3x3_packed_floats(cin, want))
            for v in (bp, sp, tp):
                assert v.shape == (want,) and float(v.sum()) == cout and float(v[cout:].abs().sum()) == 0.0
            # fp32 image [tap][ci / 4][co][4]: the columns past cout are zero
            img = wp[:9 * cin * want].view(9, cin // 4, want, 4)
            assert float(img[:, :, :cout].min()) == 1.0 and float(img[:, :, cout:].abs().sum()) == 0.0


def test_the_training_path_refuses_a_width_its_device_packer_cannot_build(lib):
    import torch
    from emotiongestures_amd._lib import EgError
    from emotiongestures_amd.train import functional as TF_
    for cout in (20, 32, 68, 100):
        with pytest.raises(EgError):
            TF_._conv_operands(torch.zeros(cout, 128, 3, 3), None)
