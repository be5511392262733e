"""The stride-2 stage-entry convolutions on parity planes (csrc/conv.hip: conv3x3_s2_planes_kernel), every output element against F.conv2d in
float64 on the CPU.  The bound is measured, not chosen: the interleaved form (EG_CONV_S2=interleaved) runs on the same inputs, and the plane walk
must stay within 2x of its maximum element error -- both forms sum the same 288 or 576 products per element in fp32 and differ only in their
order, so a factor beyond order effects is an indexing error.  tests/test_gpu_kernels.py's TOL on rel_l2 is the second net.  The pooling
partials keep the interleaved form's layout: one per 2 x 32 output block, eg_conv3x3_gap_tiles of them.
The launch function picks the form by the size of the launch, and the roll-outs rely on results that do not depend on the batch a clip is
computed in (tests/test_gpu_rollout_draws.py), so the interleaved form accumulates its taps in plane order as well and both forms fold a block's
partial row by row: outputs and partials of the two forms are also compared bit for bit."""
import contextlib
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import build_mirror, rel_l2
from emotiongestures_amd.synth import hash_uniform

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-6, "bf16x3": 3e-5, "bf16": 2e-2}         # tests/test_gpu_kernels.py:14
# the plane walk's forms per entry: both tile heights of 32 -> 64 (the default rule picks by workgroup count), the one of 64 -> 128
FORMS = {32: ("planes4", "planes8"), 64: ("planes",)}
# 5 x 7: a map smaller than a tile; 16 x 64: Wo = 32, one full column tile; 17 x 65 and 18 x 66: Wo = 33, a second column tile of one column, with
# odd and even last rows; 19 x 62: Ho = 10, not a multiple of either tile height
SHAPES = [(5, 7), (16, 64), (17, 65), (18, 66), (19, 62)]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def T(key, shape, lo=-1.0, hi=1.0, seed=0):
    return torch.from_numpy(hash_uniform(key, shape, lo, hi, seed))


@contextlib.contextmanager
def conv_s2(form):
    old = os.environ.get("EG_CONV_S2")
    os.environ["EG_CONV_S2"] = form
    try:
        yield
    finally:
        if old is None:
            del os.environ["EG_CONV_S2"]
        else:
            os.environ["EG_CONV_S2"] = old


@functools.lru_cache(maxsize=None)
def _case(cin, cout, B, H, W):
    """(x NCHW, w, bias, scale, shift, float64 convolution without epilogue): built once per shape, shared by the precisions, never modified."""
    x = T(f"x{cin}", (B, cin, H, W), -1, 1)
    w = T(f"w{cin}{cout}", (cout, cin, 3, 3), -0.1, 0.1)
    bias, scale, shift = T("b", (cout,), -0.2, 0.2), T("s", (cout,), 0.5, 1.5), T("t", (cout,), -0.3, 0.3)
    raw = F.conv2d(x.double(), w.double(), None, stride=2, padding=1)
    return x, w, bias, scale, shift, raw


def _block_sums(ref):
    """Sums of ref [B, C, Ho, Wo] over its 2 x 32 blocks, in the numbering of eg_conv3x3_gap_tiles: [B, blocks, C]."""
    B, C, Ho, Wo = ref.shape
    p = F.pad(ref, (0, -Wo % 32, 0, -Ho % 2))
    s = p.view(B, C, p.shape[2] // 2, 2, p.shape[3] // 32, 32).sum((3, 5))
    return s.reshape(B, C, -1).permute(0, 2, 1)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128)])
def test_plane_walk_against_float64_within_2x_of_the_interleaved_form(cin, cout, B, H, W, prec):
    from emotiongestures_amd import _lib, ops
    x, w, bias, scale, shift, raw = _case(cin, cout, B, H, W)
    xg = x.permute(0, 2, 3, 1).contiguous().to(dev())
    tiles = int(_lib.load().eg_conv3x3_gap_tiles(H, W, cin, cout, 2))
    for epi in (False, True):               # without / with bias, ReLU and the affine
        ref = raw
        if epi:
            ref = F.relu(raw + bias.double().view(1, -1, 1, 1)) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        args = (bias, scale, shift) if epi else (None, None, None)

        def run(form):
            with conv_s2(form):
                y, gap = ops.conv3x3(xg, w, *args, stride=2, relu=epi, want_gap=True, precision=prec)
            return y.cpu().permute(0, 3, 1, 2).double(), gap.cpu().double()

        y_old, gap_old = run("interleaved")
        e_old = float((y_old - ref).abs().max())
        for form in FORMS[cin]:
            y, gap = run(form)
            assert y.shape == ref.shape and torch.isfinite(y).all()
            # the launch function picks the form by the size of the launch, and results must not depend on the batch: the interleaved form sums the
            # taps in plane order too, and the partials fold row by row in both -- every element and every partial bit for bit
            assert torch.equal(y, y_old) and torch.equal(gap, gap_old)
            e_new = float((y - ref).abs().max())
            e_l2 = rel_l2(y.numpy(), ref.numpy())
            print(f"{cin}->{cout} B={B} {H}x{W} {prec} epilogue={int(epi)} {form}: max |err| vs float64 {e_new:.3e} (interleaved {e_old:.3e}), "
                  f"rel_l2 {e_l2:.3e}")
            assert e_new <= 2 * e_old
            assert e_l2 < TOL[prec]
            assert gap.shape == (B, tiles, cout)
            assert rel_l2(gap.sum(1).numpy(), ref.sum((2, 3)).numpy()) < max(TOL[prec], 1e-5)
            # every partial is the sum of its own 2 x 32 block
            assert rel_l2(gap.numpy(), _block_sums(ref).numpy()) < max(TOL[prec], 1e-5)


@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128)])
def test_training_forms_squares_partials_and_input_affine(cin, cout):
    """eg_conv3x3_sq_in_affine at stride 2 (the training path's forms of the same launch): x' = x * in_scale[ci] + in_shift[ci] inside the image,
    zero padding stays zero, bias and ReLU, partial sums of y and of y * y per 2 x 32 block.  A shift of 3 makes a padding position that took the
    affine show at once.  Same measured bound as above."""
    from emotiongestures_amd import _lib, ops
    from emotiongestures_amd.ops import _ptr, _stream
    lib = _lib.load()
    B, H, W = 2, 19, 66
    x, w, bias, _s, _t, _raw = _case(cin, cout, B, H, W)
    in_s, in_h = T("is", (cin,), 0.5, 1.5), T("ih", (cin,), 2.5, 3.5)
    xa = x.double() * in_s.double().view(1, -1, 1, 1) + in_h.double().view(1, -1, 1, 1)
    ref = F.relu(F.conv2d(xa, w.double(), bias.double(), stride=2, padding=1))
    d = dev()
    xg = x.permute(0, 2, 3, 1).contiguous().to(d)
    wp, bp, _, _ = ops.conv3x3_pack(w, bias, None, None, d)
    sg, hg = in_s.to(d), in_h.to(d)
    tiles = int(lib.eg_conv3x3_gap_tiles(H, W, cin, cout, 2))
    Ho, Wo = ref.shape[2], ref.shape[3]

    def run(form):
        y = torch.empty(B, Ho, Wo, cout, device=d)
        gap = torch.full((2, B, tiles, cout), float("nan"), device=d)
        with conv_s2(form):
            _lib.check(lib.eg_conv3x3_sq_in_affine(_ptr(xg), _ptr(sg), _ptr(hg), _ptr(wp), _ptr(bp), _ptr(y), _ptr(gap[0]), _ptr(gap[1]), B, H, W, cin,
                                                   cout, 2, 1, _lib.precision_code("bf16x3"), _stream(d)), "eg_conv3x3_sq_in_affine")
        return y.cpu().permute(0, 3, 1, 2).double(), gap.cpu().double()

    y_old, _ = run("interleaved")
    e_old = float((y_old - ref).abs().max())
    for form in FORMS[cin]:
        y, gap = run(form)
        e_new, e_l2 = float((y - ref).abs().max()), rel_l2(y.numpy(), ref.numpy())
        print(f"{cin}->{cout} input affine, squares, {form}: max |err| vs float64 {e_new:.3e} (interleaved {e_old:.3e}), rel_l2 {e_l2:.3e}")
        assert e_new <= 2 * e_old
        assert e_l2 < TOL["bf16x3"]
        assert torch.isfinite(gap).all()            # every partial of both planes is written
        assert rel_l2(gap[0].numpy(), _block_sums(ref).numpy()) < TOL["bf16x3"]
        assert rel_l2(gap[1].numpy(), _block_sums(ref * ref).numpy()) < TOL["bf16x3"]


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("layer", ["layer2", "layer3"])
def test_fused_stage_entry_block_on_planes_matches_the_operator_path(layer, prec):
    """eg_se_block_fused (the path the headline runs: conv1's partials feed se_gate_pre) with conv1 on planes, against the operator-by-operator block
    with conv1 in the interleaved form, and against the CPU oracle.  37 x 69 -> 19 x 35: partial last tile row and column."""
    from oracle import emogest_oracle as O
    m = build_mirror("spatial", 34, 126, 4, 4)
    blk = getattr(m.audio_encoder.feat_extractor, layer)[0]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = T("blk", (2, blk.conv1.weight.shape[1], 37, 69), -1, 1)
    ref = O.se_basic_block(sd, f"audio_encoder.feat_extractor.{layer}.0", x, blk.stride)
    blk.to(dev()).eval()
    blk.precision = prec
    with conv_s2("interleaved"):
        mod = blk(x.to(dev())).cpu()
    xg = x.to(dev()).permute(0, 2, 3, 1).contiguous()
    for form in FORMS[blk.conv1.weight.shape[1]]:
        with conv_s2(form):
            got = blk.forward_fused_nhwc(xg).permute(0, 3, 1, 2).contiguous().cpu()
        e_ref, e_mod = rel_l2(got.numpy(), ref.numpy()), rel_l2(got.numpy(), mod.numpy())
        print(f"{layer}.0 {prec} {form}: rel_l2 vs oracle {e_ref:.3e}, vs operator path {e_mod:.3e} (bound {TOL[prec] * 3:.1e})")
        assert got.shape == ref.shape
        assert e_ref < TOL[prec] * 3            # tests/test_gpu_block_entry.py's bound for the same block
        assert e_mod < TOL[prec] * 3
