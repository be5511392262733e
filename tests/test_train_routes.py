"""CPU-only: the route functions of the training tower (train/functional.py: conv3x3_route, batch_norm_route, se_tail_route) are pure -- shapes,
flags, the precision code and the module switches in, names out -- so which kernels a training step runs is checked here without a GPU and
without the library.  The tables below are written out by hand from the dispatch cascades as they stood before the route functions existed
(commit f396f39) and from the case table above test_tower_shapes_backward_matches_float64; nothing in them is computed by the code under test."""
import itertools

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from emotiongestures_amd.train import functional as F

F32, BF = 0, 1          # EG_PREC_F32, EG_PREC_BF16X3 (include/emogest.h)
R = F.ConvRoute


@pytest.fixture(autouse=True)
def _no_library_and_default_switches(monkeypatch):
    def refuse():
        raise AssertionError("a route function loaded the library")
    monkeypatch.setattr(F, "_lib", refuse)
    for name, value in (("PAD_WGRAD", True), ("S2_WGRAD", True), ("S2_DGRAD", True), ("DEFER_BN_APPLY", True), ("DEFER_BN_MIN_NUMEL", 12 << 20),
                        ("SE_TAIL_RELU_BITS", True)):
        monkeypatch.setattr(F, name, value)


# The conv3x3 call sites of train/nets.py with the flags their callers pass:
#   (cin, cout, stride, has_bias, relu, in_affine, want_gap, need_dx, passthrough)
def _conv1(c):          # se_basic_block's conv1 of an identity block: ReLU, pooling partials, the block input's alias
    return (c, c, 1, False, True, False, True, True, True)


def _conv2(c, aff=False):       # conv2 of every block (aff: behind a deferred bn1)
    return (c, c, 1, False, False, aff, True, True, False)


def _entry(ci, co):     # conv1 of a stage's stride-2 entry block: the second consumer is the strided 1x1 shortcut
    return (ci, co, 2, False, True, False, True, True, "sub")


def _final(frames):     # audio_encoder_forward's final_conv1 128 -> frames, with bias, no ReLU
    return (128, frames, 1, True, False, False, False, True, False)


SITES = {"stem": (1, 32, 1, True, True, False, False, False, False)}          # resnetse_forward: the spectrogram takes no gradient
for _c in (32, 64, 128, 256):
    SITES[f"conv1-{_c}"], SITES[f"conv2-{_c}"], SITES[f"conv2-{_c}-affine"] = _conv1(_c), _conv2(_c), _conv2(_c, True)
for _ci, _co in ((32, 64), (64, 128), (128, 256)):
    SITES[f"entry-{_ci}-{_co}"] = _entry(_ci, _co)
for _f in (34, 60, 120):
    SITES[f"final-{_f}"] = _final(_f)

_COL = R("nhwc", "implicit_gemm", "col2im", 1, False, False, False)
DEFAULT = {
    F32: {
        "stem": R("stem", "im2col", "none", 0, False, False, False),
        **{f"conv1-{c}": R("nhwc", "implicit_gemm", "rotated", 1, True, False, True) for c in (32, 64, 128, 256)},
        **{f"conv2-{c}": R("nhwc", "implicit_gemm", "rotated", 1, False, False, False) for c in (32, 64, 128, 256)},
        **{f"conv2-{c}-affine": "EgError" for c in (32, 64, 128, 256)},           # the deferred BatchNorm apply is split-bf16 only
        "entry-32-64": _COL, "entry-64-128": _COL, "entry-128-256": _COL,
        "final-34": R("channel_major", "implicit_gemm", "col2im", 0, False, False, False),
        "final-60": R("nhwc", "implicit_gemm", "col2im", 0, False, False, False),
        "final-120": R("nhwc", "implicit_gemm", "col2im", 0, False, False, False),
    },
    BF: {
        "stem": R("stem", "im2col", "none", 0, False, False, False),
        **{f"conv1-{c}": R("sq", "mfma", "rotated", 2, True, False, True) for c in (32, 64, 128, 256)},
        **{f"conv2-{c}": R("sq", "mfma", "rotated", 2, False, False, False) for c in (32, 64, 128, 256)},
        **{f"conv2-{c}-affine": R("sq_in_affine", "mfma_in_affine", "rotated", 2, False, False, False) for c in (32, 64, 128, 256)},
        **{f"entry-{a}-{b}": R("sq", "gather_mfma", "s2", 2, False, True, False) for a, b in ((32, 64), (64, 128), (128, 256))},
        "final-34": R("channel_major", "mfma_padded", "rotated_padded", 0, False, False, False),
        "final-60": R("nhwc", "mfma_padded", "rotated_padded", 0, False, False, False),
        "final-120": R("nhwc", "mfma_padded", "col2im", 0, False, False, False),           # 120 > 64: the padded rotated filter does not take it
    },
}
# What each switch changes when it is OFF (everything not listed stays as in DEFAULT; none of them touches an f32 route)
SWITCHED_OFF = {
    "PAD_WGRAD": {"final-34": R("channel_major", "implicit_gemm", "col2im", 0, False, False, False),
                  "final-60": R("nhwc", "implicit_gemm", "col2im", 0, False, False, False),
                  "final-120": R("nhwc", "implicit_gemm", "col2im", 0, False, False, False)},
    "S2_WGRAD": {f"entry-{a}-{b}": R("sq", "implicit_gemm", "s2", 2, False, True, False) for a, b in ((32, 64), (64, 128), (128, 256))},
    "S2_DGRAD": {f"entry-{a}-{b}": R("sq", "gather_mfma", "col2im", 2, False, False, False) for a, b in ((32, 64), (64, 128), (128, 256))},
}


def _route_or_error(site, prec):
    cin, cout, stride, has_bias, relu, aff, want_gap, need_dx, through = SITES[site]
    try:
        return F.conv3x3_route(cin, cout, stride, prec, has_bias, relu, aff, want_gap, need_dx, through)
    except F.L.EgError:
        return "EgError"


@pytest.mark.parametrize("off", [None, "PAD_WGRAD", "S2_WGRAD", "S2_DGRAD"])
@pytest.mark.parametrize("prec", [F32, BF], ids=["f32", "bf16x3"])
def test_routes_of_every_tower_call_site(prec, off, monkeypatch):
    assert set(DEFAULT[prec]) == set(SITES)
    expect = dict(DEFAULT[prec])
    if off is not None:
        monkeypatch.setattr(F, off, False)
        if prec == BF:
            expect.update(SWITCHED_OFF[off])
    got = {site: _route_or_error(site, prec) for site in SITES}
    assert got == expect, {s: (got[s], expect[s]) for s in SITES if got[s] != expect[s]}


FORWARD = {"sq_in_affine", "sq", "nhwc", "channel_major", "stem", "im2col"}
WGRAD = {"mfma_in_affine", "mfma", "mfma_padded", "gather_mfma", "implicit_gemm", "im2col"}
DGRAD = {"rotated", "rotated_padded", "s2", "col2im", "none"}
SPLIT_ONLY = {"sq_in_affine", "sq", "mfma_in_affine", "mfma", "mfma_padded", "gather_mfma", "rotated_padded", "s2"}


def test_route_invariants_over_the_grid(monkeypatch):
    n = 0
    for pad, s2w, s2d in itertools.product((True, False), repeat=3):
        monkeypatch.setattr(F, "PAD_WGRAD", pad)
        monkeypatch.setattr(F, "S2_WGRAD", s2w)
        monkeypatch.setattr(F, "S2_DGRAD", s2d)
        for cin, cout, stride, prec in itertools.product((1, 3, 4, 32, 64, 128, 256), (8, 32, 34, 60, 64, 120, 128, 256), (1, 2), (F32, BF)):
            for has_bias, relu, aff, want_gap, need_dx, through in itertools.product(*[(False, True)] * 5, (False, True, "sub")):
                args = (cin, cout, stride, prec, has_bias, relu, aff, want_gap, need_dx, through)
                try:
                    r = F.conv3x3_route(*args)
                except F.L.EgError:
                    assert aff, args                                # only a deferred BatchNorm in front is refused with EgError ...
                    continue
                except ValueError:
                    assert want_gap and not aff, args               # ... and pooling partials from a route that emits none with ValueError
                    continue
                n += 1
                assert r.forward in FORWARD and r.wgrad in WGRAD and r.dgrad in DGRAD and r.gap_planes in (0, 1, 2), (args, r)
                assert all(isinstance(v, bool) for v in (r.adds_full, r.adds_quarter, r.masks_bits)), (args, r)
                assert (r.forward == "sq_in_affine") == (r.wgrad == "mfma_in_affine") == bool(aff), (args, r)
                assert (r.gap_planes in (1, 2)) == bool(want_gap), (args, r)
                assert (r.dgrad == "none") == (not need_dx), (args, r)
                assert not r.masks_bits or (r.dgrad == "rotated" and through is True), (args, r)
                assert not r.adds_full or (r.dgrad in ("rotated", "rotated_padded") and through), (args, r)
                assert not r.adds_quarter or (r.dgrad == "s2" and through == "sub"), (args, r)
                assert not (r.adds_full and r.adds_quarter), (args, r)
                if prec == F32:
                    assert not {r.forward, r.wgrad, r.dgrad} & SPLIT_ONLY, (args, r)
    assert n > 50000


def test_batch_norm_route_at_the_deferral_threshold(monkeypatch):
    big, small = 25 * 128 * 124 * 32, 16 * 128 * 124 * 32
    assert small < 12 << 20 <= big
    assert F.batch_norm_route(True, BF, 2, 32, 4, big) == "deferred"
    assert F.batch_norm_route(True, BF, 2, 32, 4, small) == "from_squares"
    assert F.batch_norm_route(False, BF, 2, 32, 4, big) == "from_squares"                   # only where the caller allows it
    for planes, name in ((0, "two_pass"), (1, "from_sums"), (2, "from_squares")):
        for numel in (small, big):
            assert F.batch_norm_route(True, F32, planes, 32, 4, numel) == name              # f32 never defers
    assert F.batch_norm_route(True, BF, 1, 32, 4, big) == "from_sums"                       # needs the squares
    assert F.batch_norm_route(True, BF, 2, 96, 4, big) == "from_squares"                    # 256 % 96 != 0
    assert F.batch_norm_route(True, BF, 0, 32, 2, big) == "two_pass"
    monkeypatch.setattr(F, "DEFER_BN_APPLY", False)
    assert F.batch_norm_route(True, BF, 2, 32, 4, big) == "from_squares"


def test_se_tail_route(monkeypatch):
    assert F.se_tail_route(2, 2 * 12 * 20 * 32) == ("from_squares", True)
    assert F.se_tail_route(1, 2 * 12 * 20 * 32) == ("from_sums", True)
    assert F.se_tail_route(1, 2 * 3 * 5 * 8) == ("from_sums", False)            # 240 elements: no whole 32-element bit words
    monkeypatch.setattr(F, "SE_TAIL_RELU_BITS", False)
    assert F.se_tail_route(2, 2 * 12 * 20 * 32) == ("from_squares", False)
