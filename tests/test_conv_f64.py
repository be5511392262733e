"""CPU-only: tests/conv_f64.py rejects the errors a 3x3 convolution kernel makes, and the whole-tensor relative L2 of
tests/test_gpu_kernels.py (TOL per precision) does not.  Each mutation is applied to a float64 reference and handed to the helper as "the
kernel's output".

What the old norm accepts depends on how much of the tensor an error touches, so the acceptance is asserted where it holds and the opposite
where it does not (measured here, 32 -> 32, batch 2, 9 x 1025):
  one tap left out of the last column             helper rejects; rel_l2 8.3e-3 .. 9.1e-3 < TOL[bf16]
  one pixel of tile 1 taken from tile 0           helper rejects; rel_l2 1.2e-2 < TOL[bf16]
  channels cout-1 and cout-2 swapped              helper rejects; over the whole map rel_l2 is 0.33 and the old norm rejects it too.  Swapped in the
                                                  one-column last tile only (what a padded channel tile stored wrong in a partial tile looks like):
                                                  helper rejects, rel_l2 1.1e-2 < TOL[bf16]
  two tiles' partials exchanged                   helper rejects; the old check sums the partials over the tiles first: error exactly 0
  xl*wl added back to bf16x3                      helper accepts (against stated and against true)
  wh*xl left out of bf16x3                        helper rejects; rel_l2 1.5e-3 is above TOL[bf16x3] = 3e-5 (the old norm sees this one) and below TOL[bf16]
"""
import pytest
import torch

import conv_f64 as C

CIN = COUT = 32
B, H, W = 2, 9, 1025          # 33 column tiles, the last one a single column: an error confined to one column stays under 2e-2 of the whole norm


@pytest.fixture(scope="module")
def wide():
    x, w, bias, scale, shift, raw = C.case(CIN, COUT, 1, B, H, W)
    return x, w, bias, scale, shift, raw


def _ref(raw, prec, bias, scale, shift):
    ref = C.epilogue(raw.stated[prec], bias, True, scale, shift)
    A = C.epilogue_abs(raw.abs, bias, scale, shift)
    return ref, C.elem_bound(prec, CIN, A, ref)


def _rejected(got, ref, bound):
    with pytest.raises(AssertionError):
        C.check_map(got, ref, bound, "mutation")


def test_the_reference_passes_its_own_check_and_an_fp32_evaluation_stays_far_inside(wide):
    x, w, bias, scale, shift, raw = wide
    for prec in ("f32", "bf16", "bf16x3"):
        ref, bound = _ref(raw, prec, bias, scale, shift)
        assert C.check_map(ref.clone(), ref, bound, prec) == 0.0
    # the stated f32 sum evaluated in fp32 by torch: a correct kernel's kind of error
    got = torch.nn.functional.conv2d(x, w, bias, padding=1).relu() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref, bound = _ref(raw, "f32", bias, scale, shift)
    r = C.check_map(got.double(), ref, bound, "fp32 torch")
    print(f"fp32 evaluation of the stated sum: worst error / bound {r:.3g}")
    assert r < 0.25


@pytest.mark.parametrize("kh,kw", [(0, 0), (1, 1), (2, 1)])
def test_a_tap_left_out_of_the_last_column(wide, kh, kw):
    x, w, bias, scale, shift, raw = wide
    # the tap's own contribution to the last output column: input column W - 1 + kw - 1 (kw = 2 reads the padding: nothing to leave out)
    xs = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))[:, :, kh:kh + H, W - 1 + kw:W + kw]
    tap = torch.einsum("bchw,oc->bohw", xs, w.double()[:, :, kh, kw])
    for prec in ("f32", "bf16"):
        ref, bound = _ref(raw, prec, bias, scale, shift)
        acc = raw.stated[prec].clone()
        acc[:, :, :, -1:] -= tap
        got = C.epilogue(acc, bias, True, scale, shift)
        _rejected(got, ref, bound)
    e = C.rel_l2(got, ref)
    print(f"tap ({kh}, {kw}) left out of the last column: rel_l2 {e:.3e}")
    assert e < C.TOL["bf16"]


def test_channels_swapped(wide):
    x, w, bias, scale, shift, raw = wide
    ref, bound = _ref(raw, "bf16", bias, scale, shift)
    got = ref.clone()
    got[:, [COUT - 1, COUT - 2]] = ref[:, [COUT - 2, COUT - 1]]
    _rejected(got, ref, bound)
    e_all = C.rel_l2(got, ref)
    assert e_all >= C.TOL["bf16"]         # over the whole map the old norm sees the swap as well
    got = ref.clone()
    got[:, [COUT - 1, COUT - 2], :, -1] = ref[:, [COUT - 2, COUT - 1], :, -1]
    _rejected(got, ref, bound)
    e = C.rel_l2(got, ref)
    print(f"channels {COUT - 1} and {COUT - 2} swapped: whole map rel_l2 {e_all:.3e}, last column tile only {e:.3e}")
    assert e < C.TOL["bf16"]


def test_a_pixel_of_the_second_tile_taken_from_the_first(wide):
    x, w, bias, scale, shift, raw = wide
    ref, bound = _ref(raw, "bf16", bias, scale, shift)
    got = ref.clone()
    got[:, :, 4, 32 + 7] = ref[:, :, 4, 7]
    _rejected(got, ref, bound)
    e = C.rel_l2(got, ref)
    print(f"one pixel of tile 1 from tile 0: rel_l2 {e:.3e}")
    assert e < C.TOL["bf16"]


def test_partials_of_two_tiles_exchanged(wide):
    x, w, bias, scale, shift, raw = wide
    for prec in ("f32", "bf16x3", "bf16"):
        ref, bound = _ref(raw, prec, bias, scale, shift)
        good = C.tile_sums(ref, 4)
        assert good.shape == (B, 3 * 33, COUT)
        assert C.check_partials(good.clone(), ref, bound, 4, "partials") == 0.0
        bad = good.clone()
        bad[:, [5, 6]] = good[:, [6, 5]]
        with pytest.raises(AssertionError):
            C.check_partials(bad, ref, bound, 4, "exchanged")
        # tests/test_gpu_kernels.py: rel_l2(gap.sum(1), ref.sum((2, 3))) < max(TOL, 1e-5)
        assert C.rel_l2(bad.sum(1), ref.sum((2, 3))) < 1e-12
        with pytest.raises(AssertionError):          # one tile height too many: a partial filed under another tile
            C.check_partials(C.tile_sums(ref, 8), ref, bound, 4, "8-row tiles")


def test_the_split_terms(wide):
    x, w, bias, scale, shift, raw = wide
    A = raw.abs
    for against in ("stated", "true"):
        ref = raw.stated["bf16x3"] if against == "stated" else raw.true
        bound = C.elem_bound("bf16x3", CIN, A, ref, against)
        r = C.check_map(raw.stated["bf16x3"] + raw.dropped(), ref, bound, f"xl*wl added back, against {against}")
        print(f"xl*wl added back, against {against}: worst error / bound {r:.3g}")
        _rejected(raw.terms3["hh"] + raw.terms3["hl"], ref, bound)           # wh*xl left out
    e = C.rel_l2(raw.terms3["hh"] + raw.terms3["hl"], raw.true)
    print(f"wh*xl left out: rel_l2 {e:.3e}")
    assert C.TOL["bf16x3"] <= e < C.TOL["bf16"]          # the one mutation the old norm sees at its own precision


def test_stated_bf16x3_is_within_the_split_term_of_the_true_convolution_on_the_gpu_shapes():
    worst = 0.0
    for name, (cin, stride, rows, couts) in C.ROUTE_CASES.items():
        cout = couts[len(couts) // 2]
        for (b, h, w, ho, wo) in C.route_maps(rows, stride):
            raw = C.case(cin, cout, stride, 1, h, w)[5]
            assert raw.true.shape[2:] == (ho, wo)
            r = float(((raw.stated["bf16x3"] - raw.true).abs() / (C.SPLIT_TERM * raw.abs)).max())
            worst = max(worst, r)
            assert r <= 1.0, (name, cout, h, w, r)
    print(f"|stated(bf16x3) - true| / (3 * 2^-16 * A): worst {worst:.3g}")


def test_route_maps_cover_the_tile_edges_and_both_input_parities():
    for rows in (2, 4, 8):
        assert [(ho, wo) for _b, _h, _w, ho, wo in C.route_maps(rows, 1)] == [(3, 5), (rows, 32), (rows + 1, 33), (2 * rows + 1, 65)]
        s2 = C.route_maps(rows, 2)
        assert [((h - 1) // 2 + 1, (w - 1) // 2 + 1) for _b, h, w, _ho, _wo in s2] == [(ho, wo) for *_x, ho, wo in s2]
        assert {h % 2 for _b, h, *_r in s2} == {0, 1} and {w % 2 for _b, _h, w, *_r in s2} == {0, 1}
        assert {b for b, *_r in s2} == {1, 3}
