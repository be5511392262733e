"""CPU tests of tests/small_ops_f64.py, the float64 restatements and bounds the GPU tests of eg_conv1d, eg_layernorm / eg_layernorm_img and
eg_melspectrogram (tests/test_gpu_small_ops.py) rely on: a result that is wrong in one channel group, one tile edge, one padding column, one row's
divisor or one image slot must be rejected under the loosest bound in use, a correct fp32 result must pass, and no mel input may ask for more than
an fp32 evaluation of the reference itself delivers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import small_ops_f64 as S
from oracle import emogest_oracle as O

VARIANTS = [(0, False), (1, False), (1, True), (0, True)]          # (act, with scale / shift)


def _conv(case, act, affine, x=None):
    n, cin, cout, lin, k, stride, pad = case
    x0, w, b, sc, sh = S.conv1d_inputs(case)
    sc, sh = (sc, sh) if affine else (None, None)
    x = x0 if x is None else x
    ref = S.conv1d_f64(x0, w, b, stride, pad, act, sc, sh)
    return x0, w, b, sc, sh, ref, S.conv1d_bound(x0, w, b, stride, pad, act, sc, sh)


def _rejected(got, ref, bound, what, axes):
    with pytest.raises(AssertionError):
        S.compare_sliced(got, ref, bound, what, axes)


# ---- conv1d ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ALL_CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv1d_float32_cpu_result_is_inside_the_bound(case):
    """The bound is a-priori (any summation order of the cin * k products in fp32): torch's own float32 convolution must sit inside it, and so must
    the float64 result itself."""
    n, cin, cout, lin, k, stride, pad = case
    for act, affine in VARIANTS:
        x, w, b, sc, sh, ref, bound = _conv(case, act, affine)
        assert ref.shape == (n, cout, (lin + 2 * pad - k) // stride + 1)
        y = TF.conv1d(x, w, b, stride=stride, padding=pad)
        y = TF.leaky_relu(y, 0.2) if act else y
        y = y * sc.view(1, -1, 1) + sh.view(1, -1, 1) if affine else y
        S.compare_sliced(y, ref, bound, f"conv1d {case} act {act} affine {affine}", S.CONV_AXES)
        S.compare_sliced(ref, ref, bound, "float64 against itself", S.CONV_AXES)


def test_conv1d_lds_request_of_the_cases():
    """What the cases are chosen for: every template instantiation, the third grid axis, a request above the 64 KB default and one the library
    refuses (tests/test_gpu_small_ops.py)."""
    assert {S.conv_cog(c[2]) for c in S.ALL_CONV_CASES} == {4, 8, 16}
    assert any(c[2] > 4 * S.conv_cog(c[2]) for c in S.CONV_CASES)
    assert 64 * 1024 < S.conv_lds_bytes(100, 128, 3, 2) <= 160 * 1024
    assert all(S.conv_lds_bytes(c[1], c[2], c[4], c[5]) <= 160 * 1024 for c in S.ALL_CONV_CASES)
    assert S.conv_lds_bytes(2048, 64, 9, 1) == 5308416 > 160 * 1024


# the loosest conv1d bounds in use are those of the largest cin * k: 378 (MotionAE's first layer), 300 (the 128 KB case), 192 and 102
@pytest.mark.parametrize("case", [(2, 10, 65, 66, 3, 1, 1), (1, 6, 130, 100, 3, 2, 1), (2, 100, 128, 150, 3, 2, 1)], ids=lambda c: "-".join(map(str, c)))
def test_conv1d_mutation_one_channel_at_a_group_boundary(case):
    """Output channel 4 * COG -- the first channel of the second workgroup on the third grid axis -- scaled by 1.001."""
    co = 4 * S.conv_cog(case[2])
    assert co < case[2]
    for act, affine in VARIANTS:
        *_, ref, bound = _conv(case, act, affine)
        got = ref.clone()
        got[:, co] *= 1.001
        _rejected(got, ref, bound, "scaled channel", S.CONV_AXES)
        whole, (sl, where), _ = S.sliced_errors(got, ref, bound, S.CONV_AXES)
        assert where == f"channel {co}"


@pytest.mark.parametrize("case", [(2, 126, 32, 34, 3, 1, 0), (2, 100, 128, 150, 3, 2, 1), (2, 7, 16, 65, 3, 1, 1), (2, 3, 8, 2, 5, 1, 2)],
                         ids=lambda c: "-".join(map(str, c)))
def test_conv1d_mutation_last_position_is_its_neighbour(case):
    for act, affine in VARIANTS:
        *_, ref, bound = _conv(case, act, affine)
        got = ref.clone()
        got[:, :, -1] = ref[:, :, -2]
        _rejected(got, ref, bound, "last position", S.CONV_AXES)
        whole, (sl, where), _ = S.sliced_errors(got, ref, bound, S.CONV_AXES)
        assert ref.shape[2] <= 8 or where == f"position {ref.shape[2] - 1}"      # (with two positions a channel slice can rank worse)


@pytest.mark.parametrize("case", [(2, 100, 128, 150, 3, 2, 1), (2, 34, 34, 512, 3, 1, 1), (2, 4, 32, 40, 8, 1, 7), (2, 4, 8, 20, 3, 1, 4)],
                         ids=lambda c: "-".join(map(str, c)))
def test_conv1d_mutation_input_shifted_inside_the_padding(case):
    """The input placed one sample late inside its padding (pad + 1 zeros in front, pad - 1 behind)."""
    n, cin, cout, lin, k, stride, pad = case
    for act, affine in VARIANTS:
        x, w, b, sc, sh, ref, bound = _conv(case, act, affine)
        xs = TF.pad(x, (pad + 1, pad - 1))
        got = S.conv1d_f64(xs, w, b, stride, 0, act, sc, sh)
        assert got.shape == ref.shape
        _rejected(got, ref, bound, "shifted input", S.CONV_AXES)


def test_conv1d_padding_only_outputs_equal_post_bias():
    """pad > k: the first and the last outputs see padding only, so they are post(bias) and their bound is a few roundings of |bias|."""
    case = (2, 4, 8, 20, 3, 1, 4)
    for act, affine in VARIANTS:
        x, w, b, sc, sh, ref, bound = _conv(case, act, affine)
        post = S._post(b.double().view(1, -1, 1), act, sc, sh).expand(2, 8, 1)
        for pos in (0, 1, ref.shape[2] - 2, ref.shape[2] - 1):
            assert torch.equal(ref[:, :, pos:pos + 1], post)
        if not affine:
            assert float((bound[:, :, 0] / b.double().abs().view(1, -1)).max()) <= (4 * 3 + 4 + 1) * S.U * (1 + 1e-12)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", S.LN_CLASSES)
def test_layernorm_float32_cpu_error_is_the_recorded_figure(cls):
    """LN_CPU_F32 is a measurement: torch's float32 CPU layer_norm against layernorm_f64 in units of layernorm_scale, worst over every case and
    eps of the GPU test.  It must not exceed the recorded figure, so that the GPU tolerance (LN_FACTOR x the figure) is what the file says."""
    worst = 0.0
    for rows, d in S.ln_cases():
        for eps in S.LN_EPS:
            x, g, b = S.layernorm_inputs(rows, d, cls)
            ref = S.layernorm_f64(x, g, b, eps)
            got = TF.layer_norm(x, (d,), g, b, eps)
            assert bool(torch.isfinite(got).all())
            worst = max(worst, float(((got.double() - ref).abs() / S.layernorm_scale(x, g, b, eps)).max()))
            if cls == "constant":
                assert torch.equal(ref, b.double().expand(rows, d))
    print(f"layer_norm float32 CPU, class {cls}: worst normalised error {worst:.3e} (recorded {S.LN_CPU_F32[cls]:.3e})")
    assert worst <= S.LN_CPU_F32[cls]
    assert S.LN_TOL[cls] == 4.0 * S.LN_CPU_F32[cls]


def test_layernorm_cases_cover_every_kernel_path():
    cases = S.ln_cases()
    ds = {d for _, d in cases}
    assert ds == set(S.LN_VECTOR_D + S.LN_SCALAR_D)
    for lo, hi in ((256, 260), (512, 516), (1024, 1028)):      # both sides of the NV = 1 | 2 | 4 | 8 thresholds
        assert lo in ds and hi in ds
    for d in ds:
        assert {5, 67} <= {r for r, dd in cases if dd == d}
    for d in (512, 282):
        assert {r for r, dd in cases if dd == d} == set(S.LN_ROWS)


def _ln_wrong_divisor(x, g, b, eps, row):
    """layernorm_f64 with row `row` normalised over D - 1: mean = sum / (D - 1), variance = sum (x - mean)^2 / (D - 1)."""
    ref = S.layernorm_f64(x, g, b, eps)
    d = x.shape[1]
    xr = x[row].double()
    mean = xr.sum() / (d - 1)
    var = (xr - mean).pow(2).sum() / (d - 1)
    got = ref.clone()
    got[row] = (xr - mean) / torch.sqrt(var + eps) * g.double() + b.double()
    return got, ref


@pytest.mark.parametrize("cls", S.LN_CLASSES)
@pytest.mark.parametrize("rows,d", [(5, 2048), (67, 512), (5, 282), (130, 2047)])
def test_layernorm_mutation_one_row_with_the_wrong_divisor(rows, d, cls):
    """One row normalised with D - 1 in place of D, at the widest rows (where it changes least: 2.4e-4 of z at D = 2048), in every input class under
    that class's own tolerance -- the loosest, the offset class's 1.3e-2, sees it through the mean (1e4 / (D - 1) against a spread of 1.7)."""
    for eps in S.LN_EPS:
        x, g, b = S.layernorm_inputs(rows, d, cls)
        row = rows - 2 if rows > 2 else rows - 1
        got, ref = _ln_wrong_divisor(x, g, b, eps, row)
        bound = S.LN_TOL[cls] * S.layernorm_scale(x, g, b, eps)
        S.compare_sliced(ref, ref, bound, "float64 against itself", S.LN_AXES)
        _rejected(got, ref, bound, "wrong divisor", S.LN_AXES)
        _, (sl, where), (el, idx) = S.sliced_errors(got, ref, bound, S.LN_AXES)
        assert idx[0] == row and (where == f"row {row}" or where.startswith("column"))      # (the spike's column can rank above its row)


@pytest.mark.parametrize("cls", S.LN_CLASSES)
def test_layernorm_float32_cpu_result_passes_the_gpu_tolerance(cls):
    for rows, d in ((5, 2048), (67, 516), (130, 282), (3, 1)):
        x, g, b = S.layernorm_inputs(rows, d, cls)
        S.compare_sliced(TF.layer_norm(x, (d,), g, b, 1e-6), S.layernorm_f64(x, g, b, 1e-6), S.LN_TOL[cls] * S.layernorm_scale(x, g, b, 1e-6),
                         f"layer_norm float32 {rows} x {d} {cls}", S.LN_AXES)


# ---- images ------------------------------------------------------------------------------------------------------------------------
IMG_AXES = ("image", "row", "column")


@pytest.mark.parametrize("rows,d", [(1, 64), (65, 128), (130, 512)])
def test_images_slot_map_and_split(rows, d):
    """images_of against the header's sentence, element by element: (r, c) at [r // 64][c // 8][r % 64][c % 8] of each image, hi then lo;
    hi + lo reconstruct y to 2^-16 relative."""
    y = S.T(f"img{rows}x{d}", (rows, d), -3, 3)
    img = S.images_of(y)
    mt, ko = (rows + 63) // 64, d // 8
    assert img.shape == (2, mt, ko, 64, 8) and img.dtype == torch.int16
    flat = img.reshape(2, -1)
    hi, lo = S.split_bf16(y)
    rng = np.random.RandomState(rows + d)
    for r, c in [(0, 0), (rows - 1, d - 1), (rows - 1, 0), (0, d - 1)] + [(int(rng.randint(rows)), int(rng.randint(d))) for _ in range(200)]:
        slot = (((r >> 6) * ko + (c >> 3)) * 64 + (r & 63)) * 8 + (c & 7)
        assert flat[0, slot] == hi[r, c] and flat[1, slot] == lo[r, c], (r, c)
    back = S.image_rows(img, rows)
    assert torch.equal(back[0], hi) and torch.equal(back[1], lo)
    rec = hi.view(torch.bfloat16).float() + lo.view(torch.bfloat16).float()
    assert float(((rec - y).abs() / y.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    assert torch.equal(img.permute(0, 1, 3, 2, 4).reshape(2, mt * 64, d)[:, rows:], torch.zeros(2, mt * 64 - rows, d, dtype=torch.int16))


@pytest.mark.parametrize("rows,d", [(2, 64), (65, 128), (130, 512)])
def test_images_mutation_one_octet_in_the_neighbouring_rows_slot(rows, d):
    y = S.T(f"img{rows}x{d}", (rows, d), -3, 3)
    ref = S.images_of(y)
    S.compare_sliced(S.image_rows(ref, rows), S.image_rows(ref, rows), 0.0, "images against themselves", IMG_AXES)
    for image in (0, 1):
        got = ref.clone()
        r, o = rows - 1, (d // 8) - 1
        got[image, r >> 6, o, (r & 63) - 1] = ref[image, r >> 6, o, r & 63]      # the octet of row r lands in row r - 1's slot
        got[image, r >> 6, o, r & 63] = 0
        assert not torch.equal(S.image_rows(got, rows), S.image_rows(ref, rows))
        _rejected(S.image_rows(got, rows), S.image_rows(ref, rows), 0.0, "misplaced octet", IMG_AXES)


# ---- mel front-end -----------------------------------------------------------------------------------------------------------------
MEL = S.mel_inputs()


@pytest.mark.parametrize("name", sorted(MEL))
def test_mel_float32_reference_stays_inside_the_criterion(name):
    """A float32 evaluation of the oracle's restatement (torch.fft.rfft on float32 frames, float32 filterbank product, float32 log) against the
    float64 oracle, under the criterion the kernel is held to: an input that breaks it here would ask the kernel for more than fp32 gives."""
    audio, out_frames = MEL[name]
    ref = O.melspectrogram(audio, out_frames=out_frames)
    got, _ = S.mel_restated(audio, out_frames, torch.float32)
    worst, frac = S.mel_criterion(got, ref, name)
    print(f"mel float32 reference, {name}: max |d| {worst:.4f} dB, {100 * frac:.3f} % of bins differ")
    assert ref.shape == (audio.shape[0], 128, out_frames or 1 + audio.shape[1] // 512)
    assert np.all(got[ref == -80.0] == -80.0)          # bins at the floor stay at the floor in float32


def test_mel_inputs_are_what_they_are_for():
    for n in S.MEL_LENGTHS:
        assert MEL[f"len{n}"][0].shape == (1, n)
    assert [1 + n // 512 for n in S.MEL_LENGTHS] == [2, 2, 2, 3, 3, 32]
    for hz in S.MEL_TONES_HZ:                            # a pure tone: most bins sit at the -80 dB floor
        ref = O.melspectrogram(MEL[f"tone{hz:g}"][0])
        assert 0.5 < float((ref == -80.0).mean()) < 1.0 and ref.max() == 0.0
    audio, out_frames = MEL["loud_dropped_frame"]        # the clip maximum lies in the frame that out_frames cuts off
    _, mel = S.mel_restated(audio, None, torch.float64)
    assert mel.shape[2] == 33 and out_frames == 32
    assert int(mel[0].max(dim=0).values.argmax()) == 32
    assert float(mel[0, :, 32].max() / mel[0, :, :31].max()) > 1e3
    assert O.melspectrogram(audio, out_frames=32).max() < -6.0          # (frame 31 holds the loud tail under its window's last quarter)
    _, mel = S.mel_restated(MEL["below_amin"][0], None, torch.float64)
    assert float(mel.max()) < 1e-10 and np.all(O.melspectrogram(MEL["below_amin"][0]) == 0.0)
    _, mel = S.mel_restated(MEL["around_amin"][0], None, torch.float64)
    assert 0.05 < float((mel > 1e-10).double().mean()) < 0.95
    batch = MEL["batch_loudness"][0]
    assert batch.shape[0] == 4 and not batch[3].any() and np.all(O.melspectrogram(batch)[3] == 0.0)
