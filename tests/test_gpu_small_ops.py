"""eg_conv1d, eg_layernorm / eg_layernorm_img and eg_melspectrogram on the GPU, each called directly at the shapes where such kernels go wrong,
element by element against the float64 restatements of tests/small_ops_f64.py (bounds, tolerances and cases are defined and justified there;
tests/test_small_ops.py shows on the CPU that they reject a fault confined to one channel group, tile edge, padding column, row or image slot).

Every output is a view into the middle of a larger buffer filled with a sentinel; after the call the guard regions on both sides must be
untouched (a store past lout, cout or rows lands there).  The same call through the Python operator (ops.conv1d, ops.layernorm, MelFrontEnd) must
return the same bits."""
import numpy as np
import pytest
import torch

import small_ops_f64 as S

pytestmark = pytest.mark.gpu

GUARD = 256                       # elements on each side of an output (a multiple of 16 bytes for every dtype in use)
SENTINEL = {torch.float32: -6.0e30, torch.int16: 0x5A5A, torch.uint8: 0xA5}
VARIANTS = [(0, False), (1, False), (1, True), (0, True)]          # (act, with scale / shift)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, (lambda: _stream(dev()))


def guarded(shape, dtype=torch.float32):
    """-> (buffer, view of `shape` in its middle), everything holding the sentinel."""
    numel = int(np.prod(shape))
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL[dtype], dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + numel].view(shape)


def guards_intact(buf, what):
    torch.cuda.synchronize()
    s = torch.tensor(SENTINEL[buf.dtype], dtype=buf.dtype, device=buf.device)
    assert bool((buf[:GUARD] == s).all()), f"{what}: a store in front of the output"
    assert bool((buf[-GUARD:] == s).all()), f"{what}: a store behind the output"


def untouched(buf, what):
    torch.cuda.synchronize()
    assert bool((buf == torch.tensor(SENTINEL[buf.dtype], dtype=buf.dtype, device=buf.device)).all()), f"{what}: the output was written"


# ---- conv1d ------------------------------------------------------------------------------------------------------------------------
def _conv1d_guarded(x, w, b, sc, sh, case, act):
    L, lib, _ptr, st = _api()
    n, cin, cout, lin, k, stride, pad = case
    buf, y = guarded((n, cout, max(1, (lin + 2 * pad - k) // stride + 1)))      # (a refused shape may have no output length of its own)
    rc = lib.eg_conv1d(_ptr(x), _ptr(w), _ptr(b), _ptr(sc), _ptr(sh), _ptr(y), n, cin, cout, lin, k, stride, pad, act, st())
    return rc, buf, y


@pytest.mark.parametrize("case", S.ALL_CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv1d_matches_float64_per_element(case):
    """conv1d_kernel<COG> (csrc/misc.hip) against conv1d_f64 within conv1d_bound, per element, per sample, per channel and per position: plain,
    with LeakyReLU, with LeakyReLU + affine, and with the affine alone (act == 0 with a scale applies the affine, include/emogest.h)."""
    from emotiongestures_amd import ops
    L = _api()[0]
    n, cin, cout, lin, k, stride, pad = case
    x, w, b, scale, shift = S.conv1d_inputs(case)
    xd, wd, bd, scd, shd = (t.to(dev()) for t in (x, w, b, scale, shift))
    for act, affine in VARIANTS:
        sc, sh = (scale, shift) if affine else (None, None)
        what = f"conv1d {case} act {act} affine {affine}"
        rc, buf, y = _conv1d_guarded(xd, wd, bd, scd if affine else None, shd if affine else None, case, act)
        L.check(rc, what)
        guards_intact(buf, what)
        ref = S.conv1d_f64(x, w, b, stride, pad, act, sc, sh)
        bound = S.conv1d_bound(x, w, b, stride, pad, act, sc, sh)
        whole, sl, el = S.compare_sliced(y, ref, bound, what, S.CONV_AXES)
        print(f"{what}: {whole:.3f} / {sl:.3f} / {el:.3f} of the bound (whole / worst slice / worst element)")
        y2 = ops.conv1d(xd, w, b, stride=stride, padding=pad, leaky=bool(act), scale=sc, shift=sh)
        assert torch.equal(y2, y), what + ": ops.conv1d differs from the direct call"


def test_conv1d_padding_only_outputs_are_post_bias():
    """pad > k: the outermost outputs see padding only; they equal post(bias) to the rounding of the epilogue."""
    case = (2, 4, 8, 20, 3, 1, 4)
    x, w, b, scale, shift = S.conv1d_inputs(case)
    xd, wd, bd, scd, shd = (t.to(dev()) for t in (x, w, b, scale, shift))
    rc, buf, y = _conv1d_guarded(xd, wd, bd, None, None, case, 0)
    assert rc == 0
    for pos in (0, 1, y.shape[2] - 2, y.shape[2] - 1):
        assert torch.equal(y[:, :, pos].cpu(), b.expand(2, 8))                  # no epilogue: the bias itself, bit for bit
    rc, buf, y = _conv1d_guarded(xd, wd, bd, scd, shd, case, 1)
    assert rc == 0
    post = S._post(b.double().view(1, -1, 1), 1, scale, shift).expand(2, 8, 1)
    for pos in (0, 1, y.shape[2] - 2, y.shape[2] - 1):
        assert float((y[:, :, pos:pos + 1].cpu().double() - post).abs().max()) <= 3 * S.U * 2.0      # |values| < 2, three roundings


def test_conv1d_status_codes():
    """Argument refusal launches nothing: the output keeps its sentinel.  A workgroup's LDS need above 160 KB is EG_ERR_UNSUPPORTED and the message
    names the byte count; scale without shift stays EG_ERR_BAD_ARG; act == 0 with scale + shift is accepted (and applied, see above)."""
    L, lib, _ptr, st = _api()
    case = (1, 2048, 64, 64, 9, 1, 4)
    n, cin, cout, lin, k, stride, pad = case
    x, w, b = torch.zeros(n, cin, lin, device=dev()), torch.zeros(cout, cin, k, device=dev()), torch.zeros(cout, device=dev())
    rc, buf, y = _conv1d_guarded(x, w, b, None, None, case, 1)
    assert rc == -2
    msg = lib.eg_last_error()
    assert b"LDS" in msg and str(S.conv_lds_bytes(cin, cout, k, stride)).encode() in msg, msg
    untouched(buf, "conv1d above 160 KB of LDS")
    small = (1, 4, 4, 8, 3, 1, 1)
    xs, ws, bs, sc, sh = (t.to(dev()) for t in S.conv1d_inputs(small))
    for act in (0, 1):
        rc, buf, y = _conv1d_guarded(xs, ws, bs, sc, None, small, act)
        assert rc == -1
        untouched(buf, "conv1d scale without shift")
        rc, buf, y = _conv1d_guarded(xs, ws, bs, None, sh, small, act)
        assert rc == -1
        untouched(buf, "conv1d shift without scale")
    rc, buf, y = _conv1d_guarded(xs, ws, bs, None, None, (1, 4, 4, 2, 5, 1, 0), 0)      # kernel longer than the padded input
    assert rc == -1
    untouched(buf, "conv1d kernel longer than the padded input")
    rc, buf, y = _conv1d_guarded(xs, ws, bs, sc, sh, small, 0)
    assert rc == 0


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _layernorm_guarded(x, g, b, eps, img_entry=False, images=None):
    """eg_layernorm, or (img_entry) eg_layernorm_img with `images` (a device tensor or None = NULL), into a guarded y."""
    L, lib, _ptr, st = _api()
    rows, d = x.shape
    buf, y = guarded((rows, d))
    if img_entry:
        rc = lib.eg_layernorm_img(_ptr(x), _ptr(g), _ptr(b), _ptr(y), _ptr(images), rows, d, eps, st())
    else:
        rc = lib.eg_layernorm(_ptr(x), _ptr(g), _ptr(b), _ptr(y), rows, d, eps, st())
    return rc, buf, y


@pytest.mark.parametrize("d", S.LN_VECTOR_D + S.LN_SCALAR_D)
def test_layernorm_matches_float64_per_element(d):
    """layernorm_kernel<NV> (D % 4 == 0; both sides of every NV threshold) and layernorm_any_kernel against layernorm_f64 per element, row and
    column, in units of layernorm_scale with the tolerance LN_TOL of the input class (4 x the float32 CPU error, small_ops_f64.py): uniform rows,
    rows with a common offset of 1e4, constant rows (the output is beta: variance 0, eps decides) and one spike of 1e3 among zeros.
    The constant class is why the kernels take their mean in two steps: with mean = sum / D alone, an fp32 evaluation in the kernels' summation
    order misses beta by up to 1.4e-3 |gamma| (67 x 2047: the mean's rounding error times 1 / sqrt(eps)), where torch's float32 result is exact."""
    from emotiongestures_amd import ops
    L = _api()[0]
    worst = {c: 0.0 for c in S.LN_CLASSES}
    for rows in S.ln_rows_for(d):
        for cls in S.LN_CLASSES:
            x, g, b = S.layernorm_inputs(rows, d, cls)
            xd, gd, bd = x.to(dev()), g.to(dev()), b.to(dev())
            for eps in S.LN_EPS:
                what = f"layernorm {rows} x {d} {cls} eps {eps:g}"
                rc, buf, y = _layernorm_guarded(xd, gd, bd, eps)
                L.check(rc, what)
                guards_intact(buf, what)
                unit = S.layernorm_scale(x, g, b, eps)
                ref = S.layernorm_f64(x, g, b, eps)
                err = float(((y.cpu().double() - ref).abs() / unit).max())
                worst[cls] = max(worst[cls], err)
                print(f"{what}: worst normalised error {err:.3e} (tolerance {S.LN_TOL[cls]:.3e})")
                S.compare_sliced(y, ref, S.LN_TOL[cls] * unit, what, S.LN_AXES)
                assert torch.equal(ops.layernorm(xd, gd, bd, eps), y), what + ": ops.layernorm differs from the direct call"
    print(f"layernorm D = {d}: worst normalised errors {worst}")


@pytest.mark.parametrize("d", [64, 512, 1024, 2048])
@pytest.mark.parametrize("rows", [1, 64, 65, 130])
def test_layernorm_images_are_the_split_of_the_row_output(rows, d):
    """eg_layernorm_img: the fp32 y is eg_layernorm's bit for bit, and the second output -- y as bf16 (hi, lo) tile-planar images, which every
    encoder product that consumes a normalised row reads -- is bit-equal to eg_split_tiles of that y (and to the CPU restatement images_of) on every
    slot of a real row; padding rows of the last 64-row tile are unspecified.  y_images = NULL is eg_layernorm."""
    L, lib, _ptr, st = _api()
    x, g, b = S.layernorm_inputs(rows, d, "uniform")
    xd, gd, bd = x.to(dev()), g.to(dev()), b.to(dev())
    mt = (rows + 63) // 64
    rc, buf0, y0 = _layernorm_guarded(xd, gd, bd, 1e-6)
    L.check(rc, "eg_layernorm")
    ibuf, img = guarded((2, mt, d // 8, 64, 8), torch.int16)
    rc, buf1, y1 = _layernorm_guarded(xd, gd, bd, 1e-6, True, img)
    L.check(rc, "eg_layernorm_img")
    guards_intact(buf1, "eg_layernorm_img y")
    guards_intact(ibuf, "eg_layernorm_img images")
    assert torch.equal(y1, y0)
    rc, buf2, y2 = _layernorm_guarded(xd, gd, bd, 1e-6, True, None)
    L.check(rc, "eg_layernorm_img without images")
    guards_intact(buf2, "eg_layernorm_img without images")
    assert torch.equal(y2, y0)
    sbuf, simg = guarded((2, mt, d // 8, 64, 8), torch.int16)
    L.check(lib.eg_split_tiles(_ptr(y1), d, rows, d, _ptr(simg), st()), "eg_split_tiles")
    guards_intact(sbuf, "eg_split_tiles")
    got, want = S.image_rows(img.cpu(), rows), S.image_rows(simg.cpu(), rows)
    for i, name in enumerate(("hi", "lo")):
        bad = (got[i] != want[i]).nonzero()
        assert bad.numel() == 0, f"{name} image differs from eg_split_tiles at (row, column) {bad[0].tolist()} ({bad.shape[0]} slots)"
    assert torch.equal(got, S.image_rows(S.images_of(y1.cpu()), rows)), "the images differ from the CPU restatement of the split"


def test_layernorm_refusals():
    """D = 2052 (> 2048) is EG_ERR_UNSUPPORTED; images with D = 96 (not a multiple of 64) EG_ERR_ALIGN; nothing is launched."""
    L, lib, _ptr, st = _api()
    for d, want_images, code in ((2052, False, -2), (2052, True, -2), (96, True, -5)):
        x, g, b = torch.zeros(3, d, device=dev()), torch.ones(d, device=dev()), torch.zeros(d, device=dev())
        ibuf, img = guarded((2, 64 * ((d + 63) // 64 * 64)), torch.int16)
        rc, buf, y = _layernorm_guarded(x, g, b, 1e-6, want_images, img if want_images else None)
        assert rc == code, (d, want_images, rc)
        assert lib.eg_last_error()
        untouched(buf, f"layernorm D = {d}")
        untouched(ibuf, f"layernorm images D = {d}")
    rc, buf, y = _layernorm_guarded(torch.zeros(3, 96, device=dev()), torch.ones(96, device=dev()), torch.zeros(96, device=dev()), 1e-6)
    assert rc == 0                                                      # D = 96 without images is fine


# ---- mel front-end -----------------------------------------------------------------------------------------------------------------
MEL = S.mel_inputs()
_front = {}


def _mel():
    from emotiongestures_amd.engine import MelFrontEnd
    if "mel" not in _front:
        _front["mel"] = MelFrontEnd(dev())
    return _front["mel"]


def _mel_guarded(audio, out_frames=None):
    """eg_melspectrogram with the front-end's tables into a guarded output (and a guarded workspace: the mel powers are [B, 128, frames])."""
    L, lib, _ptr, st = _api()
    mel = _mel()
    B, n = audio.shape
    of = 1 + n // 512 if out_frames is None else out_frames
    nbytes = int(lib.eg_mel_workspace_bytes(B, n))
    wbuf, ws = guarded((nbytes,), torch.uint8)
    buf, spec = guarded((B, 128, of))
    L.check(lib.eg_melspectrogram(_ptr(audio), B, n, _ptr(mel.fb), _ptr(mel.win), _ptr(mel.tw), _ptr(mel.band), _ptr(spec), of, _ptr(ws), nbytes,
                                  st()), "eg_melspectrogram")
    guards_intact(buf, "eg_melspectrogram output")
    guards_intact(wbuf, "eg_melspectrogram workspace")
    return spec


@pytest.mark.parametrize("name", sorted(MEL))
def test_melspectrogram_matches_oracle_on_edge_inputs(name):
    """mel_power_kernel / mel_db_kernel (csrc/mel.hip: two frames per complex FFT, a per-clip maximum across 16 waves) against the float64 oracle
    under the project's criterion -- at most one fp16 ulp, < 1 % of the bins differing, fp16-representable -- on: lengths that are the minimum, not
    a multiple of the hop, one short of / exactly a frame more; pure tones (every bin the oracle puts at the -80 dB floor is exactly -80); unit
    impulses on the window zero and the frame seams; a clip whose maximum lies in the frame out_frames cuts off; a batch of very different
    loudness (each row bit-equal to the clip alone); levels below and around amin."""
    from oracle import emogest_oracle as O
    audio, out_frames = MEL[name]
    B, n = audio.shape
    ad = torch.from_numpy(audio).to(dev())
    ref = O.melspectrogram(audio, out_frames=out_frames)
    spec = _mel_guarded(ad, out_frames)
    got = spec.cpu().numpy()
    assert got.shape == (B, 128, out_frames or 1 + n // 512)
    assert torch.equal(_mel()(ad, out_frames=out_frames), spec), name + ": MelFrontEnd differs from the direct call"
    diff = np.abs(got - ref)
    print(f"mel {name}: max |d| {diff.max():.4f} dB, {100 * float((diff > 0).mean()):.3f} % of bins differ, {100 * float((ref == -80).mean()):.1f} % at the floor")
    S.mel_criterion(got, ref, name)
    assert np.all(got[ref == -80.0] == -80.0), f"{name}: {int((got[ref == -80.0] != -80.0).sum())} floor bins are not at -80 dB"
    if name == "below_amin":
        assert np.all(got == 0.0)
    if B > 1:
        for i in range(B):
            alone = _mel_guarded(ad[i:i + 1].contiguous(), out_frames)
            assert torch.equal(alone[0], spec[i]), f"{name}: clip {i} depends on the batch it travels in"
    if name == "batch_loudness":
        assert np.all(got[3] == 0.0)
        assert np.abs(got[0] - got[1]).max() <= 0.0626      # the same clip 40 dB down (no bin near amin): the same dB relative to its own maximum
