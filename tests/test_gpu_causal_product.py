"""The causal two-tap convolution as ONE pre-split product (eg_linear_presplit_causal: [tap 0 on rows r - d | tap 1 on rows r] in one K chain) and the
producer-side images of the two adds (eg_add_rows_split), against float64 numpy and against the two-launch / fp32-input paths they replace."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
from emotiongestures_amd.synth import hash_uniform

pytestmark = pytest.mark.gpu

PERIOD, C, CPAD = 60, 300, 320          # text_len, TCN channels, channels padded to the image width (zero tail octets)
FLAGS = [(False, False, False), (True, True, False), (True, True, True)]       # bias, relu, res2


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def T(key, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(hash_uniform(key, shape, lo, hi, 0))


@functools.lru_cache(maxsize=None)
def operands(M):
    return T("cx", (M, C)), T("cw0", (C, C), -0.1, 0.1), T("cw1", (C, C), -0.1, 0.1), T("cb", (C,)), T("cr", (M, C))


@functools.lru_cache(maxsize=None)
def reference(M, d, bias, relu, res2):
    """float64: y[r] = epi(b + W0 x[r - d] + W1 x[r]), x[r - d] = 0 for (r mod PERIOD) < d."""
    x, w0, w1, b, r = (t.double().numpy() for t in operands(M))
    xs = np.zeros_like(x)
    rows = np.arange(M)
    ok = (rows % PERIOD) >= d
    xs[ok] = x[rows[ok] - d]
    y = xs @ w0.T + x @ w1.T
    if bias:
        y = y + b
    if relu:
        y = np.maximum(y, 0)
    if res2:
        y = np.maximum(y + r, 0)
    return y


def packed_taps(w0, w1):
    from emotiongestures_amd import packing
    cat = torch.zeros(C, 2 * CPAD)
    cat[:, :C] = w0
    cat[:, CPAD:CPAD + C] = w1
    return torch.from_numpy(packing._pack_linear(cat, CPAD, 2 * CPAD)).to(dev())


def split_images(xd, M, K):
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    kp, mt = (K + 63) // 64 * 64, (M + 63) // 64
    img = torch.empty(2 * mt * 64 * kp, dtype=torch.int16, device=dev())
    L.check(L.load().eg_split_tiles(_ptr(xd), K, M, K, _ptr(img), _stream(dev())), "eg_split_tiles")
    return img


def one_launch(M, d, w0, w1, bias, relu, res2, tile, monkeypatch):
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    x, _w0, _w1, b, r = operands(M)
    xd = x.to(dev())
    img = split_images(xd, M, C)
    wp = packed_taps(w0, w1)
    bp = torch.zeros(CPAD, device=dev())
    bp[:C] = b.to(dev())
    rd = r.to(dev())
    zero = torch.zeros(CPAD * 32, device=dev())                    # CPAD * 128 bytes
    y = torch.full((M, C), float("nan"), device=dev())
    monkeypatch.setenv("EG_GEMM_TILE", tile)
    L.check(L.load().eg_linear_presplit_causal(_ptr(img), CPAD, _ptr(zero), _ptr(wp), 2 * CPAD, _ptr(bp) if bias else None, _ptr(rd) if res2 else None, C,
                                               _ptr(y), C, None, 0, M, C, CPAD, int(relu), d, PERIOD, L.precision_code("bf16x3"), _stream(dev())),
            "eg_linear_presplit_causal")
    torch.cuda.synchronize()
    monkeypatch.delenv("EG_GEMM_TILE")
    return y.cpu()


def two_launches(M, d, bias, relu, res2):
    """The path the one-launch product replaces: the shifted tap, then the plain tap on top of it (res1)."""
    from emotiongestures_amd import ops
    x, w0, w1, b, r = operands(M)
    xd = x.to(dev())
    h = ops.linear(xd, w0, b if bias else None, a_shift=d, a_seq=PERIOD, precision="bf16x3")
    return ops.linear(xd, w1, None, res1=h, res2=r.to(dev()) if res2 else None, relu=relu, precision="bf16x3").cpu()


@pytest.mark.parametrize("tile", ["64", "128"])
@pytest.mark.parametrize("M,d", [(180, 1), (180, 2), (180, 4), (61, 2)])
def test_causal_product_matches_fp64(M, d, tile, monkeypatch):
    """3 clips x 60 rows = 180: the last 64-row tile is partial, rows 64 and 128 are tile boundaries inside a clip (their shifted source lies in
    the previous tile), row 120 is a clip start; 61 rows = one clip plus one row.  The new path's error against float64 may be at most twice
    the two-launch path's, measured here (the K chain is reordered, not lengthened)."""
    _x, w0, w1, _b, _r = operands(M)
    for bias, relu, res2 in FLAGS:
        ref = reference(M, d, bias, relu, res2)
        new = one_launch(M, d, w0, w1, bias, relu, res2, tile, monkeypatch).numpy()
        old = two_launches(M, d, bias, relu, res2).numpy()
        e_new, e_old = rel_l2(new, ref), rel_l2(old, ref)
        print(f"M={M} d={d} tile={tile} bias={bias} relu={relu} res2={res2}: rel-L2 vs float64 one launch {e_new:.3e}, two launches {e_old:.3e}; "
              f"max|d| {np.abs(new - ref).max():.3e} / {np.abs(old - ref).max():.3e}")
        assert np.isfinite(new).all()
        assert e_new <= 2 * e_old


@pytest.mark.parametrize("tile", ["64", "128"])
@pytest.mark.parametrize("M,d", [(180, 1), (180, 2), (180, 4), (61, 2)])
def test_causal_product_zero_rows(M, d, tile, monkeypatch):
    """With tap 1 zero and no epilogue only the shifted segment contributes: rows (r mod 60) < d must be exactly zero, every other row not."""
    _x, w0, w1, _b, _r = operands(M)
    y = one_launch(M, d, w0, torch.zeros_like(w1), False, False, False, tile, monkeypatch).numpy()
    head = (np.arange(M) % PERIOD) < d
    assert (y[head] == 0).all()
    assert (np.abs(y[~head]).max(axis=1) > 0).all()
    assert rel_l2(y, reference(M, d, False, False, False) - operands(M)[0].double().numpy() @ w1.double().numpy().T) < 3e-5


def test_add_rows_split_images_and_products():
    """eg_add_rows_split: fp32 sum as eg_add_rows, images bit-equal to eg_split_tiles of that sum (rows = 68: a partial second tile; D = 512);
    the two products that now read such images (fusion_proj.0: bias + ReLU; Q|K|V: N = 1536) within the product tolerance of their fp32-input runs."""
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd import ops
    from emotiongestures_amd.engine import _ptr, _stream
    lib = L.load()
    rows, D, F = 68, 512, 34
    a, tab, b2 = T("aa", (rows, D)), T("at", (F, D)), T("ab", (rows, D))
    for table, period in ((tab, F), (b2, 0)):
        ad, td = a.to(dev()), table.to(dev())
        out = torch.empty(rows, D, device=dev())
        img = torch.zeros(2 * 128 * D, dtype=torch.int16, device=dev())
        L.check(lib.eg_add_rows_split(_ptr(ad), _ptr(td), _ptr(out), _ptr(img), rows, D, period, _stream(dev())), "eg_add_rows_split")
        assert torch.equal(out, ops.add_rows(ad, td, period=period))
        assert torch.equal(img, split_images(out, rows, D))
    for N, relu in ((512, 1), (1536, 0)):
        w, bias = T(f"aw{N}", (N, D), -0.1, 0.1), T(f"abias{N}", (N,))
        wp, npad, kpad = ops.pack_linear_weight(w, dev())
        bp = torch.zeros(npad, device=dev())
        bp[:N] = bias.to(dev())
        y_img, y_f32 = torch.empty(rows, N, device=dev()), torch.empty(rows, N, device=dev())
        L.check(lib.eg_linear_presplit(_ptr(img), D, _ptr(wp), kpad, _ptr(bp), None, None, N, _ptr(y_img), N, rows, N, D, relu,
                                       L.precision_code("bf16x3"), _stream(dev())), "eg_linear_presplit")
        L.check(lib.eg_linear(_ptr(out), D, _ptr(wp), kpad, _ptr(bp), None, None, N, _ptr(y_f32), N, rows, N, D, relu, 0, 0,
                              L.precision_code("bf16x3"), _stream(dev())), "eg_linear")
        e = rel_l2(y_img.cpu().numpy(), y_f32.cpu().numpy())
        print(f"N={N}: images vs fp32 input rel-L2 {e:.3e}")
        assert e < 3e-5             # tests/test_gpu_kernels.py TOL["bf16x3"]
