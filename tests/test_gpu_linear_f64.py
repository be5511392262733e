"""The linear family of csrc/gemm.hip on the GPU -- eg_linear, eg_linear_splitk, eg_split_tiles, eg_linear_presplit -- called through the C ABI at the
shapes where such kernels go wrong, every output ELEMENT against the float64 restatement of tests/products_f64.py within its a-priori bound
(reference, bound, case lists and their reasons are there; tests/test_products_f64.py shows on the CPU that the bounds reject a split term lost in
one 16-column tile, a dropped k, a bias one column off, a misplaced res2 and a row shift across a sequence boundary).

Every output is rows 1 .. M of a [M + 2, ldc] buffer filled with one NaN bit pattern; after the call every slot outside [0:M, 0:N] -- the rows in
front and behind, the columns N .. ldc - 1 -- must still hold that pattern bit for bit.  The gaps of strided inputs (lda > K, ldr > N) hold NaN: a
kernel that reads one into a result fails the finiteness check.  Each test prints the worst element it saw as a fraction of the bound."""
import numpy as np
import pytest
import torch

import products_f64 as P

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5           # a quiet NaN no arithmetic produces
_PACKED = {}                    # (N, K) -> (image, Npad, Kpad): one weight pack per shape for the whole module


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, _stream(dev())


def packed(n, k):
    from emotiongestures_amd import ops
    if (n, k) not in _PACKED:
        _PACKED[(n, k)] = ops.pack_linear_weight(P.linear_weight(n, k), dev())
    return _PACKED[(n, k)]


def strided(t, ld):
    """t [rows, cols] (or None) -> (device buffer [rows, ld] with NaN in the gap columns, ld)."""
    if t is None:
        return None
    buf = torch.full((t.shape[0], ld), float("nan"), device=dev())
    buf[:, :t.shape[1]] = t.to(dev())
    return buf


def canary(rows, ld):
    """-> (int32 buffer [rows + 2, ld] of SENTINEL, its row 1 as the float32 output base)."""
    buf = torch.full((rows + 2, ld), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[1:]


def canary_result(buf, m, n, what):
    """The [M, N] result out of a canary buffer, after checking that nothing else was written."""
    torch.cuda.synchronize()
    b = buf.cpu()
    out = b[1:m + 1, :n].clone()
    b[1:m + 1, :n] = SENTINEL
    bad = (b != SENTINEL).nonzero()
    assert bad.numel() == 0, f"{what}: stores outside [0:{m}, 0:{n}], first at buffer row {int(bad[0, 0]) - 1}, column {int(bad[0, 1])}"
    return out.view(torch.float32)


def run_linear(case, prec, layout, shift=0, seq=0, entry="eg_linear", ximg=None):
    """One eg_linear (or eg_linear_presplit on `ximg`) call -> the [M, N] result (CPU), canaries checked."""
    L, lib, _ptr, st = _api()
    x, w, bias, r1, r2, relu = case
    (m, k), n = x.shape, w.shape[0]
    name, lda, ldr, ldc = layout
    wp, _, kpad = packed(n, k)
    bd = None if bias is None else bias.to(dev())
    r1d, r2d = strided(r1, ldr), strided(r2, ldr)
    buf, y = canary(m, ldc)
    what = f"{entry} {m}x{n}x{k} {prec} {name}"
    if entry == "eg_linear":
        xd = strided(x, lda)
        rc = lib.eg_linear(_ptr(xd), lda, _ptr(wp), kpad, _ptr(bd), _ptr(r1d), _ptr(r2d), ldr, _ptr(y), ldc, m, n, k, int(relu), shift, seq,
                           L.precision_code(prec), st)
    else:
        rc = lib.eg_linear_presplit(_ptr(ximg), k, _ptr(wp), kpad, _ptr(bd), _ptr(r1d), _ptr(r2d), ldr, _ptr(y), ldc, m, n, k, int(relu),
                                    L.precision_code(prec), st)
    L.check(rc, what)
    return canary_result(buf, m, n, what), what


def check_linear(case, prec, layout, shift=0, seq=0, tag="eg_linear"):
    got, what = run_linear(case, prec, layout, shift, seq)
    x, w, bias, r1, r2, relu = case
    ref = P.linear_f64(x, w, bias, r1, r2, relu, shift, max(seq, 1))
    el = P.compare_sliced(got, ref, P.linear_bound(x, w, bias, r1, r2, relu, shift, max(seq, 1), prec), what, P.LIN_AXES)[2]
    return el, got


def report(entry, prec, worst):
    print(f"FRACTION {entry} {prec} {worst:.3f}")


# ---- eg_linear ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", P.PRECISIONS)
@pytest.mark.parametrize("idx", range(len(P.LINEAR_SHAPES)), ids=lambda i: "x".join(map(str, P.LINEAR_SHAPES[i])))
def test_linear_matches_float64_per_element(idx, prec):
    """eg_linear by its default dispatch (launch_gemm / skinny_ok): f32 -> gemm_kernel<F32>; bf16 -> gemm_glds_kernel<1, 2>; bf16x3 -> M <= 64:
    gemm_skinny_kernel<RT = ceil(M / 16), XF32>, M > 64: gemm_glds_kernel<3, 2>.  Dense, with every stride padded (ldc odd: scalar stores of full
    quads) and, where N % 4 == 0, with ldc = N + 4 (16-byte stores next to a gap); the epilogue option rotates with the shape."""
    m, n, k = P.LINEAR_SHAPES[idx]
    case = P.linear_inputs("lin", m, n, k, idx)
    worst = max(check_linear(case, prec, layout)[0] for layout in P.layouts(n, k))
    report("eg_linear", prec, worst)


ROUTES = [("bf16x3", "EG_GEMM_SKINNY", "0"), ("bf16x3", "EG_GEMM_SKINNY", "1"), ("bf16x3", "EG_GLDS_TILE", "0"), ("bf16x3", "EG_GLDS_TILE", "1"),
          ("bf16", "EG_GLDS_TILE", "0"), ("bf16", "EG_GLDS_TILE", "1")]


@pytest.mark.parametrize("prec,var,value", ROUTES)
def test_linear_kernel_routes(prec, var, value, monkeypatch):
    """The per-call switches of csrc/gemm.hip force a route at every shape of its range:
      EG_GEMM_SKINNY=0, M <= 64, bf16x3: skinny_ok's row limit becomes 0 -> launch_gemm -> gemm_glds_kernel<3, 2> (64 x 64 tile, X split per workgroup);
      EG_GEMM_SKINNY=1, M <= 64, bf16x3: the default, gemm_skinny_kernel<RT, XF32> (16 columns per workgroup, K steps dealt over the waves);
      EG_GLDS_TILE=0 / 1, M > 64, bf16 and bf16x3: gemm_glds_kernel<TERMS, WN = 2> (64 x 64) / <TERMS, WN = 4> (64 x 128; its second weight tile is
      clamped to the last one where N <= 64).  Strided layout only (the dense one ran above); the tiles of EG_GLDS_TILE are bitwise equal."""
    worst = 0.0
    for idx, (m, n, k) in enumerate(P.LINEAR_SHAPES):
        if (var == "EG_GEMM_SKINNY") != (m <= 64):
            continue
        case = P.linear_inputs("lin", m, n, k, idx)
        monkeypatch.setenv(var, value)
        el, got = check_linear(case, prec, P.layouts(n, k)[1])
        monkeypatch.delenv(var)
        worst = max(worst, el)
        if var == "EG_GLDS_TILE":
            assert torch.equal(got, run_linear(case, prec, P.layouts(n, k)[1])[0]), f"{m}x{n}x{k}: EG_GLDS_TILE={value} differs from the default tile"
    report(f"eg_linear[{var}={value}]", prec, worst)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("idx", range(len(P.CAUSAL_CASES)), ids=lambda i: "-".join(map(str, P.CAUSAL_CASES[i])))
def test_linear_causal_shift(idx, prec, monkeypatch):
    """a_shift / a_seq: f32 -> gemm_kernel<F32> (load_x_quad); bf16x3 -> M <= 64 with EG_GEMM_SKINNY=1: gemm_skinny_kernel<RT, XF32> (load_x_quad), else
    gemm_bf16_kernel<3> (launch_gemm's a_shift branch: register-staged X rows, zero where (m % a_seq) < a_shift)."""
    m, seq, sh, n, k = P.CAUSAL_CASES[idx]
    case = P.linear_inputs("cau", m, n, k, idx)
    worst = 0.0
    for skinny in ("0", "1"):
        monkeypatch.setenv("EG_GEMM_SKINNY", skinny)
        for layout in P.layouts(n, k)[:2]:
            worst = max(worst, check_linear(case, prec, layout, sh, seq)[0])
        monkeypatch.delenv("EG_GEMM_SKINNY")
        if prec == "f32" or m > 64:
            break                   # the switch changes nothing there
    if sh >= seq:                   # every row zero-sourced: the output is the epilogue of 0, exactly
        x, w, bias, r1, r2, relu = case
        got = run_linear(case, prec, P.layouts(n, k)[0], sh, seq)[0]
        assert torch.equal(got, P.epilogue(torch.zeros(m, n), bias, r1, r2, relu))
    report("eg_linear[a_shift]", prec, worst)


# ---- eg_linear_splitk -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("m,n,k,splits", P.SPLITK_CASES)
def test_linear_splitk(m, n, k, splits, prec):
    """launch_splitk: gemm_kernel<F32> / gemm_glds_kernel<3, 2> over nsplit 64-rounded K slices (blockIdx.z) writing raw partials, then
    splitk_reduce_kernel with the epilogue.  With and without bias, with ReLU; the partial buffer's tail behind nsplit * M * N stays untouched."""
    L, lib, _ptr, st = _api()
    x, w, bias, _, _, _ = P.linear_inputs("spk", m, n, k, 1)
    wp, _, kpad = packed(n, k)
    nsplit = P.splitk_slices(k, splits)[1]
    worst = 0.0
    for (b, relu, (name, lda, _, ldc)) in ((bias, True, P.layouts(n, k)[0]), (None, True, P.layouts(n, k)[1]), (bias, False, P.layouts(n, k)[1])):
        what = f"eg_linear_splitk {m}x{n}x{k}/{splits} {prec} {name} bias {b is not None} relu {relu}"
        xd, bd = strided(x, lda), None if b is None else b.to(dev())
        part = torch.full((nsplit * m * n + 256,), SENTINEL, dtype=torch.int32, device=dev())
        buf, y = canary(m, ldc)
        L.check(lib.eg_linear_splitk(_ptr(xd), lda, _ptr(wp), kpad, _ptr(bd), _ptr(y), ldc, m, n, k, int(relu), splits, _ptr(part),
                                     L.precision_code(prec), st), what)
        got = canary_result(buf, m, n, what)
        assert bool((part[nsplit * m * n:] == SENTINEL).all()), f"{what}: a partial sum behind slice {nsplit - 1}"
        assert bool(torch.isfinite(part[:nsplit * m * n].view(torch.float32)).all()), f"{what}: a partial slot was not written"
        ref = P.linear_f64(x, w, b, None, None, relu)
        worst = max(worst, P.compare_sliced(got, ref, P.linear_bound(x, w, b, None, None, relu, 0, 1, prec), what, P.LIN_AXES)[2])
    report("eg_linear_splitk", prec, worst)


# ---- eg_split_tiles ---------------------------------------------------------------------------------------------------------------------------
def split_tiles(x, lda):
    """eg_split_tiles of x [M, K] (CPU) read with row stride lda -> (device image buffer with a sentinel tail, its int16 slot count)."""
    L, lib, _ptr, st = _api()
    m, k = x.shape
    slots = 2 * ((m + 63) // 64) * 64 * ((k + 63) // 64 * 64)
    img = torch.full((slots + 256,), 0x5A5A, dtype=torch.int16, device=dev())
    xd = strided(x, lda)
    L.check(lib.eg_split_tiles(_ptr(xd), lda, m, k, _ptr(img), st), f"eg_split_tiles {m}x{k} lda {lda}")
    torch.cuda.synchronize()
    return img, slots


@pytest.mark.parametrize("m,k", P.SPLIT_TILES_CASES)
def test_split_tiles_is_bitwise_the_slot_map(m, k):
    """split_tile_kernel: bitwise images_of (the bf16 (hi, lo) split in the [ceil(M/64)][Kpad/8][64][8] slot map), rows >= M and columns >= K inside
    the images bitwise zero (the contract csrc/gemm.hip states), nothing written behind the images; dense and with lda = K + 4."""
    x = P.T(f"st{m}x{k}", (m, k))
    want = P.images_of(P.padded_k(x))
    for lda in (k, k + 4):
        img, slots = split_tiles(x, lda)
        got = img[:slots].cpu().view(want.shape)
        assert torch.equal(got, want), f"eg_split_tiles {m}x{k} lda {lda}: {int((got != want).sum())} slots differ"
        rows = P.image_rows(got, got.shape[1] * 64)
        assert int(rows[:, m:].abs().sum()) == 0 and int(rows[:, :, k:].abs().sum()) == 0
        assert bool((img[slots:] == 0x5A5A).all()), f"eg_split_tiles {m}x{k} lda {lda}: a store behind the images"


# ---- eg_linear_presplit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ["64", "128"])
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("idx", range(len(P.PRESPLIT_CASES)), ids=lambda i: "x".join(map(str, P.PRESPLIT_CASES[i])))
def test_linear_presplit(idx, prec, tile, monkeypatch):
    """eg_split_tiles + eg_linear_presplit with EG_GEMM_TILE = "64" (gemm_presplit_kernel<TERMS>: 4-slot ring of 32-deep steps, unrolled ring turns
    from 7 steps on) and "128" (gemm_presplit128_kernel<TERMS>: 3-slot ring, odd tile counts re-read the last tile): K from one step to 14.  Dense and
    strided ldr / ldc; bitwise eg_linear's in-kernel-split result on the same operands (skinny route off: gemm_glds_kernel, the same K order)."""
    m, n, k = P.PRESPLIT_CASES[idx]
    case = P.linear_inputs("pre", m, n, k, idx)
    x, w, bias, r1, r2, relu = case
    img, _ = split_tiles(x, k)
    worst = 0.0
    for layout in P.layouts(n, k)[:2]:
        monkeypatch.setenv("EG_GEMM_TILE", tile)
        got, what = run_linear(case, prec, layout, entry="eg_linear_presplit", ximg=img)
        monkeypatch.delenv("EG_GEMM_TILE")
        ref = P.linear_f64(x, w, bias, r1, r2, relu)
        worst = max(worst, P.compare_sliced(got, ref, P.linear_bound(x, w, bias, r1, r2, relu, 0, 1, prec), what + " tile " + tile, P.LIN_AXES)[2])
        monkeypatch.setenv("EG_GEMM_SKINNY", "0")
        same = run_linear(case, prec, layout)[0]
        monkeypatch.delenv("EG_GEMM_SKINNY")
        assert torch.equal(got, same), f"{what} tile {tile}: differs from eg_linear on the same operands"
    report(f"eg_linear_presplit[{tile}]", prec, worst)
