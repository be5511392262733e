"""Test-side float64 references and DERIVED error bounds for the inference 3x3 convolutions (csrc/conv.hip: eg_conv3x3, eg_conv3x3_se and the
forms that replace a route's kernel) and their pooling partials.  A helper module (not collected: no test_ prefix); tests/test_conv_f64.py shows
on the CPU that it rejects errors the whole-tensor relative L2 of tests/test_gpu_kernels.py accepts, tests/test_gpu_conv3x3_f64.py applies it.

References, all from torch.nn.functional.conv2d in float64, NCHW:
  stated(prec)  the sum the kernel states, in float64.  f32: the operands as given.  bf16: xh * wh.  bf16x3: wl*xh + wh*xl + wh*xh, with
                hi = bf16_rne(v), lo = bf16_rne(v - hi) on both operands (packing._bf16_split_bits, csrc/common.h).  bf16 x bf16 products are exact in
                fp32, so a correct kernel differs from `stated` by fp32 accumulation and the fp32 epilogue only.
  true          the unsplit float64 convolution.
  epilogue      v = acc + bias; relu; v * scale + shift; then relu(v * gate + res) (SE form) or v + res (residual-only form).
  A             the same expression on absolute values: conv(|x|, |w|) + |bias|, carried through |scale|, |shift|, |gate|, |res|.

Bounds (derived, not measured), U = 2^-24:
  against stated   |got - ref| <= 2 * N * U * A + 4 * U * |ref|,  N = 9 * cin terms (f32, bf16) or 27 * cin (bf16x3): first-order fp32 summation
                   in any order, times 2 for the matrix pipe's internal grouping, plus the epilogue's few roundings
  against true     bf16x3 only: + 3 * 2^-16 * A (the dropped xl*wl and the two second roundings, each at most 2^-16 |x w|)
  bf16 is compared with `stated` only: against `true` its rounding noise (~2^-8) hides indexing errors.
On top of the element bound runs tower_f64's slice walk (per channel x {first row, last row, first column, last column, each 32-column tile}); a
slice's limit is the rms of the element bound over the slice.  Each pooling partial is held against the float64 sum of its own rows x 32 tile
(numbered ty * tiles_x + tx, as eg_conv3x3_gap_tiles counts them) within the sum of its pixels' element bounds.

Worst error / bound measured on the MI355X (tests/test_gpu_conv3x3_f64.py prints them per case; a kernel believed right must stay below 0.25):
  conv, partials included, against stated   f32 0.0074    bf16x3 0.0015    bf16 0.0028      (the fp32 kernels sum sequentially, the matrix pipe in trees)
  conv against true                         bf16x3 0.012 (the split term alone reaches 0.037 of its allowance on these shapes, tests/test_conv_f64.py)
  worst single case                         32 -> 32 and 32 => 64, 0.0122 (bf16x3 against true); 256 -> 256 stays below 0.001
  stage-entry conv2 with the 1x1 shortcut   bf16x3 0.00093 (stated), 0.0048 (true)    bf16 0.0015
  eg_stem_conv 0.143, eg_se_residual_relu 0.249 (identity tail: its bound is 4 roundings of two operations, so the ratio is large by construction)
"""
import functools

import torch
import torch.nn.functional as F

import tower_f64

U = 2.0 ** -24
SPLIT_TERM = 3 * 2.0 ** -16
TOL = {"f32": 2e-6, "bf16x3": 3e-5, "bf16": 2e-2}         # tests/test_gpu_kernels.py: the whole-tensor tolerances this helper is measured against
GUARD = 4096                                                # floats of sentinel behind every output buffer
SENTINEL = -12345.5


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def split_bf16(v):
    """fp32 tensor -> (hi, lo) as float64: hi = bf16_rne(v), lo = bf16_rne(v - hi) (v - hi is exact in fp32)."""
    v = v.float()
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def conv64(x, w, stride=1):
    return F.conv2d(x.double(), w.double(), None, stride=stride, padding=1)


def terms(prec, cin):
    return (27 if prec == "bf16x3" else 9) * cin


class Raw:
    """The float64 convolutions of one (x, w, stride) without epilogue: true, stated per precision, the absolute-value sum."""

    def __init__(self, x, w, stride=1):
        self.cin, self.stride = x.shape[1], stride
        xh, xl = split_bf16(x)
        wh, wl = split_bf16(w)
        self.true = conv64(x, w, stride)
        hh = conv64(xh, wh, stride)
        self.terms3 = dict(hh=hh, lh=conv64(xl, wh, stride), hl=conv64(xh, wl, stride))        # lh: xl * wh, hl: xh * wl
        self.ll = None
        self._xl_wl = (xl, wl)
        self.stated = {"f32": self.true, "bf16": hh, "bf16x3": self.terms3["hl"] + self.terms3["lh"] + hh}
        self.abs = conv64(x.abs(), w.abs(), stride)

    def dropped(self):
        """xl * wl, the term bf16x3 leaves out."""
        if self.ll is None:
            self.ll = conv64(*self._xl_wl, self.stride)
        return self.ll


def _cv(v):
    return None if v is None else v.double().view(1, -1, 1, 1)


def epilogue(acc, bias=None, relu=False, scale=None, shift=None, gate=None, res=None):
    """acc [B, C, H, W] float64; bias / scale / shift [C]; gate [B, C]; res like acc.  gate + res: relu(v * gate + res); res alone: v + res."""
    v = acc if bias is None else acc + _cv(bias)
    if relu:
        v = F.relu(v)
    if scale is not None:
        v = v * _cv(scale)
    if shift is not None:
        v = v + _cv(shift)
    if gate is not None:
        v = F.relu(v * gate.double()[:, :, None, None] + res.double())
    elif res is not None:
        v = v + res.double()
    return v


def epilogue_abs(acc_abs, bias=None, scale=None, shift=None, gate=None, res=None):
    """A: the epilogue on absolute values (a ReLU does not enlarge an error)."""
    ab = lambda t: None if t is None else t.abs()           # noqa: E731
    v = epilogue(acc_abs, ab(bias), False, ab(scale), ab(shift), None, None)
    if gate is not None:
        v = v * gate.double().abs()[:, :, None, None]
    if res is not None:
        v = v + res.double().abs()
    return v


def elem_bound(prec, cin, A, ref, against="stated"):
    b = 2 * terms(prec, cin) * U * A + 4 * U * ref.abs()
    if against == "true":
        assert prec == "bf16x3", "only bf16x3 is held against the unsplit convolution"
        b = b + SPLIT_TERM * A
    return b


# ---- checks --------------------------------------------------------------------------------------------------------------------------
def map_errors(got, ref, bound):
    """-> (worst |got - ref| / bound, its index, worst slice ||d_s|| / ||bound_s||, the slice) for NCHW float64 maps."""
    d = (got.double() - ref).abs()
    ratio = d / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    worst_s, where = 0.0, ""
    for fam, idx, dn, bn, _n in tower_f64._slice_errors(d, bound):
        if dn > worst_s * bn:
            worst_s, where = dn / max(bn, 1e-300), f"{fam}, {idx}"
    return float(ratio.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape)), worst_s, where


def check_map(got, ref, bound, what):
    """Every element finite and within its bound, every slice within the rms of its bounds.  -> worst error / bound."""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements (an element never written?)"
    r, idx, rs, where = map_errors(got, ref, bound)
    assert r <= 1.0, (f"{what}: element (b, c, y, x) = {idx} is {float(got[idx]):.9g}, float64 {float(ref[idx]):.9g}: "
                      f"|d| = {abs(float(got[idx]) - float(ref[idx])):.3e} = {r:.3g} x its bound {float(bound[idx]):.3e}")
    assert rs <= 1.0, f"{what}: slice rms error {rs:.3g} x the rms of its bounds at {where}"
    return r


def tile_sums(t, rows):
    """Sums of t [B, C, H, W] over its rows x 32 tiles, numbered ty * tiles_x + tx: [B, tiles, C]."""
    B, C, H, W = t.shape
    p = F.pad(t, (0, -W % 32, 0, -H % rows))
    s = p.view(B, C, p.shape[2] // rows, rows, p.shape[3] // 32, 32).sum((3, 5))
    return s.reshape(B, C, -1).permute(0, 2, 1)


def check_partials(got, ref_map, bound_map, rows, what):
    """got [B, tiles, C]: each partial against the float64 sum of its own tile, within the sum of the tile's element bounds.  -> worst ratio."""
    ref, lim = tile_sums(ref_map, rows), tile_sums(bound_map, rows)
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: partials {tuple(got.shape)} vs {tuple(ref.shape)} tiles of {rows} x 32"
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} partials not written"
    ratio = (got.double() - ref).abs() / lim.clamp_min(1e-300)
    i = int(ratio.argmax())
    b, t, c = (int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    r = float(ratio[b, t, c])
    assert r <= 1.0, f"{what}: partial (clip {b}, tile {t}, channel {c}) is {float(got[b, t, c]):.9g}, its tile sums to {float(ref[b, t, c]):.9g}: {r:.3g} x the bound"
    return r


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


# ---- guarded output buffers ----------------------------------------------------------------------------------------------------------
def guarded(shape, device):
    """A NaN-filled output of `shape` with GUARD sentinel floats behind it: -> (the output view, the whole buffer)."""
    n = 1
    for s in shape:
        n *= int(s)
    n_al = (n + 3) // 4 * 4
    buf = torch.full((n_al + GUARD,), SENTINEL, dtype=torch.float32, device=device)
    buf[:n] = float("nan")
    return buf[:n].view(*shape), buf


def guard_intact(buf, shape):
    n = 1
    for s in shape:
        n *= int(s)
    tail = buf[n:]
    return bool((tail == SENTINEL).all())


# ---- the cases of tests/test_gpu_conv3x3_f64.py (shared with the CPU self-test) -------------------------------------------------------
# route name (csrc/conv.hip ROUTES) -> (cin, stride, tile rows, output-channel counts: cout_lo, one multiple of 4 but not of 16, one that is no
# multiple of 4 where the range has one, cout_hi)
ROUTE_CASES = {
    "R_32": (32, 1, 4, (32,)),
    "R_32_NARROW": (32, 1, 8, (17, 20, 31)),
    "R_32_64": (32, 2, 2, (49, 52, 64)),
    "R_64": (64, 1, 8, (49, 52, 64)),
    "R_64_128": (64, 2, 2, (113, 116, 128)),
    "R_64_128_S1": (64, 1, 4, (128,)),
    "R_128_48": (128, 1, 4, (1, 20, 34, 48)),
    "R_128_64": (128, 1, 4, (49, 60, 64)),
    "R_128": (128, 1, 4, (65, 68, 100, 128)),
    "R_128_256": (128, 2, 2, (241, 244, 256)),
    "R_256": (256, 1, 2, (256,)),
}


def route_maps(rows, stride):
    """-> [(batch, H, W, Ho, Wo)]: output maps 3 x 5 (smaller than a tile), rows x 32 (one tile), (rows + 1) x 33 (one row and one column into the next
    tiles), (2 rows + 1) x 65; batches 3, 1, 3, 1.  At stride 2 the input heights alternate odd / even (2 Ho - 1, 2 Ho), the widths even / odd."""
    out = []
    for i, (ho, wo) in enumerate(((3, 5), (rows, 32), (rows + 1, 33), (2 * rows + 1, 65))):
        h, w = (ho, wo) if stride == 1 else (2 * ho - (i + 1) % 2, 2 * wo - i % 2)
        out.append(((3, 1, 3, 1)[i], h, w, ho, wo))
    return out


@functools.lru_cache(maxsize=None)
def case(cin, cout, stride, B, H, W):
    """(x NCHW, w, bias, scale, shift, Raw) on synth.hash_uniform data: built once per shape, shared, never modified."""
    from emotiongestures_amd.synth import hash_uniform

    def T(key, shape, lo, hi):
        return torch.from_numpy(hash_uniform(key, shape, lo, hi, 0))

    x = T(f"x{cin}", (B, cin, H, W), -1, 1)
    w = T(f"w{cin}{cout}", (cout, cin, 3, 3), -0.1, 0.1)
    bias, scale, shift = T("b", (cout,), -0.2, 0.2), T("s", (cout,), 0.5, 1.5), T("t", (cout,), -0.3, 0.3)
    return x, w, bias, scale, shift, Raw(x, w, stride)
