"""The inference 3x3 convolutions and the SE tail (csrc/conv.hip), every output element against float64 within the derived bounds of
tests/conv_f64.py: every entry of the route table at the edges of its output-channel range, every form that replaces a route's kernel under its own
name, eg_conv3x3_se's three forms, the SE tail operators one by one, and the refusals.

The C ABI is called directly on NaN-filled outputs with 4096 sentinel floats behind each: an element never written, a padded channel tile stored
past cout and a last partial tile stored past the map all show.  Each test prints its worst error / bound; the summary is in conv_f64's docstring.
`test_every_route_form_and_padded_count_was_launched` is the last test of the module and reads what the tests above recorded in this process.

The gate operators' bound is 4 x the error of the same formula evaluated in fp32 by torch on the CPU against float64 (both sides sum the same number
of fp32 terms in a different order), with a floor of 2^-20 (a fast exponential and a reciprocal on a value of at most 1).  Measured on the MI355X
(worst |gate - float64| over the cases, and the bound it was held to):
  C = 32, 64    6.8e-08 (bound 9.5e-07: the floor)        C = 128    2.9e-07 (9.5e-07)        C = 256    7.1e-07 (1.9e-06; torch fp32 4.7e-07)
  The worst error / bound is 0.47, eg_se_gate on conv2's own partials against the formula on t1 at C = 256, 3 x 5.
"""
import contextlib
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import conv_f64 as C
from emotiongestures_amd.synth import hash_uniform

pytestmark = pytest.mark.gpu

PRECS = ("f32", "bf16x3", "bf16")
UNSUPPORTED = -2                                           # include/emogest.h: EG_ERR_UNSUPPORTED
LAUNCHED = {}                                              # route name -> {(cout, form)}
WORST = {}                                                 # (kind, precision) -> worst error / bound


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def T(key, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(hash_uniform(key, shape, lo, hi, 0))


def note(kind, prec, r):
    WORST[(kind, prec)] = max(WORST.get((kind, prec), 0.0), r)


@contextlib.contextmanager
def env(**kv):
    """Set (or, for None, unset) the kernels' A/B switches for the block; they are read per call."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def operands(cin, cout, stride, B, H, W):
    """The case's device operands: x NHWC, the packed weight image and the three vectors at the route's padded width."""
    from emotiongestures_amd import ops
    x, w, bias, scale, shift, _raw = C.case(cin, cout, stride, B, H, W)
    return (nhwc(x).to(dev()),) + tuple(ops.conv3x3_pack(w, bias, scale, shift, dev(), stride))


def launch(xg, wp, bias, scale, shift, B, H, W, cin, cout, stride, relu, nchw, prec, gate=None, res=None, se=False, want_gap=True):
    """eg_conv3x3 / eg_conv3x3_se on guarded NaN-filled buffers -> (y NCHW float64 on the CPU, partials [B, tiles, cout] float64 or None)."""
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd._host import ptr, stream
    lib, d = L.load(), dev()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    tiles = int(lib.eg_conv3x3_gap_tiles(H, W, cin, cout, stride))
    yshape = (B, cout, Ho * Wo) if nchw else (B, Ho, Wo, cout)
    y, ybuf = C.guarded(yshape, d)
    gap, gbuf = C.guarded((B, tiles, cout), d) if want_gap else (None, None)
    code = L.precision_code(prec)
    if se:
        rc = lib.eg_conv3x3_se(ptr(xg), ptr(wp), ptr(bias), ptr(scale), ptr(shift), ptr(gate), ptr(res), ptr(y), ptr(gap), B, H, W, cin, cout, stride,
                               int(relu), int(nchw), code, stream(d))
    else:
        rc = lib.eg_conv3x3(ptr(xg), ptr(wp), ptr(bias), ptr(scale), ptr(shift), ptr(y), ptr(gap), B, H, W, cin, cout, stride, int(relu), int(nchw), code,
                            stream(d))
    L.check(rc, "eg_conv3x3")
    torch.cuda.synchronize()
    assert C.guard_intact(ybuf, yshape), f"{cin}->{cout} stride {stride} {H}x{W} {prec}: y was written past its end"
    if want_gap:
        assert C.guard_intact(gbuf, (B, tiles, cout)), f"{cin}->{cout} stride {stride} {H}x{W} {prec}: the partials were written past their end"
    yc = y.cpu()
    yc = yc.view(B, cout, Ho, Wo) if nchw else yc.permute(0, 3, 1, 2)
    return yc.double(), (gap.cpu().double() if want_gap else None)


def hold(got, gap, raw, prec, cin, rows, what, bias=None, relu=False, scale=None, shift=None, gate=None, res=None):
    """The map and its partials against float64: `stated` in every precision, bf16x3 against the unsplit convolution as well."""
    A = C.epilogue_abs(raw.abs, bias, scale, shift, gate, res)
    worst = 0.0
    for against in ("stated", "true") if prec == "bf16x3" else ("stated",):
        ref = C.epilogue(raw.stated[prec] if against == "stated" else raw.true, bias, relu, scale, shift, gate, res)
        bound = C.elem_bound(prec, cin, A, ref, against)
        r = C.check_map(got, ref, bound, f"{what} against {against}")
        if gap is not None:
            r = max(r, C.check_partials(gap, ref, bound, rows, f"{what} against {against}"))
        note(f"conv against {against}", prec, r)
        worst = max(worst, r)
    return worst


# ---- every route, at the edges of its output-channel range -------------------------------------------------------------------------------
ROUTE_PARAMS = [(name, cout) for name, (_ci, _s, _r, couts) in C.ROUTE_CASES.items() for cout in couts]


@pytest.mark.parametrize("name,cout", ROUTE_PARAMS, ids=[f"{n}-{c}" for n, c in ROUTE_PARAMS])
def test_route_against_float64(name, cout):
    from emotiongestures_amd import _lib as L
    lib = L.load()
    cin, stride, rows, _couts = C.ROUTE_CASES[name]
    assert int(lib.eg_conv3x3_cout_pad(cin, cout, stride)) >= cout
    layouts = (False, True) if cout % 4 == 0 else (True,)          # NHWC needs cout % 4 == 0
    worst = 0.0
    with env(EG_CONV_SPLIT=None, EG_CONV_S2=None):
        for (B, H, W, Ho, Wo) in C.route_maps(rows, stride):
            x, w, bias, scale, shift, raw = C.case(cin, cout, stride, B, H, W)
            xg, wp, bp, sp, tp = operands(cin, cout, stride, B, H, W)
            tiles = int(lib.eg_conv3x3_gap_tiles(H, W, cin, cout, stride))
            assert tiles == -(-Ho // rows) * -(-Wo // 32)
            for prec in PRECS:
                for nchw in layouts:
                    for epi in (False, True):           # without / with bias + ReLU + affine
                        what = f"{name} {cin}->{cout} stride {stride} B={B} {H}x{W} {prec} {'NCHW' if nchw else 'NHWC'} epilogue={int(epi)}"
                        args = (bp, sp, tp) if epi else (None, None, None)
                        y, gap = launch(xg, wp, *args, B, H, W, cin, cout, stride, epi, nchw, prec)
                        assert gap.shape[1] == tiles
                        ekw = dict(bias=bias, relu=True, scale=scale, shift=shift) if epi else {}
                        worst = max(worst, hold(y, gap, raw, prec, cin, rows, what, **ekw))
                        LAUNCHED.setdefault(name, set()).add((cout, "nchw" if nchw else "nhwc"))
    print(f"{name} {cin}->{cout} stride {stride}: worst error / bound {worst:.3g}")


# ---- forms that replace a route's kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["1", "2", "4", None])
@pytest.mark.parametrize("c", [64, 128])
def test_channel_split_forms_against_float64(c, split):
    name = {64: "R_64", 128: "R_128"}[c]
    rows = C.ROUTE_CASES[name][2]
    worst = 0.0
    with env(EG_CONV_SPLIT=split, EG_CONV_S2=None):
        for (B, H, W, _ho, _wo) in C.route_maps(rows, 1):
            x, w, bias, scale, shift, raw = C.case(c, c, 1, B, H, W)
            xg, wp, bp, sp, tp = operands(c, c, 1, B, H, W)
            y, gap = launch(xg, wp, bp, sp, tp, B, H, W, c, c, 1, True, False, "bf16x3")
            worst = max(worst, hold(y, gap, raw, "bf16x3", c, rows, f"{c}->{c} EG_CONV_SPLIT={split} B={B} {H}x{W}", bias=bias, relu=True, scale=scale, shift=shift))
    LAUNCHED.setdefault(name, set()).add((c, f"split={split}"))
    print(f"{c}->{c} EG_CONV_SPLIT={split}: worst error / bound {worst:.3g}")


@pytest.mark.parametrize("form", ["interleaved", "planes4", "planes8", None])
@pytest.mark.parametrize("name", ["R_32_64", "R_64_128"])
def test_stride2_forms_against_float64(name, form):
    cin, stride, rows, couts = C.ROUTE_CASES[name]
    cout = couts[-1]
    worst = 0.0
    with env(EG_CONV_SPLIT=None, EG_CONV_S2=form):
        for (B, H, W, _ho, _wo) in C.route_maps(rows, 2) + [(3, 19, 62, 10, 31)]:        # Ho = 10: no multiple of the 4- or 8-row plane tiles
            x, w, bias, scale, shift, raw = C.case(cin, cout, 2, B, H, W)
            xg, wp, bp, sp, tp = operands(cin, cout, 2, B, H, W)
            for prec in ("bf16x3", "bf16"):
                y, gap = launch(xg, wp, bp, sp, tp, B, H, W, cin, cout, 2, True, False, prec)
                worst = max(worst, hold(y, gap, raw, prec, cin, rows, f"{cin}->{cout} EG_CONV_S2={form} B={B} {H}x{W} {prec}", bias=bias, relu=True, scale=scale, shift=shift))
    LAUNCHED.setdefault(name, set()).add((cout, f"s2={form}"))
    print(f"{cin}->{cout} EG_CONV_S2={form}: worst error / bound {worst:.3g}")


@functools.lru_cache(maxsize=None)
def _persistent_case():
    """16 x 64 map, 8 tiles a clip, 65 clips: the largest float64 reference of the module (65 x 32 x 16 x 64), built once; 64 clips are its head."""
    return C.case(32, 32, 1, 65, 16, 64)


@pytest.mark.parametrize("B,H,W,total", [(1, 9, 65, 9), (64, 16, 64, 512), (65, 16, 64, 520)])
def test_persistent_32_to_32_walk_against_float64(B, H, W, total):
    """csrc/conv.hip conv3x3_c32_persistent_kernel (split-bf16, NHWC): 9 tiles run on a grid rounded up to 16 whose surplus workgroups exit; 512 tiles
    fill the grid cap; at 520 a workgroup walks a second tile."""
    from emotiongestures_amd import _lib as L
    assert int(L.load().eg_conv3x3_gap_tiles(H, W, 32, 32, 1)) * B == total
    if (H, W) == (16, 64):
        x, w, bias, scale, shift, raw65 = _persistent_case()
        x = x[:B]
    else:
        x, w, bias, scale, shift, raw65 = C.case(32, 32, 1, B, H, W)
    from emotiongestures_amd import ops
    xg = nhwc(x).to(dev())
    wp, bp, sp, tp = ops.conv3x3_pack(w, bias, scale, shift, dev(), 1)
    worst = 0.0
    for prec in ("bf16x3", "bf16"):
        raw = type("Head", (), dict(stated={p: v[:B] for p, v in raw65.stated.items()}, true=raw65.true[:B], abs=raw65.abs[:B]))
        y, gap = launch(xg, wp, bp, sp, tp, B, H, W, 32, 32, 1, True, False, prec)
        worst = max(worst, hold(y, gap, raw, prec, 32, 4, f"32->32 persistent, {total} tiles, {prec}", bias=bias, relu=True, scale=scale, shift=shift))
    LAUNCHED.setdefault("R_32", set()).add((32, f"persistent tiles={total}"))
    print(f"32->32 persistent, {total} tiles: worst error / bound {worst:.3g}")


# ---- eg_conv3x3_se -------------------------------------------------------------------------------------------------------------------------
SE_PARAMS = [(name, cout) for name, (_ci, s, _r, couts) in C.ROUTE_CASES.items() if s == 1 for cout in couts if cout % 4 == 0]


@pytest.mark.parametrize("name,cout", SE_PARAMS, ids=[f"{n}-{c}" for n, c in SE_PARAMS])
def test_conv3x3_se_forms_against_float64(name, cout):
    cin, _s, rows, _couts = C.ROUTE_CASES[name]
    B, H, W, Ho, Wo = C.route_maps(rows, 1)[2]                  # (rows + 1) x 33, batch 3
    x, w, bias, scale, shift, raw = C.case(cin, cout, 1, B, H, W)
    xg, wp, bp, sp, tp = operands(cin, cout, 1, B, H, W)
    gate, res = T("gate", (B, cout), 0.0, 1.0).clamp_min(1e-3), T("res", (B, cout, H, W), -1, 1)
    gg, rg = gate.to(dev()), nhwc(res).to(dev())
    worst = 0.0
    with env(EG_CONV_SPLIT=None, EG_CONV_S2=None):
        for prec in PRECS:
            what = f"{name} {cin}->{cout} {prec} eg_conv3x3_se"
            y, gap = launch(xg, wp, None, sp, tp, B, H, W, cin, cout, 1, False, False, prec, gate=gg, res=rg, se=True)
            # the partials of the SE form are not a documented output of the fused tail: the map alone is held
            worst = max(worst, hold(y, None, raw, prec, cin, rows, what + " gate + residual", scale=scale, shift=shift, gate=gate, res=res))
            y, gap = launch(xg, wp, bp, sp, tp, B, H, W, cin, cout, 1, True, False, prec, res=rg, se=True)
            worst = max(worst, hold(y, None, raw, prec, cin, rows, what + " residual alone", bias=bias, relu=True, scale=scale, shift=shift, res=res))
            y0, gap0 = launch(xg, wp, bp, sp, tp, B, H, W, cin, cout, 1, True, False, prec, se=True)
            y1, gap1 = launch(xg, wp, bp, sp, tp, B, H, W, cin, cout, 1, True, False, prec)
            assert torch.equal(y0, y1) and torch.equal(gap0, gap1), what + ": gate == residual == NULL is not eg_conv3x3 bit for bit"
    LAUNCHED.setdefault(name, set()).add((cout, "se"))
    print(f"{name} {cin}->{cout} eg_conv3x3_se: worst error / bound {worst:.3g}")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _served(cin, stride, cout):
    """include/emogest.h, eg_conv3x3: the served (Cin, stride, Cout)."""
    table = {(32, 1): (17, 32), (32, 2): (49, 64), (64, 1): (49, 64), (64, 2): (113, 128), (128, 1): (1, 128), (128, 2): (241, 256), (256, 1): (256, 256)}
    lo, hi = table.get((cin, stride), (1, 0))
    return lo <= cout <= hi or (cin, stride, cout) == (64, 1, 128)


def test_unserved_shapes_are_refused_before_a_launch():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd._host import ptr, stream
    lib, d = L.load(), dev()
    x = torch.zeros(1, 4, 6, 256, device=d)
    w = torch.zeros(int(lib.eg_conv3x3_packed_floats(256, 272)), device=d)
    refused = 0
    for cin in (16, 32, 48, 64, 96, 128, 256):
        for stride in (1, 2):
            for cout in (1, 16, 17, 32, 33, 48, 49, 64, 65, 112, 113, 128, 129, 240, 241, 256, 257):
                assert (int(lib.eg_conv3x3_cout_pad(cin, cout, stride)) > 0) == _served(cin, stride, cout), (cin, stride, cout)
                if _served(cin, stride, cout):
                    continue
                y, ybuf = C.guarded((1, cout, 4 * 6), d)
                rc = lib.eg_conv3x3(ptr(x), ptr(w), None, None, None, ptr(y), None, 1, 4, 6, cin, cout, stride, 0, 1, 0, stream(d))
                torch.cuda.synchronize()
                assert rc == UNSUPPORTED, (cin, stride, cout, rc)
                assert bool(torch.isnan(y).all()) and C.guard_intact(ybuf, (1, cout, 24)), (cin, stride, cout)
                refused += 1
    assert refused > 150


# ---- the SE tail operators ------------------------------------------------------------------------------------------------------------------
GATE_FLOOR = 2.0 ** -20
TILE_ROWS = {32: 4, 64: 8, 128: 4, 256: 2}                  # the C -> C stride-1 routes


def _gate_formula(mean, w1, b1, w2, b2):
    return torch.sigmoid(F.linear(F.relu(F.linear(mean, w1, b1)), w2, b2))


def _se_weights(c):
    return T("se.w1", (c // 8, c), -0.3, 0.3), T("se.b1", (c // 8,), -0.1, 0.1), T("se.w2", (c, c // 8), -0.3, 0.3), T("se.b2", (c,), -0.1, 0.1)


def _hold_gate(got, ref64, ref32, what):
    e_gpu, e_cpu = float((got.double() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
    lim = max(4 * e_cpu, GATE_FLOOR)
    print(f"{what}: max |gate - float64| GPU {e_gpu:.3e}, torch fp32 on the CPU {e_cpu:.3e}, bound {lim:.3e}")
    assert bool(torch.isfinite(got).all()) and e_gpu <= lim, f"{what}: gate error {e_gpu:.3e} > {lim:.3e}"
    note("gate: error", "f32", e_gpu)
    note("gate: error / bound", "f32", e_gpu / lim)


@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_se_gates_against_float64(c):
    """eg_se_gate (from conv2's partials) and eg_se_gate_pre (from t1's window sums and border lines), on the GPU's own t1 and partials.  conv1's shift
    gives t1 a non-zero mean and BN2's shift is non-zero, so a border line taken from the wrong side moves the mean."""
    from emotiongestures_amd import _lib as L, ops
    from emotiongestures_amd._host import ptr, stream
    lib, d = L.load(), dev()
    rows = TILE_ROWS[c]
    w1, b1, w2, b2 = _se_weights(c)
    sw = [t.to(d) for t in (w1, b1, w2, b2)]
    for (B, H, W) in ((2, 2, 2), (3, 3, 5), (2, rows + 1, 33)):
        x = T(f"gx{c}", (B, c, H, W), -1, 1)
        wa, wb = T(f"w{c}a", (c, c, 3, 3), -0.1, 0.1), T(f"w{c}b", (c, c, 3, 3), -0.1, 0.1)
        s1, t1s = T("s1", (c,), 0.5, 1.5), T("t1", (c,), 0.2, 0.6)
        s2, t2s = T("s2", (c,), 0.5, 1.5), T("t2", (c,), -0.3, 0.3)
        xg = nhwc(x).to(d)
        t1, gap1 = ops.conv3x3(xg, wa, None, s1, t1s, relu=True, want_gap=True, precision="f32")
        c2 = ops.conv3x3_pack(wb, None, s2, t2s, d)
        tiles = int(lib.eg_conv3x3_gap_tiles(H, W, c, c, 1))
        assert gap1.shape == (B, tiles, c)
        t1c = t1.cpu().permute(0, 3, 1, 2).contiguous()
        what = f"C={c} B={B} {H}x{W}"

        def mean_bn2(dt):
            y = F.conv2d(t1c.to(dt), wb.to(dt), None, padding=1)
            return y.mean((2, 3)) * s2.to(dt) + t2s.to(dt), y

        m64, y64 = mean_bn2(torch.float64)
        m32, _ = mean_bn2(torch.float32)
        g64 = _gate_formula(m64, *(t.double() for t in (w1, b1, w2, b2)))
        g32 = _gate_formula(m32, w1, b1, w2, b2)
        gate, gbuf = C.guarded((B, c), d)
        L.check(lib.eg_se_gate_pre(ptr(t1), ptr(gap1), tiles, ptr(c2[0]), ptr(c2[2]), ptr(c2[3]), *(ptr(t) for t in sw), ptr(gate), B, H, W, c, stream(d)),
                "eg_se_gate_pre")
        torch.cuda.synchronize()
        assert C.guard_intact(gbuf, (B, c))
        _hold_gate(gate.cpu(), g64, g32, "eg_se_gate_pre " + what)
        # eg_se_gate on conv2's own partials (the GPU's): the float64 formula on their sum
        y2, gap2 = ops.conv3x3(t1, wb, None, s2, t2s, want_gap=True, precision="f32", packed=c2)
        gsum = gap2.cpu()
        p64 = _gate_formula(gsum.double().sum(1) / (H * W), *(t.double() for t in (w1, b1, w2, b2)))
        p32 = _gate_formula(gsum.sum(1) / (H * W), w1, b1, w2, b2)
        gate2, gbuf2 = C.guarded((B, c), d)
        L.check(lib.eg_se_gate(ptr(gap2), tiles, *(ptr(t) for t in sw), ptr(gate2), B, c, H * W, stream(d)), "eg_se_gate")
        torch.cuda.synchronize()
        assert C.guard_intact(gbuf2, (B, c))
        _hold_gate(gate2.cpu(), p64, p32, "eg_se_gate " + what)
        # and the two gates describe the same block: eg_se_gate's partials are sums of BN2(conv2(t1)) as well
        _hold_gate(gate2.cpu(), g64, g32, "eg_se_gate against the formula on t1 " + what)


def _shortcut64(x, dsw, dss, dsh, stride, prec="f32"):
    """-> (BN(conv1x1 stride s (x)) in float64 with the operands split as `prec` states, the same on absolute values)."""
    if prec == "f32":
        d = F.conv2d(x.double(), dsw.double(), None, stride=stride)
    else:
        (xh, xl), (wh, wl) = C.split_bf16(x), C.split_bf16(dsw)
        d = F.conv2d(xh, wh, None, stride=stride)
        if prec == "bf16x3":
            d = d + F.conv2d(xl, wh, None, stride=stride) + F.conv2d(xh, wl, None, stride=stride)
    a = F.conv2d(x.double().abs(), dsw.double().abs(), None, stride=stride)
    return d * dss.double().view(1, -1, 1, 1) + dsh.double().view(1, -1, 1, 1), a * dss.double().abs().view(1, -1, 1, 1) + dsh.double().abs().view(1, -1, 1, 1)


@pytest.mark.parametrize("cin,c,stride", [(32, 32, 1), (64, 64, 1), (128, 128, 1), (256, 256, 1), (32, 64, 2), (64, 128, 2), (128, 256, 2)])
def test_se_residual_relu_against_float64(cin, c, stride):
    """out = relu(y * gate + shortcut), shortcut = x or BN(conv1x1 stride 2 (x)): fp32 arithmetic, cin products and a handful of roundings per element:
    |d| <= (2 * cin_shortcut + 4) * 2^-24 * A."""
    from emotiongestures_amd import ops
    rows = 2 if stride == 2 or c == 256 else TILE_ROWS[c]
    B, Ho, Wo = 3, rows + 1, 33
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo)
    y, gate, x = T("ty", (B, c, Ho, Wo), -1, 1), T("tg", (B, c), 0, 1), T("tx", (B, cin, H, W), -1, 1)
    d = dev()
    if stride == 1:
        got = ops.se_residual_relu(nhwc(y).to(d), gate.to(d), nhwc(x).to(d))
        sc, sa, n = x.double(), x.double().abs(), 0
    else:
        dsw, dss, dsh = T("dw", (c, cin, 1, 1), -0.2, 0.2), T("ds", (c,), 0.5, 1.5), T("dh", (c,), -0.3, 0.3)
        got = ops.se_residual_relu(nhwc(y).to(d), gate.to(d), nhwc(x).to(d), dsw, dss.to(d), dsh.to(d), stride=2)
        (sc, sa), n = _shortcut64(x, dsw, dss, dsh, 2), cin
    g = gate.double()[:, :, None, None]
    ref, A = F.relu(y.double() * g + sc), y.double().abs() * g + sa
    r = C.check_map(got.cpu().permute(0, 3, 1, 2).double(), ref, (2 * n + 4) * C.U * A, f"eg_se_residual_relu {cin}->{c} stride {stride}")
    note("se_residual_relu", "f32", r)
    print(f"eg_se_residual_relu {cin}->{c} stride {stride}: worst error / bound {r:.3g}")


BLOCKS = [(32, 32, 1, ("f32", "bf16x3", "bf16")), (64, 64, 1, ("f32", "bf16x3")), (128, 128, 1, ("f32", "bf16x3")), (256, 256, 1, ("f32", "bf16x3")),
          (32, 64, 2, ("bf16x3", "bf16")), (64, 128, 2, ("bf16x3", "bf16"))]


@pytest.mark.parametrize("cin,c,stride,precs", BLOCKS, ids=[f"{a}-{b}" for a, b, _s, _p in BLOCKS])
def test_se_block_fused_launch_by_launch(cin, c, stride, precs):
    """eg_se_block_fused, each of its three launches on its own: t1 and conv1's partials against float64 of x; the gate (and a stage entry's shortcut vectors)
    against the float64 formula on the GPU's t1; out against float64 on the GPU's t1 and gate.  conv2 of a stage entry contracts the 1x1 shortcut D itself:
    acc = conv2 + D * f, out = relu(acc * q + h) with f = sd / q, q = gate * s2, h = shift2 * gate + hd; its bound counts the shortcut's 3 * cin (bf16x3; cin
    in bf16) products with the convolution's terms and adds 8 roundings for f, q and h."""
    from emotiongestures_amd import _lib as L, ops, packing
    from emotiongestures_amd._host import ptr, stream
    lib, d = L.load(), dev()
    rows1 = C.ROUTE_CASES[{(32, 32): "R_32", (64, 64): "R_64", (128, 128): "R_128", (256, 256): "R_256", (32, 64): "R_32_64", (64, 128): "R_64_128"}[(cin, c)]][2]
    rows2 = TILE_ROWS[c]
    B, Ho, Wo = 2, rows2 + 1, 33
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo)
    x, w1, _b, s1, _t, raw1 = C.case(cin, c, stride, B, H, W)
    t1s = T("t1", (c,), 0.2, 0.6)
    w2 = T(f"w{c}b", (c, c, 3, 3), -0.1, 0.1)
    s2, t2s = T("s2", (c,), 0.5, 1.5), T("t2", (c,), -0.3, 0.3)
    fw1, fb1, fw2, fb2 = _se_weights(c)
    sw = [t.to(d) for t in (fw1, fb1, fw2, fb2)]
    xg = nhwc(x).to(d)
    c1, c2 = ops.conv3x3_pack(w1, None, s1, t1s, d, stride), ops.conv3x3_pack(w2, None, s2, t2s, d)
    tiles = int(lib.eg_conv3x3_gap_tiles(H, W, cin, c, stride))
    dsw = dss = dsh = dimg = dssg = dshg = None
    if stride == 2:
        dsw, dss, dsh = T("dw", (c, cin, 1, 1), -0.2, 0.2), T("ds", (c,), 0.5, 1.5), T("dh", (c,), -0.3, 0.3)
        dimg, dssg, dshg = torch.from_numpy(packing._pack_conv1x1_bf16(dsw)).to(d), dss.to(d), dsh.to(d)
    for prec in precs:
        what = f"eg_se_block_fused {cin}->{c} stride {stride} {prec}"
        (t1, b_t1), (out, b_out), (gap, b_gap), (gate, b_gate) = (C.guarded(s, d) for s in ((B, Ho, Wo, c), (B, Ho, Wo, c), (B, tiles, c), (B, c)))
        scv, b_scv = C.guarded((3, B, c), d) if stride == 2 else (None, None)
        with env(EG_CONV_SPLIT=None, EG_CONV_S2=None):
            L.check(lib.eg_se_block_fused(ptr(xg), ptr(c1[0]), ptr(c1[2]), ptr(c1[3]), ptr(c2[0]), ptr(c2[2]), ptr(c2[3]), *(ptr(t) for t in sw), ptr(dimg),
                                          ptr(dssg), ptr(dshg), ptr(t1), ptr(out),
                                          ptr(gap), ptr(gate), ptr(scv), B, H, W, cin, c, stride, L.precision_code(prec), stream(d)), "eg_se_block_fused")
        torch.cuda.synchronize()
        for buf, shape in ((b_t1, (B, Ho, Wo, c)), (b_out, (B, Ho, Wo, c)), (b_gap, (B, tiles, c)), (b_gate, (B, c))) + (((b_scv, (3, B, c)),) if stride == 2 else ()):
            assert C.guard_intact(buf, shape), what
        # launch 1: t1 = BN1(relu(conv1(x))) and its partials
        t1c = t1.cpu().permute(0, 3, 1, 2).contiguous()
        r1 = hold(t1c.double(), gap.cpu().double(), raw1, prec, cin, rows1, what + " t1", relu=True, scale=s1, shift=t1s)
        # launch 2: the gate from the GPU's t1
        def mean_bn2(dt):
            return F.conv2d(t1c.to(dt), w2.to(dt), None, padding=1).mean((2, 3)) * s2.to(dt) + t2s.to(dt)
        g64 = _gate_formula(mean_bn2(torch.float64), *(t.double() for t in (fw1, fb1, fw2, fb2)))
        g32 = _gate_formula(mean_bn2(torch.float32), fw1, fb1, fw2, fb2)
        gc = gate.cpu()
        _hold_gate(gc, g64, g32, what + " gate")
        # launch 3: out from the GPU's t1 and gate
        raw2 = C.Raw(t1c, w2, 1)
        if stride == 1:
            r3 = hold(out.cpu().permute(0, 3, 1, 2).double(), None, raw2, prec, c, rows2, what + " out", scale=s2, shift=t2s, gate=gc, res=x)
        else:
            gq = gc.double()
            v = scv.cpu().double()
            q = gq * s2.double()
            for k, (ref, mag) in enumerate(((dss.double() / q, (dss.double() / q).abs()), (q, q.abs()), (t2s.double() * gq + dsh.double(), (t2s.double() * gq).abs() + dsh.double().abs()))):
                e = ((v[k] - ref).abs() / (4 * C.U * mag)).max()
                assert bool(torch.isfinite(v[k]).all()) and float(e) <= 1.0, f"{what}: shortcut vector {'fqh'[k]} is {float(e):.3g} x (4 * 2^-24 * |value|) off"
            g4 = gq[:, :, None, None]
            A = (raw2.abs * s2.double().abs().view(1, -1, 1, 1) + t2s.double().abs().view(1, -1, 1, 1)) * g4
            worst = 0.0
            for against in ("stated", "true") if prec == "bf16x3" else ("stated",):
                sc, sa = _shortcut64(x, dsw, dss, dsh, 2, prec if against == "stated" else "f32")
                acc = raw2.stated[prec] if against == "stated" else raw2.true
                ref = F.relu((acc * s2.double().view(1, -1, 1, 1) + t2s.double().view(1, -1, 1, 1)) * g4 + sc)
                n = C.terms(prec, c) + (3 if prec == "bf16x3" else 1) * cin
                bound = (2 * n + 8) * C.U * (A + sa) + (C.SPLIT_TERM * (A + sa) if against == "true" else 0.0)
                worst = max(worst, C.check_map(out.cpu().permute(0, 3, 1, 2).double(), ref, bound, f"{what} out against {against}"))
                note(f"block entry out against {against}", prec, worst)
            r3 = worst
        print(f"{what}: worst error / bound t1 {r1:.3g}, out {r3:.3g}")


@pytest.mark.parametrize("H,W", [(3, 5), (4, 33), (9, 65)])
def test_stem_conv_against_float64(H, W):
    from emotiongestures_amd import ops
    B, c = 2, 32
    x = T("spec", (B, H, W), -80, 0)
    w, b, s, t = T("w", (c, 1, 3, 3), -0.3, 0.3), T("b", (c,), -0.1, 0.1), T("s", (c,), 0.5, 1.5), T("t", (c,), -0.2, 0.2)
    d = dev()
    got = ops.stem_conv(x.to(d), w, b.to(d), s.to(d), t.to(d)).cpu().permute(0, 3, 1, 2).double()
    raw = C.Raw(x.unsqueeze(1), w, 1)
    ref = C.epilogue(raw.true, b, True, s, t)
    r = C.check_map(got, ref, C.elem_bound("f32", 1, C.epilogue_abs(raw.abs, b, s, t), ref), f"eg_stem_conv {H}x{W}")
    note("stem", "f32", r)
    print(f"eg_stem_conv {H}x{W}: worst error / bound {r:.3g}")


# ---- what was launched ------------------------------------------------------------------------------------------------------------------------
def test_every_route_form_and_padded_count_was_launched():
    """From the record of the tests above (same process, module order): every route of csrc/conv.hip at each of its output-channel counts in every layout the
    count allows, every replacing form under its own name, eg_conv3x3_se on every stride-1 count it serves."""
    want = {}
    for name, (_cin, stride, _rows, couts) in C.ROUTE_CASES.items():
        w = want.setdefault(name, set())
        for cout in couts:
            w.add((cout, "nchw"))
            if cout % 4 == 0:
                w.add((cout, "nhwc"))
                if stride == 1:
                    w.add((cout, "se"))
    for c, name in ((64, "R_64"), (128, "R_128")):
        want[name] |= {(c, f"split={s}") for s in ("1", "2", "4", None)}
    for cout, name in ((64, "R_32_64"), (128, "R_64_128")):
        want[name] |= {(cout, f"s2={f}") for f in ("interleaved", "planes4", "planes8", None)}
    want["R_32"] |= {(32, f"persistent tiles={n}") for n in (9, 512, 520)}
    assert set(want) == {"R_32", "R_32_NARROW", "R_32_64", "R_64", "R_64_128", "R_64_128_S1", "R_128", "R_128_64", "R_128_48", "R_128_256", "R_256"}
    missing = {name: sorted(w - LAUNCHED.get(name, set()), key=str) for name, w in want.items() if w - LAUNCHED.get(name, set())}
    assert not missing, f"not launched by this module's tests: {missing}"
    for (kind, prec), r in sorted(WORST.items()):
        print(f"worst over the module: {kind} [{prec}] {r:.3g}")
