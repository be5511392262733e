"""small_linear_kernel and convt1d_kernel of csrc/misc.hip -- the CVAE chain's siblings of eg_conv1d -- on the GPU through eg_small_linear and
eg_conv_transpose1d, every ELEMENT against float64 (tests/misc_f64.py sections 3 and 4).  Outputs in canary-guarded buffers, inputs in NaN-filled
ones: the gap between In and ldx is NaN, and so is what follows the last input position of every row."""
import pytest
import torch

import misc_f64 as M
import misc_gpu as G
import train_tail_gpu as D

pytestmark = pytest.mark.gpu
_ID = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("case", M.SL_CASES, ids=_ID)
def test_small_linear_matches_float64_per_element(case):
    """One wave per output: In below, at and past 64 and 128 (a lane's chain of one, two and three terms), outputs past the 64 workgroups of the grid
    (Out = 512: a workgroup's second turn), y written at a column offset into wider rows whose other columns must keep their canary."""
    L, lib, ptr, st = D.api()
    n, In, Out, ldx, ldy, col = case
    x, w, b = M.sl_inputs(case)
    what = f"small_linear {case}"
    y = D.Guarded((n, ldy))
    xd, wd, bd = G.up_nan(x, ldx), G.up_nan(w), G.up_nan(b)
    L.check(lib.eg_small_linear(ptr(xd), ldx, ptr(wd), ptr(bd), ptr(y.t[0, col:]), ldy, n, In, Out, st), what)
    got = y.intact(what)
    last = min(ldy, col + Out)
    D.frac("small_linear", got[:, col:last], M.sl_eval(x, w, b)[:, :last - col], M.sl_bound(x, w, b)[:, :last - col], what, ("row", "output"))
    keep = torch.ones(n, ldy, dtype=torch.bool)
    keep[:, col:last] = False
    assert bool((G.bits(got)[keep] == D.SENTINEL).all()), what + ": columns outside the outputs were written"
    D.report("small_linear")


@pytest.mark.parametrize("case", M.CT_CASES, ids=_ID)
def test_conv_transpose1d_matches_float64_per_element(case):
    """ConvTranspose1d(k 3, stride 2, padding 1, output_padding 1) -> LeakyReLU -> affine: lin on both sides of the 128-output workgroup, lin = 1.  The
    first output has no tap 2 term (t < 0) and the last odd one no tap 0 term (li = lin): both are dropped, not multiplied by zero -- x[lin] is the
    next row's first element, or NaN behind the last row."""
    L, lib, ptr, st = D.api()
    n, cin, cout, lin = case
    x, w, b, sc, sh = M.ct_inputs(case)
    what = f"conv_transpose1d {case}"
    y = D.Guarded((n, cout, 2 * lin))
    dev = [G.up_nan(t) for t in (x, w, b, sc, sh)]
    L.check(lib.eg_conv_transpose1d(*(ptr(t) for t in dev), ptr(y.t), n, cin, cout, lin, st), what)
    D.frac("conv_transpose1d", y.intact(what), M.ct_f64(x, w, b, sc, sh), M.ct_bound(x, w, b, sc, sh), what, M.CT_AXES)
    D.report("conv_transpose1d")
