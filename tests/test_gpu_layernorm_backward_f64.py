"""LayerNorm backward on the GPU -- eg_layernorm_backward (ln_bwd_kernel, one wave per row) and eg_layernorm_backward_ex (ln_bwd_ex_kernel<NV>: a wave
walks rows-per-wave rows, the affine gradients come from the same pass through per-workgroup partials and col_finalize_kernel) of csrc/train.hip --
called through the C ABI, every ELEMENT against the float64 autograd of layer_norm (tests/grads_f64.py: reference, tolerances, case lists):
    dx          within 4 x the error of torch's float32 CPU backward on the same inputs (LN_BWD_CPU_F32, in layernorm_scale units);
    xhat        (plain entry) within the forward LayerNorm tolerance of small_ops_f64.py per row class: a constant row gives xhat = 0 exactly;
    dgamma / dbeta   within their a-priori bounds;
    dx_dropped  BITWISE oracle.dropout_keep_mask applied to the returned dx with the fp32 scale 1 / (1 - p).
Outputs sit in buffers filled with one NaN bit pattern (a row before and after, guards around the vectors, a guard behind the workspace, which is
exactly eg_layernorm_backward_ex_workspace_floats long): every slot outside the result must keep it."""
import numpy as np
import pytest
import torch

import grads_f64 as G
from oracle import emogest_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5
GUARD = 256
BAD_ARG, UNSUPPORTED = -1, -2
_REF = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, _stream(dev())


def canary2(rows, d):
    buf = torch.full((rows + 2, d), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[1:]


def canary1(n):
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[GUARD:]


def result2(buf, rows, what):
    b = buf.cpu()
    assert bool((b[0] == SENTINEL).all()) and bool((b[rows + 1] == SENTINEL).all()), f"{what}: stores in front of or behind the rows"
    return b[1:rows + 1].clone().view(torch.float32)


def result1(buf, n, what):
    b = buf.cpu()
    assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all()), f"{what}: stores around the vector"
    return b[GUARD:GUARD + n].clone().view(torch.float32)


def reference(rows, d, cls):
    """One float64 reference per (rows, D, class) for the whole module."""
    key = (rows, d, cls)
    if key not in _REF:
        x, dy, g, row_cls = G.lnb_inputs(rows, d, cls)
        _REF[key] = (x, dy, g, row_cls) + G.lnb_f64(x, dy, g) + (G.lnb_dx_scale(x, g),)
    return _REF[key]


def check_dx(got, ref, scale, tol, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    return G.compare_sliced(got, ref, tol * scale, what, G.LNB_AXES)[2]


def report(entry, worst):
    print(f"FRACTION {entry} {worst:.3f}")


@pytest.mark.parametrize("rows,d", G.LNB_PLAIN_CASES)
def test_layernorm_backward_matches_float64_per_element(rows, d):
    """ln_bwd_kernel: ceil(rows / 4) workgroups, lanes stride the row by 64 (D = 2: 62 idle lanes; 63 / 65: one short / one extra stride); the three
    input classes."""
    for cls in G.LNB_CLASSES:
        plain_case(rows, d, cls)


def plain_case(rows, d, cls):
    L, lib, _ptr, st = _api()
    x, dy, g, row_cls, rdx, rxhat, _, _, scale = reference(rows, d, cls)
    what = f"eg_layernorm_backward {rows}x{d} {cls}"
    xbuf, dx = canary2(rows, d)
    hbuf, xhat = canary2(rows, d)
    xd, dyd, gd = x.to(dev()), dy.to(dev()), g.to(dev())
    L.check(lib.eg_layernorm_backward(_ptr(xd), _ptr(dyd), _ptr(gd), _ptr(dx), _ptr(xhat), rows, d, G.LNB_EPS, st), what)
    torch.cuda.synchronize()
    which = "plain2" if d == 2 else "plain"
    report(f"eg_layernorm_backward dx[{cls}]", check_dx(result2(xbuf, rows, what), rdx, scale, G.lnb_dx_tol(which, cls), what + " dx"))
    got = result2(hbuf, rows, what)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite xhat"
    report(f"eg_layernorm_backward xhat[{cls}]", G.compare_sliced(got, rxhat, G.lnb_xhat_tol(x, row_cls, cls=cls), what + " xhat", G.LNB_AXES)[2])


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("rows,d,rw", G.LNB_EX_CASES)
def test_layernorm_backward_ex_matches_float64_per_element(rows, d, rw, p):
    """ln_bwd_ex_kernel<2> (D <= 512) / <4>: rows-per-wave rw = 1, 2, 3 and the clamp at 8 as grads_f64.LNB_EX_CASES states; partial and full lane
    coverage of both NV; the last workgroup's waves without rows; the Dropout'ed second output; the three input classes."""
    for cls in G.LNB_CLASSES:
        ex_case(rows, d, rw, cls, p)


def ex_case(rows, d, rw, cls, p):
    L, lib, _ptr, st = _api()
    x, dy, g, row_cls, rdx, _, rdg, rdb, scale = reference(rows, d, cls)
    what = f"eg_layernorm_backward_ex {rows}x{d} rw {rw} {cls} p {p}"
    need = int(lib.eg_layernorm_backward_ex_workspace_floats(rows, d))
    assert need == G.ln_ex_workspace_floats(rows, d), f"{what}: the library asks for {need} workspace floats"
    xbuf, dx = canary2(rows, d)
    mbuf, dxm = canary2(rows, d)
    gbuf, dg = canary1(d)
    bbuf, db = canary1(d)
    sbuf = torch.full((need + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    xd, dyd, gd = x.to(dev()), dy.to(dev()), g.to(dev())
    L.check(lib.eg_layernorm_backward_ex(_ptr(xd), _ptr(dyd), _ptr(gd), _ptr(dx), _ptr(dxm) if p > 0 else None, _ptr(dg), _ptr(db),
                                         rows, d, G.LNB_EPS, p, G.LNB_SEED, G.LNB_OFFSET, None, _ptr(sbuf), st), what)
    torch.cuda.synchronize()
    assert bool((sbuf[need:] == SENTINEL).all()), f"{what}: a store behind the {need} workspace floats"
    assert bool(torch.isfinite(sbuf[:need].view(torch.float32)).all()), f"{what}: a partial was not written"
    got = result2(xbuf, rows, what)
    report(f"eg_layernorm_backward_ex dx[{cls}]", check_dx(got, rdx, scale, G.lnb_dx_tol("ex", cls), what + " dx"))
    bg, bb = G.lnb_affine_bounds(x, dy, row_cls)
    report("eg_layernorm_backward_ex dgamma", G.compare_sliced(result1(gbuf, d, what), rdg, bg, what + " dgamma", ("column",))[2])
    report("eg_layernorm_backward_ex dbeta", G.compare_sliced(result1(bbuf, d, what), rdb, bb, what + " dbeta", ("column",))[2])
    if p > 0:
        keep = torch.from_numpy(O.dropout_keep_mask(G.LNB_SEED, G.LNB_OFFSET, rows * d, p)).view(rows, d)
        inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        want = torch.where(keep, got * inv, torch.zeros_like(got))
        assert torch.equal(result2(mbuf, rows, what).view(torch.int32), want.view(torch.int32)), f"{what}: dx_dropped is not the mask applied to dx"
        assert 0.7 < float(keep.double().mean()) < 0.9 or rows * d < 2000
    else:
        assert bool((mbuf == SENTINEL).all()), f"{what}: dx_dropped written at p = 0"


def test_layernorm_backward_ex_refusals_leave_the_outputs_untouched():
    """D = 96 (not a multiple of 64) and D = 1088 (> 1024) -> EG_ERR_UNSUPPORTED; p > 0 without dx_dropped and p = 0 with it -> EG_ERR_BAD_ARG."""
    L, lib, _ptr, st = _api()
    rows = 5
    x = torch.zeros(rows, 1088, device=dev())
    g = torch.ones(1088, device=dev())
    xbuf, dx = canary2(rows, 1088)
    mbuf, dxm = canary2(rows, 1088)
    gbuf, dg = canary1(1088)
    bbuf, db = canary1(1088)
    ws = torch.full((4 * 1088 + GUARD,), SENTINEL, dtype=torch.int32, device=dev())

    def call(d=64, p=0.0, dropped=None):
        return lib.eg_layernorm_backward_ex(_ptr(x), _ptr(x), _ptr(g), _ptr(dx), dropped, _ptr(dg), _ptr(db), rows, d, G.LNB_EPS, p, 1, 0, None, _ptr(ws), st)

    for what, rc, want in (("D = 96", call(d=96), UNSUPPORTED), ("D = 1088", call(d=1088), UNSUPPORTED), ("p > 0, dx_dropped = NULL", call(p=0.2), BAD_ARG),
                           ("p = 0 with dx_dropped", call(dropped=_ptr(dxm)), BAD_ARG)):
        assert rc == want, f"{what}: status {rc}, expected {want} ({lib.eg_last_error().decode()})"
        torch.cuda.synchronize()
        assert all(bool((b == SENTINEL).all()) for b in (xbuf, mbuf, gbuf, bbuf, ws)), f"{what}: something was written"
    assert call() == 0 and call(p=0.2, dropped=_ptr(dxm)) == 0
    torch.cuda.synchronize()
