"""The channels-last 1-D convolutions of the training path on the GPU -- eg_conv1d_cl_forward, eg_conv1d_cl_backward_input and
eg_conv1d_cl_backward_weight of csrc/conv1d_train.hip -- called through the C ABI, every ELEMENT against torch's conv1d and its autograd in float64
within the a-priori bound of tests/grads_f64.py (case list with the kernel each entry point takes per case: the untiled kernels, the six CPW
instantiations of the two tiled ones, the one-launch weight gradient, its three tiled instantiations and the fold; tests/test_grads_f64.py checks
those routes against the restated launch conditions and shows that the bounds reject a tap read across the tile seam, a partial left out of the
fold and a bias added twice).

Every output is the middle of a buffer filled with one NaN bit pattern; after a call everything around the result must still hold it, the guard
behind the workspace (exactly eg_conv1d_cl_backward_weight_workspace_floats long) included."""
import pytest
import torch

import grads_f64 as G

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5
GUARD = 256
BAD_ARG, WORKSPACE = -1, -3
_REF = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, _stream(dev())


def canary(n):
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[GUARD:]


def result(buf, shape, what):
    n = 1
    for s in shape:
        n *= s
    b = buf.cpu()
    assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all()), f"{what}: stores around the result"
    return b[GUARD:GUARD + n].clone().view(torch.float32).view(shape)


def reference(c):
    if c not in _REF:
        _REF[c] = (G.c1_inputs(c), G.c1_f64(c))
    return _REF[c]


def geometry(c, lo):
    return (c.b, c.l, c.ci, lo, c.co, c.k, c.stride, c.pad, c.dil)


def report(entry, worst):
    print(f"FRACTION {entry} {worst:.3f}")


IDS = ["b{0}_l{1}_ci{2}_co{3}_k{4}_s{5}_p{6}_d{7}".format(*c[:8]) for c in G.C1_CASES]


@pytest.mark.parametrize("c", G.C1_CASES, ids=IDS)
def test_conv1d_cl_forward_matches_float64_per_element(c):
    """conv1d_cl_fwd_tiled_kernel<CPW> / conv1d_cl_fwd_kernel as c.fwd states; with and without bias."""
    L, lib, _ptr, st = _api()
    (x, w, by, bx, dy, lo), r = reference(c)
    xd, wd, bd = x.to(dev()), w.to(dev()), by.to(dev())
    worst = 0.0
    for bias, ref, bound in ((bd, r["y"], r["b_y"]), (None, r["y0"], r["b_y0"])):
        what = f"eg_conv1d_cl_forward {tuple(c[:8])} ({c.fwd}) bias {bias is not None}"
        buf, y = canary(c.b * lo * c.co)
        L.check(lib.eg_conv1d_cl_forward(_ptr(xd), _ptr(wd), _ptr(bias), _ptr(y), *geometry(c, lo), st), what)
        torch.cuda.synchronize()
        worst = max(worst, G.compare_sliced(result(buf, (c.b, lo, c.co), what), ref, bound, what, G.C1_AXES)[2])
    report("eg_conv1d_cl_forward", worst)


@pytest.mark.parametrize("c", G.C1_CASES, ids=IDS)
def test_conv1d_cl_backward_input_matches_float64_per_element(c):
    """conv1d_cl_bwd_input_tiled_kernel<CPW> / conv1d_cl_bwd_input_kernel as c.dx states; without bias (the Conv1d input gradient) and WITH one (the
    ConvTranspose1d forward)."""
    L, lib, _ptr, st = _api()
    (x, w, by, bx, dy, lo), r = reference(c)
    dyd, wd, bd = dy.to(dev()), w.to(dev()), bx.to(dev())
    worst = 0.0
    for bias, ref, bound in ((None, r["dx0"], r["b_dx0"]), (bd, r["dx"], r["b_dx"])):
        what = f"eg_conv1d_cl_backward_input {tuple(c[:8])} ({c.dx}) bias {bias is not None}"
        buf, dx = canary(c.b * c.l * c.ci)
        L.check(lib.eg_conv1d_cl_backward_input(_ptr(dyd), _ptr(wd), _ptr(bias), _ptr(dx), *geometry(c, lo), st), what)
        torch.cuda.synchronize()
        worst = max(worst, G.compare_sliced(result(buf, (c.b, c.l, c.ci), what), ref, bound, what, G.C1_AXES)[2])
    report("eg_conv1d_cl_backward_input", worst)


def run_weight(c, want_db_dy=True, want_db_x=False):
    """One eg_conv1d_cl_backward_weight call -> (dw, db_dy or None, db_x or None), canaries checked."""
    L, lib, _ptr, st = _api()
    (x, w, by, bx, dy, lo), r = reference(c)
    xd, dyd = x.to(dev()), dy.to(dev())
    what = f"eg_conv1d_cl_backward_weight {tuple(c[:8])} ({'dw_one' if want_db_x else c.dw}) db_dy {want_db_dy} db_x {want_db_x}"
    need = int(lib.eg_conv1d_cl_backward_weight_workspace_floats(c.b, c.ci, lo, c.co, c.k, c.stride, c.dil))
    assert need == G.c1_weight_workspace_floats(c.b, c.ci, lo, c.co, c.k, c.stride, c.dil), f"{what}: the library asks for {need} workspace floats"
    wbuf, dw = canary(c.co * c.ci * c.k)
    ybuf, db_dy = canary(c.co)
    xbuf, db_x = canary(c.ci)
    sbuf = torch.full((need + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    L.check(lib.eg_conv1d_cl_backward_weight(_ptr(xd), _ptr(dyd), _ptr(dw), _ptr(db_dy) if want_db_dy else None, _ptr(db_x) if want_db_x else None,
                                             *geometry(c, lo), _ptr(sbuf) if need else None, need, st), what)
    torch.cuda.synchronize()
    assert bool((sbuf[need:] == SENTINEL).all()), f"{what}: a store behind the {need} workspace floats"
    if want_db_x:
        assert bool((sbuf == SENTINEL).all()), f"{what}: db_x takes the one-launch kernel, yet the workspace was written"
    out = [result(wbuf, (c.co, c.ci, c.k), what)]
    for buf, want, n in ((ybuf, want_db_dy, c.co), (xbuf, want_db_x, c.ci)):
        if want:
            out.append(result(buf, (n,), what))
        else:
            assert bool((buf == SENTINEL).all()), f"{what}: a bias gradient written without being asked for"
            out.append(None)
    return out, what, r


@pytest.mark.parametrize("c", G.C1_CASES, ids=IDS)
def test_conv1d_cl_backward_weight_matches_float64_per_element(c):
    """conv1d_cl_bwd_weight_kernel, or conv1d_cl_bwd_weight_tiled_kernel<COB> + conv1d_cl_bwd_weight_fold_kernel over the stated number of partials."""
    (dw, db_dy, _), what, r = run_weight(c)
    worst = G.compare_sliced(dw, r["dw"], r["b_dw"], what + " dw", ("output channel", "input channel", "tap"))[2]
    worst = max(worst, G.compare_sliced(db_dy, r["db_dy"], r["b_db_dy"], what + " db_dy", ("channel",))[2])
    (dw2, db2, _), _, _ = run_weight(c)
    assert torch.equal(dw2.view(torch.int32), dw.view(torch.int32)) and torch.equal(db2.view(torch.int32), db_dy.view(torch.int32)), f"{what}: two runs differ"
    report("eg_conv1d_cl_backward_weight", worst)


@pytest.mark.parametrize("c", G.C1_DBX_CASES, ids=lambda c: "b{0}_l{1}_ci{2}_co{3}".format(*c[:4]))
def test_conv1d_cl_backward_weight_bias_outputs(c):
    """db_x requested (the ConvTranspose1d bias gradient): always the one-launch kernel, the workspace untouched; db_dy = NULL on the tiled route: the
    fold skips the bias column."""
    (dw, db_dy, db_x), what, r = run_weight(c, want_db_dy=True, want_db_x=True)
    worst = G.compare_sliced(dw, r["dw"], r["b_dw"], what + " dw", ("output channel", "input channel", "tap"))[2]
    worst = max(worst, G.compare_sliced(db_dy, r["db_dy"], r["b_db_dy"], what + " db_dy", ("channel",))[2])
    worst = max(worst, G.compare_sliced(db_x, r["db_x"], r["b_db_x"], what + " db_x", ("channel",))[2])
    (dw, _, _), what, r = run_weight(c, want_db_dy=False)
    worst = max(worst, G.compare_sliced(dw, r["dw"], r["b_dw"], what + " dw", ("output channel", "input channel", "tap"))[2])
    report("eg_conv1d_cl_backward_weight[bias outputs]", worst)


def test_conv1d_cl_refusals_leave_the_outputs_untouched():
    """k = 9, a len_out that does not fit len, stride 0 -> EG_ERR_BAD_ARG from all three entry points; a workspace one float short on the tiled weight
    route -> EG_ERR_WORKSPACE; nothing is written."""
    L, lib, _ptr, st = _api()
    c = next(c for c in G.C1_CASES if c.dw == "dw_tiled<8>/8")
    (x, w, by, bx, dy, lo), _ = reference(c)
    xd, wd, dyd = x.to(dev()), torch.zeros(c.co, c.ci, 9, device=dev()), dy.to(dev())
    need = G.c1_weight_workspace_floats(c.b, c.ci, lo, c.co, c.k, c.stride, c.dil)
    bufs = [canary(max(c.b * lo * c.co, c.b * c.l * c.ci, c.co * c.ci * 9))[0] for _ in range(3)]
    ybuf, dxbuf, dwbuf = bufs
    y, dx, dw = (b.view(torch.float32)[GUARD:] for b in bufs)
    sbuf = torch.full((need + GUARD,), SENTINEL, dtype=torch.int32, device=dev())

    def calls(lo_=lo, k=c.k, stride=c.stride, wsn=need):
        geo = (c.b, c.l, c.ci, lo_, c.co, k, stride, c.pad, c.dil)
        return (lib.eg_conv1d_cl_forward(_ptr(xd), _ptr(wd), None, _ptr(y), *geo, st),
                lib.eg_conv1d_cl_backward_input(_ptr(dyd), _ptr(wd), None, _ptr(dx), *geo, st),
                lib.eg_conv1d_cl_backward_weight(_ptr(xd), _ptr(dyd), _ptr(dw), None, None, *geo, _ptr(sbuf), wsn, st))

    for what, rcs, want in (("k = 9", calls(k=9), (BAD_ARG,) * 3), ("len_out too long", calls(lo_=lo + 1), (BAD_ARG,) * 3), ("stride 0", calls(stride=0), (BAD_ARG,) * 3)):
        assert tuple(rcs) == want, f"{what}: status {rcs}, expected {want} ({lib.eg_last_error().decode()})"
        torch.cuda.synchronize()
        assert all(bool((b == SENTINEL).all()) for b in bufs + [sbuf]), f"{what}: something was written"
    rc = lib.eg_conv1d_cl_backward_weight(_ptr(xd), _ptr(dyd), _ptr(dw), None, None, c.b, c.l, c.ci, lo, c.co, c.k, c.stride, c.pad, c.dil, _ptr(sbuf), need - 1, st)
    assert rc == WORKSPACE, f"workspace one float short: status {rc} ({lib.eg_last_error().decode()})"
    torch.cuda.synchronize()
    assert bool((dwbuf == SENTINEL).all()) and bool((sbuf == SENTINEL).all()), "workspace one float short: something was written"
    assert calls() == (0, 0, 0)
    torch.cuda.synchronize()


def test_pad_cols_is_bitwise_a_zero_padded_copy():
    """pad_cols_kernel (the ninth kernel of the file): [rows, k] -> [rows, k_padded], zeros in the padding, nothing behind."""
    L, lib, _ptr, st = _api()
    for rows, k, kp in ((1, 1, 4), (5, 126, 128), (300, 282, 284), (7, 64, 64)):
        x = G.T(f"pad{rows}x{k}", (rows, k))
        xd = x.to(dev())
        buf, y = canary(rows * kp)
        L.check(lib.eg_pad_cols(_ptr(xd), _ptr(y), rows, k, kp, st), "eg_pad_cols")
        torch.cuda.synchronize()
        got = result(buf, (rows, kp), f"eg_pad_cols {rows}x{k}->{kp}")
        want = torch.zeros(rows, kp)
        want[:, :k] = x
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
