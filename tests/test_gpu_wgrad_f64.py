"""The weight-gradient products on the GPU -- eg_linear_wgrad_mfma (csrc/lingrad.hip), eg_gemm_tn and eg_colsum (csrc/train.hip) -- called through the
C ABI at the shapes where their row split, XCD tile remap, split-K and ragged-tile paths change, every ELEMENT of dW, db and C against the float64
restatement of tests/grads_f64.py within its a-priori bound (reference, bounds, case lists with the route of each case are there;
tests/test_grads_f64.py shows on the CPU that the bounds reject a dropped 32-row group, a lo x hi term lost in one 16 x 16 tile, a slice left out of
the fold, db short of 16 rows in one column quad and db taken from the un-remapped tile).

Every output is the middle of a buffer filled with one NaN bit pattern -- a row before and after, the pitch-gap columns, guards around db, a guard
behind the workspace, which is passed at exactly the size the library asks for: after the call every slot outside the result must still hold the
pattern bit for bit.  The gaps of strided inputs hold NaN.  Each test prints the worst element it saw as a fraction of the bound."""
import pytest
import torch

import grads_f64 as G

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5           # a quiet NaN no arithmetic produces
GUARD = 256
BAD_ARG, WORKSPACE = -1, -3


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, _stream(dev())


def strided(t, ld, off=0):
    """t [rows, cols] -> a device view [rows, ld] whose gap columns (and the floats around it) hold NaN, starting `off` floats into its buffer."""
    rows, cols = t.shape
    flat = torch.full((rows * ld + off + 4,), float("nan"), device=dev())
    view = flat[off:off + rows * ld].view(rows, ld)
    view[:, :cols] = t.to(dev())
    return view


def canary2(rows, ld):
    buf = torch.full((rows + 2, ld), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[1:]


def canary1(n):
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[GUARD:]


def result2(buf, m, n, what):
    b = buf.cpu()
    out = b[1:m + 1, :n].clone()
    b[1:m + 1, :n] = SENTINEL
    bad = (b != SENTINEL).nonzero()
    assert bad.numel() == 0, f"{what}: stores outside [0:{m}, 0:{n}], first at buffer row {int(bad[0, 0]) - 1}, column {int(bad[0, 1])}"
    return out.view(torch.float32)


def result1(buf, n, what):
    b = buf.cpu()
    assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all()), f"{what}: stores around the vector"
    return b[GUARD:GUARD + n].clone().view(torch.float32)


def workspace(need):
    """-> (buffer of need + GUARD sentinel words, pointer view or None).  The guard behind `need` must survive the call."""
    buf = torch.full((need + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    return buf, (buf.view(torch.float32) if need else None)


def report(entry, worst):
    print(f"FRACTION {entry} {worst:.3f}")


# ---- eg_linear_wgrad_mfma ---------------------------------------------------------------------------------------------------------------------
def run_wgrad(c, dy, x):
    L, lib, _ptr, st = _api()
    ldy, ldx, lddw, off, with_db = G.wg_layout(c.layout, c.n, c.k)
    what = f"eg_linear_wgrad_mfma {c.rows}x{c.n}x{c.k} {c.layout}"
    need = int(lib.eg_linear_wgrad_mfma_workspace_floats(c.rows, c.n, c.k))
    assert need == G.lingrad_workspace_floats(c.rows, c.n, c.k), f"{what}: the library asks for {need} workspace floats"
    dyd, xd = strided(dy, ldy, off), strided(x, ldx, off)
    wbuf, dw = canary2(c.n, lddw)
    bbuf, db = canary1(c.n)
    sbuf, ws = workspace(need)
    L.check(lib.eg_linear_wgrad_mfma(_ptr(dyd), ldy, _ptr(xd), ldx, _ptr(dw), lddw, _ptr(db) if with_db else None, c.rows, c.n, c.k,
                                     _ptr(ws) if need else None, need, st), what)
    torch.cuda.synchronize()
    assert bool((sbuf[need:] == SENTINEL).all()), f"{what}: a store behind the {need} workspace floats"
    got_w = result2(wbuf, c.n, c.k, what + " dW")
    if with_db:
        got_b = result1(bbuf, c.n, what + " db")
    else:
        assert bool((bbuf == SENTINEL).all()), f"{what}: db written without being asked for"
        got_b = None
    return got_w, got_b, what


@pytest.mark.parametrize("idx", range(len(G.WGRAD_CASES)), ids=lambda i: "{0}x{1}x{2}-{3}".format(*G.WGRAD_CASES[i][:4]))
def test_linear_wgrad_matches_float64_per_element(idx):
    """linear_wgrad_bf16_kernel<false> (+ linear_wgrad_reduce_kernel when plan_lingrad splits the rows): S, rows_per and the XCD blocking of each case
    are stated in grads_f64.WGRAD_CASES.  dW and db per element; db at every n tile (under the remap it comes from the workgroups whose REMAPPED
    tx is 0); two runs bitwise equal."""
    c = G.WGRAD_CASES[idx]
    dy, x = G.wgrad_inputs(c.rows, c.n, c.k)
    got_w, got_b, what = run_wgrad(c, dy, x)
    ref_w, ref_b = G.wgrad_f64(dy, x)
    bw, bb = G.wgrad_bounds(dy, x, G.E_X3, c.S)
    worst = G.compare_sliced(got_w, ref_w, bw, what + " dW", G.WG_AXES)[2]
    report("eg_linear_wgrad_mfma dW", worst)
    if got_b is not None:
        report("eg_linear_wgrad_mfma db", G.compare_sliced(got_b, ref_b, bb, what + " db", ("column",))[2])
    again_w, again_b, _ = run_wgrad(c, dy, x)
    assert torch.equal(again_w.view(torch.int32), got_w.view(torch.int32)), f"{what}: two runs differ in dW"
    assert got_b is None or torch.equal(again_b.view(torch.int32), got_b.view(torch.int32)), f"{what}: two runs differ in db"


def test_linear_wgrad_refusals_leave_the_outputs_untouched():
    """ldy < N, ldx < K, lddw < K, rows = 0, a null dY / X / dW -> EG_ERR_BAD_ARG; a workspace one float short (or none) when the rows are split ->
    EG_ERR_WORKSPACE; all on the host before any launch: dW, db and the workspace keep the sentinel."""
    L, lib, _ptr, st = _api()
    rows, n, k = 1100, 64, 64
    need = G.lingrad_workspace_floats(rows, n, k)
    assert need > 0
    dy, x = (t.to(dev()) for t in G.wgrad_inputs(rows, n, k))
    wbuf, dw = canary2(n, k)
    bbuf, db = canary1(n)
    sbuf, ws = workspace(need)

    def call(dy_p=_ptr(dy), x_p=_ptr(x), dw_p=_ptr(dw), ldy=n, ldx=k, lddw=k, r=rows, ws_p=_ptr(ws), wsn=need):
        return lib.eg_linear_wgrad_mfma(dy_p, ldy, x_p, ldx, dw_p, lddw, _ptr(db), r, n, k, ws_p, wsn, st)

    for what, rc, want in (("ldy < N", call(ldy=n - 1), BAD_ARG), ("ldx < K", call(ldx=k - 1), BAD_ARG), ("lddw < K", call(lddw=k - 1), BAD_ARG),
                           ("rows = 0", call(r=0), BAD_ARG), ("dY = NULL", call(dy_p=None), BAD_ARG), ("X = NULL", call(x_p=None), BAD_ARG),
                           ("dW = NULL", call(dw_p=None), BAD_ARG), ("workspace one float short", call(wsn=need - 1), WORKSPACE),
                           ("workspace = NULL", call(ws_p=None), WORKSPACE)):
        assert rc == want, f"{what}: status {rc}, expected {want} ({lib.eg_last_error().decode()})"
        torch.cuda.synchronize()
        assert bool((wbuf == SENTINEL).all()) and bool((bbuf == SENTINEL).all()) and bool((sbuf == SENTINEL).all()), f"{what}: something was written"
    assert call() == 0                      # the same buffers are accepted once the arguments are right
    torch.cuda.synchronize()
    assert bool(torch.isfinite(result2(wbuf, n, k, "accepted call")).all())
    # without the split a one-float (or no) workspace is enough
    assert lib.eg_linear_wgrad_mfma(_ptr(dy), n, _ptr(x), k, _ptr(dw), k, _ptr(db), 640, n, k, None, 0, st) == 0
    torch.cuda.synchronize()


# ---- eg_gemm_tn -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(G.TN_CASES)), ids=lambda i: "{0}x{1}x{2}-{3}-acc{4}".format(*G.TN_CASES[i][:5]))
def test_gemm_tn_matches_float64_per_element(idx):
    """gemm_tn_kernel<false> (+ tn_reduce_kernel when K is split or C accumulates): C = A^T B (+ C_prev), exact fp32 products, E = 0.  The workspace is
    exactly what the library asks for (m n floats when only `accumulate` needs one); slices behind nz stay untouched."""
    L, lib, _ptr, st = _api()
    c = G.TN_CASES[idx]
    a, b, prev = G.gemm_tn_inputs(c.m, c.n, c.k)
    lda, ldb, ldc = G.tn_layout(c.layout, c.m, c.n)
    what = f"eg_gemm_tn {c.m}x{c.n}x{c.k} {c.layout} accumulate {c.accumulate}"
    need = int(lib.eg_gemm_tn_workspace_floats(c.m, c.n, c.k))
    assert need == G.gemm_tn_workspace_floats(c.m, c.n, c.k), f"{what}: the library asks for {need} workspace floats"
    need = max(need, c.m * c.n if c.accumulate else 0)
    ad, bd = strided(a, lda), strided(b, ldb)
    cbuf, cd = canary2(c.m, ldc)
    if c.accumulate:
        cd[:c.m, :c.n] = prev.to(dev())
    sbuf, ws = workspace(need)
    L.check(lib.eg_gemm_tn(_ptr(ad), lda, _ptr(bd), ldb, _ptr(cd), ldc, c.m, c.n, c.k, _ptr(ws) if need else None, need, c.accumulate, st), what)
    torch.cuda.synchronize()
    used = c.nz * c.m * c.n if (c.nz > 1 or c.accumulate) else 0
    assert bool((sbuf[used:] == SENTINEL).all()), f"{what}: a store behind the {used} workspace floats of {c.nz} slices"
    got = result2(cbuf, c.m, c.n, what)
    prev = prev if c.accumulate else None
    ref = G.wgrad_f64(a, b, prev)[0]
    report("eg_gemm_tn", G.compare_sliced(got, ref, G.wgrad_bounds(a, b, 0.0, c.nz, prev)[0], what, G.WG_AXES)[2])


def test_gemm_tn_refusals_leave_the_output_untouched():
    """A workspace one float short of eg_gemm_tn_workspace_floats, `accumulate` without a workspace -> EG_ERR_WORKSPACE; lda < m, k = 0 ->
    EG_ERR_BAD_ARG; C keeps the sentinel."""
    L, lib, _ptr, st = _api()
    m, n, k = 65, 63, 513
    a, b, _ = (t.to(dev()) for t in G.gemm_tn_inputs(m, n, k))
    need = G.gemm_tn_workspace_floats(m, n, k)
    assert need == 3 * m * n
    cbuf, cd = canary2(m, n)
    sbuf, ws = workspace(need)
    for what, rc, want in (("workspace one float short", lib.eg_gemm_tn(_ptr(a), m, _ptr(b), n, _ptr(cd), n, m, n, k, _ptr(ws), need - 1, 0, st), WORKSPACE),
                           ("accumulate without a workspace", lib.eg_gemm_tn(_ptr(a), m, _ptr(b), n, _ptr(cd), n, m, n, 32, None, 0, 1, st), WORKSPACE),
                           ("lda < m", lib.eg_gemm_tn(_ptr(a), m - 1, _ptr(b), n, _ptr(cd), n, m, n, k, _ptr(ws), need, 0, st), BAD_ARG),
                           ("k = 0", lib.eg_gemm_tn(_ptr(a), m, _ptr(b), n, _ptr(cd), n, m, n, 0, _ptr(ws), need, 0, st), BAD_ARG)):
        assert rc == want, f"{what}: status {rc}, expected {want} ({lib.eg_last_error().decode()})"
        torch.cuda.synchronize()
        assert bool((cbuf == SENTINEL).all()) and bool((sbuf == SENTINEL).all()), f"{what}: something was written"


# ---- eg_colsum --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,c,kernel,z", G.COLSUM_CASES)
def test_colsum_matches_float64_per_element(rows, c, kernel, z):
    """col_sums: col_direct_kernel (C % 4 == 0, rows <= 1024), col_partial_fast_kernel + col_finalize_kernel (C | 1024) or col_partial_kernel +
    col_finalize_kernel (any C); the route of each case is in grads_f64.COLSUM_CASES.  (sum a, sum a b) with b, (sum a, sum a^2) without, and
    each output alone; all held to the db bound."""
    L, lib, _ptr, st = _api()
    a, b = G.colsum_inputs(rows, c)
    ad, bd = a.to(dev()), b.to(dev())
    need = int(lib.eg_colreduce_workspace_floats(c))
    worst = 0.0
    for second, want0, want1 in ((bd, True, True), (None, True, True), (bd, True, False), (bd, False, True)):
        what = f"eg_colsum {rows}x{c} ({kernel}) b {second is not None} o0 {want0} o1 {want1}"
        buf0, o0 = canary1(c)
        buf1, o1 = canary1(c)
        sbuf, ws = workspace(need)
        L.check(lib.eg_colsum(_ptr(ad), _ptr(second) if second is not None else None, _ptr(o0) if want0 else None, _ptr(o1) if want1 else None,
                              rows, c, _ptr(ws), st), what)
        torch.cuda.synchronize()
        assert bool((sbuf[need:] == SENTINEL).all()), f"{what}: a store behind the workspace"
        other = b if second is not None else a
        b0, b1 = G.colsum_bounds(a, other, z)
        for buf, want, ref, bound, name in ((buf0, want0, a.double().sum(0), b0, "sum a"), (buf1, want1, (a.double() * other.double()).sum(0), b1, "sum a b")):
            if want:
                worst = max(worst, G.compare_sliced(result1(buf, c, what), ref, bound, f"{what} {name}", ("column",))[2])
            else:
                assert bool((buf == SENTINEL).all()), f"{what}: {name} written without being asked for"
    report("eg_colsum", worst)
