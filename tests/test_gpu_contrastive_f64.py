"""The five contrastive-loss kernels of csrc/misc.hip on the GPU through eg_contrastive_loss and eg_contrastive_loss_backward, every ELEMENT against
float64 (tests/misc_f64.py section 2: reference, bounds, cases, input classes).  cross is passed once as NULL and once as a canary-guarded buffer;
the row losses and hits are read from the workspace, which has exactly the advertised size; the gradients are held to 4 x the error of torch's own
float32 CPU autograd plus the rounding of their terms."""
import functools

import numpy as np
import pytest
import torch

import misc_f64 as M
import misc_gpu as G
import train_tail_gpu as D

pytestmark = pytest.mark.gpu
_ID = lambda c: f"{c.n}x{c.d}"


@functools.lru_cache(maxsize=4)
def _case(n, d, cls):
    face, audio = M.con_inputs(n, d, cls)
    return (face, audio) + M.con_bounds(face, audio)


@pytest.mark.parametrize("case", M.CON_CASES, ids=_ID)
def test_contrastive_forward_matches_float64_per_element(case):
    """cross, the row losses, loss and acc on every input class.  A vacuous element (a face row bit-identical to its audio row: D = 0 in float64) is
    held one-sidedly, its row to a hit and a row loss of at most 8 u; the hit of every decided row is exact -- among them the tied maxima, 256
    columns apart in one thread and in neighbouring threads, where the lower index wins; with every row decided acc is exact."""
    L, lib, ptr, st = D.api()
    n, d = case.n, case.d
    for cls in M.con_classes_for(case):
        face, audio, ref, bound = _case(n, d, cls)
        fd, ad = G.up_nan(face), G.up_nan(audio)
        what = f"contrastive {n}x{d} {cls}"
        outs = []
        for with_cross in (True, False):
            cross, loss, acc, ws = D.Guarded((n, n)), D.Guarded((1,)), D.Guarded((1,)), D.workspace(2 * n)
            assert lib.eg_contrastive_workspace_bytes(n) == 8 * n
            L.check(lib.eg_contrastive_loss(ptr(fd), ptr(ad), n, d, ptr(cross.t) if with_cross else None, ptr(loss.t), ptr(acc.t), ptr(ws.t), 8 * n, st), what)
            w = ws.intact(what + " workspace")
            outs.append((loss.intact(what + " loss"), acc.intact(what + " acc"), w))
            if not with_cross:
                cross.untouched(what + " cross NULL")
                continue
            got = cross.intact(what + " cross")
            vac = bound["vacuous"]
            D.frac("contrastive cross", torch.where(vac, ref["cross"], got.double()), ref["cross"], torch.where(vac, torch.zeros_like(ref["cross"]), bound["cross"]),
                   what + " cross", ("face row", "audio row"))
            assert bool((got.double()[vac] >= bound["cross_floor"][vac]).all()), what + ": a vacuous element is below 1 / (D + E_D + 1e-8)"
        (l0, a0, w0), (l1, a1, w1) = outs
        assert torch.equal(G.bits(l0), G.bits(l1)) and torch.equal(G.bits(a0), G.bits(a1)) and torch.equal(G.bits(w0), G.bits(w1)), what + ": cross NULL changes the result"
        rowloss, hit = w0[:n], G.bits(w0[n:2 * n]).bool()
        rows = bound["row_kind"] != 2
        assert bool(torch.isfinite(rowloss).all()) and bool(torch.isfinite(l0).all()), what + ": non-finite loss"
        D.frac("contrastive rowloss", rowloss[rows], ref["rowloss"][rows], bound["rowloss"][rows], what + " rowloss", ("row",))
        if bound["loss"] != float("inf"):
            D.frac("contrastive loss", l0[0], ref["loss"], torch.tensor(bound["loss"]), what + " loss")
        dec = bound["decided"]
        assert torch.equal(hit[dec], ref["hit"][dec]), what + f": hits of decided rows differ at {(hit != ref['hit'])[dec].nonzero().flatten().tolist()}"
        assert float(a0[0]) == float(np.float32(int(hit.sum())) / np.float32(n)), what + ": acc is not hits / n"
        if bool(dec.all()):
            assert float(a0[0]) == float(np.float32(int(ref["hit"].sum())) / np.float32(n)), what + ": acc"
    D.report("contrastive cross", "contrastive rowloss", "contrastive loss")


@pytest.mark.parametrize("case", M.CON_GRAD_CASES, ids=_ID)
def test_contrastive_backward_matches_float64_per_element(case):
    """gface and gaudio on every input class against the closed form in float64 (which tests/test_misc_f64.py shows to be torch's autograd).  The
    all-zero face row takes the 1e12 of F.normalize's clamp; W_ii of the bit-identical pair, read from the workspace, is exactly 0; the near class,
    whose float64 gradients are below 1e-36, must be finite and below 1e-30."""
    L, lib, ptr, st = D.api()
    n, d = case.n, case.d
    for cls in M.con_classes_for(case):
        face, audio = M.con_inputs(n, d, cls)
        what = f"contrastive backward {n}x{d} {cls}"
        floats = n * n + 2 * n
        assert lib.eg_contrastive_backward_workspace_bytes(n) == 4 * floats
        gf, ga, ws = D.Guarded((n, d)), D.Guarded((n, d)), D.workspace(floats)
        fd, ad = G.up_nan(face), G.up_nan(audio)
        L.check(lib.eg_contrastive_loss_backward(ptr(fd), ptr(ad), n, d, ptr(gf.t), ptr(ga.t), ptr(ws.t), 4 * floats, st), what)
        W = ws.intact(what + " workspace")[:n * n].view(n, n)
        gotf, gota = gf.intact(what + " gface"), ga.intact(what + " gaudio")
        if cls == "near":
            assert bool(torch.isfinite(gotf).all()) and bool(torch.isfinite(gota).all()), what
            assert float(gotf.abs().max()) <= M.CON_GRAD_NEAR_ABS and float(gota.abs().max()) <= M.CON_GRAD_NEAR_ABS, what
            continue
        ref = M.con_grads(face, audio)
        tf, ta = M.con_grad_tols(ref, cls)
        D.frac("contrastive gface", gotf, ref["gface"], tf, what + " gface", ("row", "dim"))
        D.frac("contrastive gaudio", gota, ref["gaudio"], ta, what + " gaudio", ("row", "dim"))
        if cls == "identical":
            assert float(W[n - 1, n - 1]) == 0.0, what + ": a gradient through D = 0"
        if cls == "zero_row":
            assert float(ref["finv"][n // 2]) == 1e12
    D.report("contrastive gface", "contrastive gaudio")
