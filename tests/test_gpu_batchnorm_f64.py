"""Train-mode BatchNorm on the GPU -- eg_bn_train_forward, eg_bn_train_backward, eg_bn_train_forward_gap, eg_bn_train_forward_sq and
eg_bn_train_stats_sq of csrc/train.hip -- called through the C ABI, every ELEMENT against float64 (tests/train_tail_f64.py: references, bounds with
their derivations, the case list with the kernel route of each case; tests/test_train_tail_f64.py shows on the CPU that correct arithmetic stays at
half of every bound and that single-site faults exceed them).  Outputs sit in canary-guarded buffers, optional outputs are passed as NULL, the
workspace is exactly eg_colreduce_workspace_floats long (tests/train_tail_gpu.py).

A defect of the forward is pinned here: with a one-step mean (sum / rows from the fp32 chains) test_two_pass_forward_matches_float64_per_element
fails on the constant 100.3 channel of the const_zero class and on the mean-100 class (save_mean 1.9 x its bound at 3712 x 34, y - beta = -7e-3 gamma
where float64 has 0), which is why bn_finalize_kernel corrects the mean with the residual sum of the centred pass."""
import pytest
import torch

import train_tail_f64 as S
import train_tail_gpu as D

pytestmark = pytest.mark.gpu

EPS = S.BN_EPS
_ID = lambda k: f"{k.rows}x{k.c}" + ("" if k.aligned else "-misaligned")


def _ws(c, off=0):
    return D.workspace(int(D.api()[1].eg_colreduce_workspace_floats(c)), off)


def _check_forward(tag, what, out, ref, bound, y=True, running=True, channels=None):
    D.frac(tag + " save_mean", out["mean"], ref["mean"], bound["mean"], what + " save_mean", ("channel",))
    D.frac(tag + " save_rstd", out["rstd"], ref["rstd"], bound["rstd"], what + " save_rstd", ("channel",), channels)
    if running:
        D.frac(tag + " running_mean", out["running_mean"], ref["running_mean"], bound["running_mean"], what + " running_mean", ("channel",))
        D.frac(tag + " running_var", out["running_var"], ref["running_var"], bound["running_var"], what + " running_var", ("channel",))
    if y:
        D.frac(tag + " y", out["y"], ref["y"], bound["y"], what + " y", S.BN_AXES, channels)


@pytest.mark.parametrize("case", S.BN_CASES, ids=_ID)
def test_two_pass_forward_matches_float64_per_element(case):
    """y, save_mean, save_rstd and the running statistics (unbiased variance; rows = 1 the biased one; momentum 0.1 and 0.37; NULL running buffers
    leave nothing written) on every input class: centred uniform, mean 100 with unit spread, columns over three decades, one constant 100.3 and one
    all-zero channel."""
    L, lib, ptr, st = D.api()
    off = 0 if case.aligned else 1
    rows, c = case.rows, case.c
    plan = S.bn_plan(rows, c, case.aligned)
    assert plan.route == case.fwd and S.apply_route(c, case.aligned) == case.apply
    for cls in S.BN_CLASSES:
        for mom, running in (((0.1, True), (0.37, True), (0.1, False)) if cls == "uniform" else ((0.1, True),)):
            x, g, b, dy, rm, rv = S.bn_inputs(rows, c, cls)
            ref, bound = S.bn_forward_bounds(x, g, b, rm, rv, mom, plan)
            what = f"bn forward {rows}x{c} {cls} mom {mom} ({case.fwd}, {case.apply})"
            y, sm, sr = D.Guarded((rows, c), off), D.Guarded((c,), off), D.Guarded((c,), off)
            grm, grv = D.Guarded((c,), off, rm), D.Guarded((c,), off, rv)
            ws = _ws(c, off)
            xd, gd, bd = D.up(x, off), D.up(g, off), D.up(b, off)           # (named: a temporary would be freed and its block handed to the next upload)
            rc = lib.eg_bn_train_forward(ptr(xd), ptr(gd), ptr(bd), ptr(y.t), ptr(sm.t), ptr(sr.t),
                                         ptr(grm.t) if running else None, ptr(grv.t) if running else None, rows, c, mom, EPS, ptr(ws.t), st)
            L.check(rc, what)
            ws.intact(what + " workspace")
            out = {"y": y.intact(what + " y"), "mean": sm.intact(what + " save_mean"), "rstd": sr.intact(what + " save_rstd"),
                   "running_mean": grm.intact(what + " running_mean"), "running_var": grv.intact(what + " running_var")}
            if not running:
                assert torch.equal(out["running_mean"], rm) and torch.equal(out["running_var"], rv)
            _check_forward("bn_forward", what, out, ref, bound, running=running)
            if cls == "const_zero":
                assert torch.equal(out["y"][:, c - 1], b[c - 1].expand(rows)), what + ": the all-zero channel is beta exactly"
    D.report("bn_forward save_mean", "bn_forward save_rstd", "bn_forward running_mean", "bn_forward running_var", "bn_forward y")


@pytest.mark.parametrize("case", S.BN_CASES, ids=_ID)
def test_backward_matches_float64_per_element(case):
    """dx within 4 x torch's float32 CPU backward error (BN_DX_CPU_F32, per input class, in units of |gamma| rstd rms(dy)), dgamma and dbeta within
    their a-priori bounds, on the fp32 save_mean / save_rstd the kernel is given; with relu_mask = 1, dx is +0 bitwise wherever x <= 0."""
    L, lib, ptr, st = D.api()
    off = 0 if case.aligned else 1
    rows, c = case.rows, case.c
    plan = S.bwd_plan(rows, c, case.aligned)
    assert plan.route == case.bwd
    for cls in S.BN_CLASSES:
        x, g, b, dy, rm, rv = S.bn_inputs(rows, c, cls)
        fwd = S.bn_forward_f64(x, g, b, rm, rv, 0.1)
        m32, r32 = fwd["mean"].float(), fwd["rstd"].float()
        ref, bound = S.bn_backward_bounds(x, dy, g, m32, r32, plan)
        tol = S.bn_dx_tol(cls) * S.bn_dx_unit(dy, g, r32)
        xd, dyd, gd, md, rd = D.up(x, off), D.up(dy, off), D.up(g, off), D.up(m32, off), D.up(r32, off)
        for relu in (0, 1):
            what = f"bn backward {rows}x{c} {cls} relu_mask {relu} ({case.bwd})"
            dx, dg, db = D.Guarded((rows, c), off), D.Guarded((c,), off), D.Guarded((c,), off)
            ws = _ws(c, off)
            rc = lib.eg_bn_train_backward(ptr(xd), ptr(dyd), ptr(gd), ptr(md), ptr(rd), ptr(dx.t), ptr(dg.t), ptr(db.t), rows, c, relu, ptr(ws.t), st)
            L.check(rc, what)
            ws.intact(what + " workspace")
            got = dx.intact(what + " dx")
            want = ref["dx"]
            if relu:
                dead = x <= 0
                assert bool((got.view(torch.int32)[dead] == 0).all()), what + ": dx is not +0 where x <= 0"
                want = torch.where(dead, torch.zeros_like(want), want)
            D.frac("bn_backward dx", got, want, tol, what + " dx", S.BN_AXES)
            D.frac("bn_backward dgamma", dg.intact(what + " dgamma"), ref["dgamma"], bound["dgamma"], what + " dgamma", ("channel",))
            D.frac("bn_backward dbeta", db.intact(what + " dbeta"), ref["dbeta"], bound["dbeta"], what + " dbeta", ("channel",))
    D.report("bn_backward dx", "bn_backward dgamma", "bn_backward dbeta")


@pytest.mark.parametrize("case", S.gap_cases(), ids=lambda k: "x".join(map(str, k)))
def test_partial_fed_entry_points_match_float64_per_element(case):
    """eg_bn_train_forward_gap (clip_sum_from_gap, bn_mean_from_clips, the shared centred pass: the bounds of the two-pass forward),
    eg_bn_train_forward_sq and eg_bn_train_stats_sq (clip_sums_sq, bn_finalize_sq: held to the conditioning of E[x^2] - mean^2 on per-tile sums
    rounded once to fp32) fed with per-tile sums the test makes in float64.  rstd of the _sq routes is also held in the variance domain, which is the
    only check where mean^2 / var exhausts fp32 (the constant channel)."""
    L, lib, ptr, st = D.api()
    batch, tiles, c = case
    for cls in ("uniform", "offset", "const_zero"):
        x, g, b, rm, rv, gap, gap_sq = S.gap_inputs(batch, tiles, c, cls)
        rows = x.shape[0]
        xd, gd, bd, gapd, sqd = D.up(x), D.up(g), D.up(b), D.up(gap), D.up(gap_sq)
        ref, bound = S.bn_forward_bounds(x, g, b, rm, rv, 0.1, S.bn_plan(rows, c))
        for with_y, with_clip in ((True, True), (False, False)):
            what = f"bn forward_gap {case} {cls} y {with_y} clip_sum {with_clip}"
            y, sm, sr, cs = D.Guarded((rows, c)), D.Guarded((c,)), D.Guarded((c,)), D.Guarded((batch, c))
            grm, grv, ws = D.Guarded((c,), 0, rm), D.Guarded((c,), 0, rv), _ws(c)
            rc = lib.eg_bn_train_forward_gap(ptr(xd), ptr(gapd), tiles, batch, ptr(gd), ptr(bd), ptr(y.t) if with_y else None, ptr(sm.t), ptr(sr.t),
                                             ptr(cs.t) if with_clip else None, ptr(grm.t), ptr(grv.t), rows, c, 0.1, EPS, ptr(ws.t), st)
            L.check(rc, what)
            ws.intact(what + " workspace")
            out = {"mean": sm.intact(what), "rstd": sr.intact(what), "running_mean": grm.intact(what), "running_var": grv.intact(what)}
            if with_y:
                out["y"] = y.intact(what + " y")
                D.frac("bn_gap clip_sum", cs.intact(what + " clip_sum"), gap.double().sum(1), S.clip_sum_bound(gap), what + " clip_sum", ("clip", "channel"))
            else:
                y.untouched(what + " y")
                cs.untouched(what + " clip_sum")
            _check_forward("bn_gap", what, out, ref, bound, y=with_y)
        ref, bound = S.bn_sq_bounds(x, g, b, rm, rv, 0.1, gap, gap_sq)
        lin = torch.isfinite(bound["rstd"])
        what = f"bn forward_sq {case} {cls}"
        y, sm, sr, cs = D.Guarded((rows, c)), D.Guarded((c,)), D.Guarded((c,)), D.Guarded((batch, c))
        grm, grv, ws = D.Guarded((c,), 0, rm), D.Guarded((c,), 0, rv), _ws(c)
        rc = lib.eg_bn_train_forward_sq(ptr(xd), ptr(gapd), ptr(sqd), tiles, batch, ptr(gd), ptr(bd), ptr(y.t), ptr(sm.t), ptr(sr.t), ptr(cs.t),
                                        ptr(grm.t), ptr(grv.t), rows, c, 0.1, EPS, ptr(ws.t), st)
        L.check(rc, what)
        ws.intact(what + " workspace")
        out = {"y": y.intact(what), "mean": sm.intact(what), "rstd": sr.intact(what), "running_mean": grm.intact(what), "running_var": grv.intact(what)}
        _check_forward("bn_sq", what, out, ref, bound, channels=lin)
        D.frac("bn_sq rstd as variance", S.sq_var_of(out["rstd"]), ref["var"], bound["var"], what + " rstd in the variance domain", ("channel",))
        D.frac("bn_gap clip_sum", cs.intact(what + " clip_sum"), gap.double().sum(1), S.clip_sum_bound(gap), what + " clip_sum", ("clip", "channel"))
        what = f"bn stats_sq {case} {cls}"
        sm2, sr2, asc, ash = D.Guarded((c,)), D.Guarded((c,)), D.Guarded((c,)), D.Guarded((c,))
        ws = _ws(c)
        rc = lib.eg_bn_train_stats_sq(ptr(gapd), ptr(sqd), tiles, batch, ptr(gd), ptr(bd), ptr(sm2.t), ptr(sr2.t), None, None, ptr(asc.t), ptr(ash.t),
                                      rows, c, 0.1, EPS, ptr(ws.t), st)
        L.check(rc, what)
        ws.intact(what + " workspace")
        assert torch.equal(sm2.intact(what), out["mean"]) and torch.equal(sr2.intact(what), out["rstd"]), what + ": statistics differ from forward_sq"
        scale = g.double() * ref["rstd"]
        D.frac("bn_stats_sq aff_scale", asc.intact(what), scale, bound["aff_scale"], what + " aff_scale", ("channel",), lin)
        D.frac("bn_stats_sq aff_shift", ash.intact(what), b.double() - ref["mean"] * scale, bound["aff_shift"], what + " aff_shift", ("channel",), lin)
    D.report("bn_gap save_mean", "bn_gap save_rstd", "bn_gap running_mean", "bn_gap running_var", "bn_gap y", "bn_gap clip_sum", "bn_sq save_mean",
             "bn_sq save_rstd", "bn_sq rstd as variance", "bn_sq running_mean", "bn_sq running_var", "bn_sq y", "bn_stats_sq aff_scale",
             "bn_stats_sq aff_shift")


def test_partial_fed_refusals_launch_nothing():
    """C = 48 (no divisor of 256) is EG_ERR_UNSUPPORTED at all three entry points, batch = 513 without a clip_sum buffer at forward_gap; every
    output keeps its canary."""
    L, lib, ptr, st = D.api()
    for c, batch, clip in ((48, 2, True), (4, 513, False)):
        rows = batch
        x, g, b = D.up(torch.ones(rows, c)), D.up(torch.ones(c)), D.up(torch.zeros(c))
        gap = D.up(torch.ones(batch, 1, c))
        outs = [D.Guarded((rows, c)), D.Guarded((c,)), D.Guarded((c,)), D.Guarded((batch, c)), D.Guarded((c,)), D.Guarded((c,))]
        y, sm, sr, cs, a0, a1 = outs
        ws = _ws(c)
        rc = lib.eg_bn_train_forward_gap(ptr(x), ptr(gap), 1, batch, ptr(g), ptr(b), ptr(y.t), ptr(sm.t), ptr(sr.t), ptr(cs.t) if clip else None, None, None,
                                         rows, c, 0.1, EPS, ptr(ws.t), st)
        assert rc == D.UNSUPPORTED and lib.eg_last_error(), (c, batch, rc)
        if c == 48:
            rc = lib.eg_bn_train_forward_sq(ptr(x), ptr(gap), ptr(gap), 1, batch, ptr(g), ptr(b), ptr(y.t), ptr(sm.t), ptr(sr.t), ptr(cs.t), None, None,
                                            rows, c, 0.1, EPS, ptr(ws.t), st)
            assert rc == D.UNSUPPORTED
            rc = lib.eg_bn_train_stats_sq(ptr(gap), ptr(gap), 1, batch, ptr(g), ptr(b), ptr(sm.t), ptr(sr.t), None, None, ptr(a0.t), ptr(a1.t), rows, c,
                                          0.1, EPS, ptr(ws.t), st)
            assert rc == D.UNSUPPORTED
        for o in outs + [ws]:
            o.untouched(f"refused C = {c}, batch = {batch}")
