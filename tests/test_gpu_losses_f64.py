"""eg_smooth_l1, eg_cross_entropy (plain and focal), eg_kld and eg_reparameterize on the GPU through the C ABI, every ELEMENT against float64
(tests/train_tail_f64.py sections 2-4: references, bounds, cases).  Outputs in canary-guarded buffers, optional gradients passed as NULL,
workspaces of exactly the advertised size (1024 floats for smooth-L1, B floats for the cross entropy, whose workspace is the per-row loss)."""
import pytest
import torch

import train_tail_f64 as S
import train_tail_gpu as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", S.SL1_N)
def test_smooth_l1_matches_float64_per_element(n):
    """smooth_l1_kernel + sum_small_kernel: one block, a ragged last block, and 262147 elements (every one of the 1024 blocks strides twice);
    inputs on the 1/64 grid hold d = +-beta, d = 0 and d = -0; dpred per element, NULL and non-NULL; the loss a priori."""
    L, lib, ptr, st = D.api()
    p, t = S.sl1_inputs(n)
    pd, td = D.up(p), D.up(t)
    for beta in S.SL1_BETA:
        for scale in (1.0, 100.0):
            rl, rd = S.sl1_eval(p, t, beta, scale)
            bl, bd = S.sl1_bounds(p, t, beta, scale)
            for with_grad in (True, False):
                what = f"smooth_l1 n {n} beta {beta} scale {scale} dpred {with_grad}"
                loss, dp, ws = D.Guarded((1,)), D.Guarded((n,)), D.workspace(1024)
                L.check(lib.eg_smooth_l1(ptr(pd), ptr(td), ptr(loss.t), ptr(dp.t) if with_grad else None, n, beta, scale, ptr(ws.t), st), what)
                ws.intact(what + " workspace")
                D.frac("smooth_l1 loss", loss.intact(what + " loss")[0], rl, bl, what + " loss")
                if with_grad:
                    D.frac("smooth_l1 dpred", dp.intact(what + " dpred"), rd, bd, what + " dpred", ("element",))
                else:
                    dp.untouched(what + " dpred")
    D.report("smooth_l1 loss", "smooth_l1 dpred")


@pytest.mark.parametrize("C", S.CE_C)
@pytest.mark.parametrize("B", S.CE_B)
def test_cross_entropy_matches_float64_per_element(B, C):
    """ce_kernel: the per-row loss (the workspace), the mean loss and dlogits for plain CE (gamma = -1) and focal gamma 0, 1, 2, alpha NULL and per
    sample, on uniform logits, the label 30 above / below the rest (pt -> 1 / ~1e-13), a tie at the maximum and every logit shifted by 1e4."""
    L, lib, ptr, st = D.api()
    for cls in S.CE_CLASSES:
        z, y, a = S.ce_inputs(B, C, cls)
        zd, yd, ad = D.up(z), D.up(y), D.up(a)
        for gamma in S.CE_GAMMA:
            for alpha in ((None, a) if gamma >= 0 else (None,)):
                rr, rl, rd = S.ce_eval(z, y, alpha, gamma, 1.0)
                br, bl, bd = S.ce_bounds(z, y, alpha, gamma, 1.0)
                for with_grad in ((True, False) if cls == "uniform" else (True,)):
                    what = f"ce {B}x{C} {cls} gamma {gamma} alpha {alpha is not None} dlogits {with_grad}"
                    loss, dl, row = D.Guarded((1,)), D.Guarded((B, C)), D.workspace(B)
                    rc = lib.eg_cross_entropy(ptr(zd), ptr(yd), ptr(ad) if alpha is not None else None, gamma, 1.0, ptr(loss.t),
                                              ptr(dl.t) if with_grad else None, B, C, ptr(row.t), st)
                    L.check(rc, what)
                    D.frac("cross_entropy rowloss", row.intact(what + " rowloss"), rr, br, what + " rowloss", ("sample",))
                    D.frac("cross_entropy loss", loss.intact(what + " loss")[0], rl, bl, what + " loss")
                    if with_grad:
                        D.frac("cross_entropy dlogits", dl.intact(what + " dlogits"), rd, bd, what + " dlogits", ("sample", "class"))
                    else:
                        dl.untouched(what + " dlogits")
    D.report("cross_entropy rowloss", "cross_entropy loss", "cross_entropy dlogits")


@pytest.mark.parametrize("shape", S.KLD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kld_and_reparameterize_match_float64_per_element(shape):
    """kld_kernel (one workgroup; 7 x 1000 gives 28 elements per thread) with and without its gradients, and reparam_kernel, for log-variances in
    [-2, 1] and [-10, 10]."""
    L, lib, ptr, st = D.api()
    n, d = shape
    for lv in S.KLD_LOGVAR:
        mu, l, eps = S.kld_inputs(n, d, lv)
        md, ld, ed = D.up(mu), D.up(l), D.up(eps)
        ref, bound = S.kld_eval(mu, l, 0.5), S.kld_bounds(mu, l, 0.5)
        for with_grad in (True, False):
            what = f"kld {n}x{d} logvar {lv} grads {with_grad}"
            loss, dmu, dlv = D.Guarded((1,)), D.Guarded((n, d)), D.Guarded((n, d))
            L.check(lib.eg_kld(ptr(md), ptr(ld), ptr(loss.t), ptr(dmu.t) if with_grad else None, ptr(dlv.t) if with_grad else None, n, d, 0.5, st), what)
            D.frac("kld loss", loss.intact(what + " loss")[0], ref[0], bound[0], what + " loss")
            if with_grad:
                D.frac("kld dmu", dmu.intact(what + " dmu"), ref[1], bound[1], what + " dmu", ("sample", "dim"))
                D.frac("kld dlogvar", dlv.intact(what + " dlogvar"), ref[2], bound[2], what + " dlogvar", ("sample", "dim"))
            else:
                dmu.untouched(what + " dmu")
                dlv.untouched(what + " dlogvar")
        what = f"reparameterize {n}x{d} logvar {lv}"
        z = D.Guarded((n, d))
        L.check(lib.eg_reparameterize(ptr(md), ptr(ld), ptr(ed), ptr(z.t), n * d, st), what)
        D.frac("reparameterize", z.intact(what), S.reparam_eval(mu, l, eps), S.reparam_bound(mu, l, eps), what, ("sample", "dim"))
    D.report("kld loss", "kld dmu", "kld dlogvar", "reparameterize")
