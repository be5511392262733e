"""CPU checks of tests/train_tail_f64.py.  (1) The per-element bounds the GPU tests of BatchNorm, the losses, the gates, Adam and the segment
operators use are not violated by correct arithmetic: the emulated fp32 data flow, in two summation orders, stays at or under half of them at EVERY
case.  (2) They are not vacuous: each single-site fault, switched on, exceeds its bound.  (3) Every case takes the kernel route its comment states,
by the restated planners.  (4) The recorded error of torch's float32 CPU batch-norm backward, which the dx tolerance is 4 x of, is re-measured and
must not be stale by more than 2 x.  (5) The restatement of f32_to_bf16_rne is torch's cast on every finite pattern, keeps NaN, and without its NaN
case reproduces the three wrong patterns of the defect."""
import numpy as np
import pytest
import torch

import train_tail_f64 as S

WORST = {}
HALF = 0.5
F32 = torch.float32


def _half(name, got, ref, bound, what):
    el = S.worst(got, ref, bound)
    assert el <= HALF, f"{what}: correct arithmetic reaches {el:.3f} of the bound ({name})"
    WORST[name] = max(WORST.get(name, 0.0), el)


def _report(*names):
    print("; ".join(f"{n} {WORST[n]:.3f}" for n in names), "(worst element of correct arithmetic as a fraction of the bound)")
    for n in names:
        assert WORST[n] <= S.WORST_OF_CORRECT_ARITHMETIC[n], f"{n}: {WORST[n]:.3f} against the recorded {S.WORST_OF_CORRECT_ARITHMETIC[n]}"


def _bn_case_outputs(case, cls, mom):
    x, g, b, dy, rm, rv = S.bn_inputs(case.rows, case.c, cls)
    plan = S.bn_plan(case.rows, case.c, case.aligned)
    ref, bound = S.bn_forward_bounds(x, g, b, rm, rv, mom, plan)
    return (x, g, b, dy, rm, rv), plan, ref, bound


FWD_KEYS = ("mean", "rstd", "running_mean", "running_var", "y")


# ---- 1. correct arithmetic stays inside half the bounds -------------------------------------------------------------------------------------
def test_batchnorm_emulation_is_within_half_the_bound_at_every_case():
    for case in S.BN_CASES:
        for cls in S.BN_CLASSES:
            for mom in ((0.1, 0.37) if cls == "uniform" else (0.1,)):
                (x, g, b, dy, rm, rv), plan, ref, bound = _bn_case_outputs(case, cls, mom)
                for order in ("forward", "reversed"):
                    out = S.emulate_bn_forward(x, g, b, rm, rv, mom, plan, order)
                    for k in FWD_KEYS:
                        _half("bn " + k, out[k], ref[k], bound[k], f"bn {case.rows}x{case.c} {cls} mom {mom} {order} {k}")
            m32, r32 = ref["mean"].float(), ref["rstd"].float()
            bp = S.bwd_plan(case.rows, case.c, case.aligned)
            bref, bb = S.bn_backward_bounds(x, dy, g, m32, r32, bp)
            unit = S.bn_dx_unit(dy, g, r32)
            for order in ("forward", "reversed"):
                out = S.emulate_bn_backward(x, dy, g, m32, r32, bp, order)
                what = f"bn backward {case.rows}x{case.c} {cls} {order}"
                _half("bn dbeta", out["dbeta"], bref["dbeta"], bb["dbeta"], what + " dbeta")
                _half("bn dgamma", out["dgamma"], bref["dgamma"], bb["dgamma"], what + " dgamma")
                _half("bn dx", out["dx"], bref["dx"], S.bn_dx_tol(cls) * unit, what + " dx")
    _report(*("bn " + k for k in FWD_KEYS), "bn dbeta", "bn dgamma", "bn dx")


def test_partial_fed_batchnorm_emulations_are_within_half_the_bound_at_every_case():
    for batch, tiles, c in S.gap_cases():
        for cls in ("uniform", "offset", "const_zero"):
            x, g, b, rm, rv, gap, gap_sq = S.gap_inputs(batch, tiles, c, cls)
            rows = x.shape[0]
            plan = S.bn_plan(rows, c)
            ref, bound = S.bn_forward_bounds(x, g, b, rm, rv, 0.1, plan)
            m0 = (gap.double().sum((0, 1)) / rows).float().numpy()
            what = f"bn_gap {batch}x{tiles}x{c} {cls}"
            for order in ("forward", "reversed"):
                out = S.emulate_bn_forward(x, g, b, rm, rv, 0.1, plan, order, m0=m0)
                _half("bn_gap mean", out["mean"], ref["mean"], bound["mean"], what + " mean")
                _half("bn_gap rstd", out["rstd"], ref["rstd"], bound["rstd"], what + " rstd")
                _half("bn y", out["y"], ref["y"], bound["y"], what + " y")
            ref, bound = S.bn_sq_bounds(x, g, b, rm, rv, 0.1, gap, gap_sq)
            out = S.emulate_bn_sq(x, g, b, rm, rv, 0.1, gap, gap_sq)
            what = f"bn_sq {batch}x{tiles}x{c} {cls}"
            _half("bn_sq mean", out["mean"], ref["mean"], bound["mean"], what + " mean")
            _half("bn_sq rstd", out["rstd"], ref["rstd"], bound["rstd"], what + " rstd")
            _half("bn_sq var", S.sq_var_of(out["rstd"]), ref["var"], bound["var"], what + " rstd in the variance domain")
            for k in ("running_mean", "running_var", "y"):
                _half("bn_sq " + k, out[k], ref[k], bound[k], what + " " + k)
            scale = g.double() * ref["rstd"]
            _half("bn_sq aff", out["aff_scale"], scale, bound["aff_scale"], what + " aff_scale")
            _half("bn_sq aff", out["aff_shift"], b.double() - ref["mean"] * scale, bound["aff_shift"], what + " aff_shift")
    _report("bn_gap mean", "bn_gap rstd", "bn_sq mean", "bn_sq rstd", "bn_sq var", "bn_sq running_mean", "bn_sq running_var", "bn_sq y", "bn_sq aff")


def test_loss_emulations_are_within_half_the_bound_at_every_case():
    for n in S.SL1_N:
        p, t = S.sl1_inputs(n)
        for beta in S.SL1_BETA:
            for scale in (1.0, 100.0):
                rl, rd = S.sl1_eval(p, t, beta, scale)
                bl, bd = S.sl1_bounds(p, t, beta, scale)
                for flip in (False, True):
                    l, d = S.sl1_eval(p, t, beta, scale, F32, flip)
                    _half("smooth_l1 loss", l, rl, bl, f"smooth_l1 {n} beta {beta} loss")
                    _half("smooth_l1 dpred", d, rd, bd, f"smooth_l1 {n} beta {beta} dpred")
    for B in S.CE_B:
        for C in S.CE_C:
            for cls in S.CE_CLASSES:
                z, y, a = S.ce_inputs(B, C, cls)
                for gamma in S.CE_GAMMA:
                    for alpha in ((None, a) if gamma >= 0 else (None,)):
                        rr, rl, rd = S.ce_eval(z, y, alpha, gamma, 1.0)
                        br, bl, bd = S.ce_bounds(z, y, alpha, gamma, 1.0)
                        for flip in (False, True):
                            r, l, d = S.ce_eval(z, y, alpha, gamma, 1.0, F32, flip)
                            what = f"ce {B}x{C} {cls} gamma {gamma} alpha {alpha is not None}"
                            _half("ce rowloss", r, rr, br, what + " rowloss")
                            _half("ce loss", l, rl, bl, what + " loss")
                            _half("ce dlogits", d, rd, bd, what + " dlogits")
    for n, d in S.KLD_SHAPES:
        for lv in S.KLD_LOGVAR:
            mu, l, eps = S.kld_inputs(n, d, lv)
            ref, bound = S.kld_eval(mu, l, 0.5), S.kld_bounds(mu, l, 0.5)
            for flip in (False, True):
                out = S.kld_eval(mu, l, 0.5, F32, flip)
                _half("kld loss", out[0], ref[0], bound[0], f"kld {n}x{d} loss")
                _half("kld grads", out[1], ref[1], bound[1], f"kld {n}x{d} dmu")
                _half("kld grads", out[2], ref[2], bound[2], f"kld {n}x{d} dlogvar")
            _half("reparam", S.reparam_eval(mu, l, eps, F32), S.reparam_eval(mu, l, eps), S.reparam_bound(mu, l, eps), f"reparam {n}x{d}")
    _report("smooth_l1 loss", "smooth_l1 dpred", "ce rowloss", "ce loss", "ce dlogits", "kld loss", "kld grads", "reparam")


def test_gate_emulations_are_within_half_the_bound_at_every_case():
    for shape in S.GATE_SHAPES:
        B, P, D, chunk = shape
        for sat in (False, True):
            m, p, g, _ = S.gate_inputs(B, P, D, chunk, sat)
            (ro, rs), (bo, bs) = S.sp_eval(m, p, chunk), S.sp_bounds(m, p, chunk)
            gate32 = rs.float()
            (rdp, rdm), (bdp, bdm) = S.sp_bwd_eval(m, p, gate32, g, chunk), S.sp_bwd_bounds(m, p, gate32, g, chunk)
            for flip in (False, True):
                o, s = S.sp_eval(m, p, chunk, F32, flip)
                assert bool(torch.isfinite(o).all())
                _half("sp out", o, ro, bo, f"sp {shape} sat {sat} out")
                _half("sp gate", s, rs, bs, f"sp {shape} sat {sat} gate")
                dp, dm = S.sp_bwd_eval(m, p, gate32, g, chunk, F32, flip)
                _half("sp dp", dp, rdp, bdp, f"sp {shape} sat {sat} dp")
                _half("sp dm", dm, rdm, bdm, f"sp {shape} sat {sat} dm")
            if sat and chunk:
                assert set(gate32.unique().tolist()) <= {0.0, 1.0}, "the saturated class must round the gate to exactly 0 or 1"
    for shape in S.TM_SHAPES:
        B, P, D, chunk = shape
        m, p, g, score = S.gate_inputs(B, P, D, chunk)
        (ro, rw), (bo, bw) = S.tm_eval(score, p, chunk), S.tm_bounds(score, p, chunk)
        w32 = rw.float()
        (rdp, rds), (bdp, bds) = S.tm_bwd_eval(w32, p, g, chunk), S.tm_bwd_bounds(w32, p, g, chunk)
        for flip in (False, True):
            o, w = S.tm_eval(score, p, chunk, F32, flip)
            _half("tm out", o, ro, bo, f"tm {shape} out")
            _half("tm w", w, rw, bw, f"tm {shape} w")
            dp, ds = S.tm_bwd_eval(w32, p, g, chunk, F32, flip)
            _half("tm dp", dp, rdp, bdp, f"tm {shape} dp")
            _half("tm dscore", ds, rds, bds, f"tm {shape} dscore")
            assert bool((ds.double().sum(1).abs() <= bds.sum(1) + (rds.sum(1)).abs()).all())
    _report("sp out", "sp gate", "sp dp", "sp dm", "tm out", "tm w", "tm dp", "tm dscore")


def test_adam_and_segment_emulations_are_within_half_the_bound_at_every_case():
    for n in S.ADAM_N:
        for cls in S.ADAM_CLASSES:
            p, g, m, v = S.adam_inputs(n, cls)
            for t in S.ADAM_T:
                for wd in ((0.0,) if cls == "zero" else S.ADAM_WD):
                    ref, bound = S.adam_eval(p, g, m, v, t, wd), S.adam_bounds(p, g, m, v, t, wd)
                    out = S.adam_eval(p, g, m, v, t, wd, F32)
                    for k, r, o, bd in zip("pmv", ref, out, bound):
                        _half("adam " + k, o, r, bd, f"adam {n} {cls} t {t} wd {wd} {k}")
                    if cls == "zero":
                        assert torch.equal(out[0], p)
    for case in S.SEG_CASES:
        x, dy, gate, add = S.seg_inputs(case)
        ref, bound = S.seg_eval(x, dy, gate, add, 1.0 / case.hw), S.seg_bounds(x, dy, gate, add, 1.0 / case.hw, S.seg_plan(case))
        for flip in (False, True):
            out = S.seg_eval(x, dy, gate, add, 1.0 / case.hw, F32, flip)
            for name, o, r, bd in zip(("seg_mean", "seg_dot", "se_scale", "se_scale"), out, ref, bound):
                _half(name, o, r, bd, f"{name} {tuple(case[:3])}")
    _report("adam p", "adam m", "adam v", "seg_mean", "seg_dot", "se_scale")


# ---- 2. single-site faults exceed the bounds ---------------------------------------------------------------------------------------------
def _bn_fault(case, cls, fault, key):
    (x, g, b, dy, rm, rv), plan, ref, bound = _bn_case_outputs(case, cls, 0.1)
    out = S.emulate_bn_forward(x, g, b, rm, rv, 0.1, plan, "forward", fault)
    return S.worst(out[key], ref[key], bound[key])


def _case(rows, c):
    return next(k for k in S.BN_CASES if (k.rows, k.c) == (rows, c))


def test_fault_batchnorm_last_row_chunk_dropped():
    for rows, c in ((129, 34), (520, 64), (3712, 34)):
        assert _bn_fault(_case(rows, c), "uniform", "drop_last_chunk", "mean") > 1.0
        assert _bn_fault(_case(rows, c), "uniform", "drop_last_chunk", "y") > 1.0
    case = _case(1025, 60)
    x, g, b, dy, rm, rv = S.bn_inputs(case.rows, case.c, "uniform")
    ref = S.bn_forward_f64(x, g, b, rm, rv, 0.1)
    bp = S.bwd_plan(case.rows, case.c)
    bref, bb = S.bn_backward_bounds(x, dy, g, ref["mean"].float(), ref["rstd"].float(), bp)
    out = S.emulate_bn_backward(x, dy, g, ref["mean"].float(), ref["rstd"].float(), bp, "forward", "drop_last_chunk")
    assert S.worst(out["dbeta"], bref["dbeta"], bb["dbeta"]) > 1.0 and S.worst(out["dgamma"], bref["dgamma"], bb["dgamma"]) > 1.0
    assert S.worst(out["dx"], bref["dx"], S.bn_dx_tol("uniform") * S.bn_dx_unit(dy, g, ref["rstd"].float())) > 1.0


def test_fault_batchnorm_65th_column_taken_from_column_1():
    for cls in S.BN_CLASSES:
        assert _bn_fault(_case(127, 130), cls, "col64_from_col0", "y") > 1.0


def test_fault_batchnorm_biased_variance_written_to_running_var():
    for rows, c in ((2, 60), (129, 34), (3712, 34), (1024, 4)):
        assert _bn_fault(_case(rows, c), "uniform", "biased_running_var", "running_var") > 1.0
    assert _bn_fault(_case(1, 34), "uniform", "biased_running_var", "running_var") <= HALF          # rows = 1 IS the biased variance


def test_fault_batchnorm_one_step_mean_misses_a_constant_channel():
    """The arithmetic before the two-step mean: the constant 100.3 channel of the 3712-row generic case comes out ~4 ulp off, y - beta ~ 7e-3 gamma."""
    case = _case(3712, 34)
    assert _bn_fault(case, "const_zero", "one_step_mean", "mean") > 1.0
    assert _bn_fault(case, "const_zero", "one_step_mean", "y") > 1.0
    (x, g, b, dy, rm, rv), plan, ref, bound = _bn_case_outputs(case, "const_zero", 0.1)
    out = S.emulate_bn_forward(x, g, b, rm, rv, 0.1, plan)
    assert torch.equal(out["y"][:, 17], b[17].expand(3712)) and float(out["mean"][17]) == S.f32(100.3)


def test_fault_smooth_l1_threshold_and_the_value_neutral_branch():
    for n in (255, 257):
        p, t = S.sl1_inputs(n)
        rl, rd = S.sl1_eval(p, t, 0.25, 1.0)
        bl, bd = S.sl1_bounds(p, t, 0.25, 1.0)
        l, d = S.sl1_eval(p, t, 0.25, 1.0, F32, fault="beta_ignored")
        assert S.worst(l, rl, bl) > 1.0 and S.worst(d, rd, bd) > 1.0


def test_smooth_l1_branch_at_beta_is_value_neutral():
    """|d| = beta: 0.5 d^2 / beta = |d| - 0.5 beta = 0.5 beta and d / beta = sign(d): `<` and `<=` give the same bits, so the choice of branch there
    is not observable (the issue's `<=` fault cannot exceed any bound); the grid inputs do contain such elements."""
    for beta in S.SL1_BETA:
        p, t = S.sl1_inputs(257)
        assert int(((p - t).abs() == beta).sum()) >= 2
        for dt in (F32, torch.float64):
            a, b = S.sl1_eval(p, t, beta, 1.0, dt), S.sl1_eval(p, t, beta, 1.0, dt, fault="branch_le")
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fault_softmax_without_max_subtraction():
    z, y, a = S.ce_inputs(6, 65, "shifted")
    rr, rl, rd = S.ce_eval(z, y, None, -1.0, 1.0)
    br, bl, bd = S.ce_bounds(z, y, None, -1.0, 1.0)
    r, l, d = S.ce_eval(z, y, None, -1.0, 1.0, F32, fault="no_max")
    assert S.worst(r, rr, br) > 1.0 and S.worst(d, rd, bd) > 1.0
    m, p, g, score = S.gate_inputs(2, 64, 4, 64)
    (ro, rw), (bo, bw) = S.tm_eval(score + 60.0, p, 64), S.tm_bounds(score + 60.0, p, 64)
    o, w = S.tm_eval(score + 60.0, p, 64, F32, fault="no_max")
    assert S.worst(w, rw, bw) > 1.0 and S.worst(o, ro, bo) > 1.0


def test_fault_spatial_gate_dm_missing_its_last_frame():
    for shape in ((2, 5, 126, 3), (3, 8, 64, 8), (2, 34, 282, 17)):
        B, P, D, chunk = shape
        m, p, g, _ = S.gate_inputs(B, P, D, chunk)
        gate32 = S.sp_eval(m, p, chunk)[1].float()
        (rdp, rdm), (bdp, bdm) = S.sp_bwd_eval(m, p, gate32, g, chunk), S.sp_bwd_bounds(m, p, gate32, g, chunk)
        dp, dm = S.sp_bwd_eval(m, p, gate32, g, chunk, F32, fault="dm_last_frame")
        assert S.worst(dm, rdm, bdm) > 1.0 and S.worst(dp, rdp, bdp) <= HALF


def test_fault_adam_bias_correction_and_float4_head():
    p, g, m, v = S.adam_inputs(1027, "decades")
    for t in (1, 2, 1000):
        ref, bound = S.adam_eval(p, g, m, v, t, 0.0), S.adam_bounds(p, g, m, v, t, 0.0)
        out = S.adam_eval(p, g, m, v, t, 0.0, F32, fault="no_bc2")
        assert S.worst(out[0], ref[0], bound[0]) > 1.0, t
    ref, bound = S.adam_eval(p, g, m, v, 2, 0.0), S.adam_bounds(p, g, m, v, 2, 0.0)
    for phase in (1, 2, 3):
        plan = S.adam_plan(1027, phase)
        out = [o.clone() for o in S.adam_eval(p, g, m, v, 2, 0.0, F32)]
        for o, old in zip(out, (p, m, v)):
            o[plan.head] = old[plan.head]               # the first element of the float4 body left as it was
        assert all(S.worst(o, r, bd) > 1.0 for o, r, bd in zip(out, ref, bound)), phase
        out = [o.clone() for o in S.adam_eval(p, g, m, v, 2, 0.0, F32)]
        for o, old in zip(out, (p, m, v)):
            o[0] = old[0]                               # the head element in front of the first 16-byte boundary skipped
        assert all(S.worst(o, r, bd) > 1.0 for o, r, bd in zip(out, ref, bound)), phase


def test_fault_segment_sum_last_row_lane_and_wrong_clip():
    case = S.SEG_CASES[3]
    x, dy, gate, add = S.seg_inputs(case)
    ref, bound = S.seg_eval(x, dy, gate, add, 1.0), S.seg_bounds(x, dy, gate, add, 1.0, S.seg_plan(case))
    out = S.seg_eval(x[:, :-1], dy[:, :-1], gate, add, 1.0, F32)
    assert S.worst(out[0], ref[0], bound[0]) > 1.0 and S.worst(out[1], ref[1], bound[1]) > 1.0
    out = S.seg_eval(x, dy, gate.roll(1, 0), add, 1.0, F32)
    assert S.worst(out[2], ref[2], bound[2]) > 1.0


# ---- 3. routes ------------------------------------------------------------------------------------------------------------------------------
def test_case_lists_state_the_routes_the_planners_give():
    for k in S.BN_CASES:
        assert S.bn_plan(k.rows, k.c, k.aligned).route == k.fwd, k
        assert S.bwd_plan(k.rows, k.c, k.aligned).route == k.bwd, k
        assert S.apply_route(k.c, k.aligned) == k.apply, k
    assert {k.c for k in S.BN_CASES} >= {34, 60, 120, 130, 4, 32, 256, 1024, 64}
    assert {k.rows for k in S.BN_CASES} >= {1, 2, 29, 33, 127, 129, 520, 1024, 1025}
    p = S.bn_plan(520, 64)
    assert (p.nblk, p.rows_per, 520 - 2 * p.rows_per) == (3, 174, 172)
    assert S.bn_plan(129, 34).nblk == 2 and S.bn_plan(127, 130).nblk == 1 and S.bn_plan(3712, 34).nblk == 29
    assert S.bn_plan(29, 1024).lanes == 1 and S.bn_plan(1024, 4).lanes == 256
    assert S.bn_plan(10 ** 6, 34).nblk <= S.COL_MAX_PART
    for case in S.SEG_CASES:
        assert S.seg_plan(case).route == case.route, case
    assert S.seg_plan(S.SEG_CASES[6]).nblk == 2
    assert S.adam_plan(4103) == S.AdamPlan("float4", 0, 1025, 3, 2)
    assert S.adam_plan(1027, 1) == S.AdamPlan("float4", 3, 256, 0, 1) and S.adam_plan(9, 3) == S.AdamPlan("float4", 1, 2, 0, 1)
    assert S.adam_plan(7).route == "scalar" and S.adam_plan(1027, 0, 2).route == "scalar" and S.adam_plan(8).route == "float4"
    assert S.sl1_blocks(262147) == 1024 and S.sl1_blocks(257) == 2 and -(-262147 // (1024 * 256)) == 2
    for c in S.GAP_C:
        assert S.gap_tiles(c)[2] > 256 // c


# ---- 4. the measured tolerance is fresh -----------------------------------------------------------------------------------------------------
def test_batchnorm_backward_cpu_float32_figures_are_current():
    seen = {c: (0.0, None) for c in S.BN_CLASSES}
    for case in S.BN_CASES:
        for cls in S.BN_CLASSES:
            x, g, b, dy, rm, rv = S.bn_inputs(case.rows, case.c, cls)
            ref = S.bn_forward_f64(x, g, b, rm, rv, 0.1)
            m32, r32 = ref["mean"].float(), ref["rstd"].float()
            dx = S.bn_dx_cpu_float32(x, dy, g, m32, r32)
            err = float(((dx.double() - S.bn_backward_f64(x, dy, g, m32, r32)["dx"]).abs() / S.bn_dx_unit(dy, g, r32)).max())
            if err > seen[cls][0]:
                seen[cls] = (err, (case.rows, case.c))
    print("torch float32 CPU batch-norm backward, worst |dx - float64| / unit per class:", {c: (f"{v:.3e}", w) for c, (v, w) in seen.items()})
    for cls, (v, _) in seen.items():
        rec = S.BN_DX_CPU_F32[cls]
        assert rec / 2 <= v <= rec * 2, f"{cls}: measured {v:.3e}, recorded {rec:.3e}"


# ---- 5. the bf16 restatement -----------------------------------------------------------------------------------------------------------------
def test_bf16_restatement_is_torchs_cast_and_keeps_nan():
    bits = S.bf16_finite_bits()
    want = S.bits_to_f32(bits).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    for nan_case in (True, False):
        assert np.array_equal(S.bf16_rne_bits(bits, nan_case), want)
    assert S.is_bf16_nan(S.bf16_rne_bits(S.BF16_NAN_BITS)).all()
    old = S.bf16_rne_bits([0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001], nan_case=False)
    assert old.tolist() == [0x8000, 0x0000, 0x7F80] and not S.is_bf16_nan(old).any()
    assert {0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x00000001, 0x80000000, 0x7F800000} <= set(bits)
