"""CPU checks of tests/misc_f64.py.  (1) The per-element bounds the GPU tests of the prior encoder, the contrastive loss, eg_small_linear and
eg_conv_transpose1d use are not violated by correct arithmetic: the emulated fp32 data flow, in two summation orders, stays at or under half of them
at EVERY case.  (2) They are not vacuous: each single-site fault, switched on, exceeds its bound on a named case.  (3) Every prior-encoder case takes
the route its comment states, by the restated launch arithmetic, and its inputs meet the conditions that let the gates discriminate.  (4) The closed
form of the contrastive gradients is torch's float64 autograd, and the recorded error of torch's float32 CPU autograd, which the gradient tolerance
is 4 x of, is re-measured and must not be stale by more than 2 x."""
import functools

import pytest
import torch

import misc_f64 as M

WORST = {}
HALF = 0.5
F32 = torch.float32
ORDERS = (False, True)


def _half(name, got, ref, bound, what):
    el = M.worst(got, ref, bound)
    assert el <= HALF, f"{what}: correct arithmetic reaches {el:.3f} of the bound ({name})"
    WORST[name] = max(WORST.get(name, 0.0), el)


def _report(*names):
    print("; ".join(f"{n} {WORST[n]:.3f}" for n in names), "(worst element of correct arithmetic as a fraction of the bound)")
    for n in names:
        assert WORST[n] <= M.WORST_OF_CORRECT_ARITHMETIC[n], f"{n}: {WORST[n]:.3f} against the recorded {M.WORST_OF_CORRECT_ARITHMETIC[n]}"


def _exceeds(got, ref, bound):
    return M.worst(got, ref, bound) > 1.0


@functools.lru_cache(maxsize=None)
def _prior(i):
    c = M.PRIOR_CASES[i]
    inp = M.prior_inputs(c)
    ref, bound = M.prior_bounds(inp, c)
    return c, inp, ref, bound


def _prior_named(**kw):
    for i, c in enumerate(M.PRIOR_CASES):
        if all(getattr(c, k) == v for k, v in kw.items()):
            return _prior(i)
    raise KeyError(kw)


LIVE = [i for i, c in enumerate(M.PRIOR_CASES) if not c.refused]
PRIOR_KEYS = ("cat", "tm_mem", "tm_pe", "tm_gram")


# ---- prior encoder ----------------------------------------------------------------------------------------------------------------------------
def test_prior_cases_take_the_route_they_state():
    for c in M.PRIOR_CASES:
        plan = M.prior_plan(c)
        assert (plan.staged, plan.refused) == (c.staged, c.refused), (c, plan)
        assert plan.slices == (1 if c.variant == 1 else M.cdiv(c.D, 64))
        assert c.Dpad >= c.D and (c.variant == 0 or 1 <= c.chunk <= min(c.P, c.PL, 64))
    byD = {c.D: M.prior_plan(c).slices for c in M.PRIOR_SPATIAL}
    assert (byD[1], byD[63], byD[64], byD[65], byD[126], byD[128], byD[282]) == (1, 1, 1, 2, 2, 2, 5)
    unstaged = [c for c in M.PRIOR_SPATIAL if not c.staged]
    assert len(unstaged) == 1 and M.prior_plan(unstaged[0]).smem == 64080
    assert M.prior_plan(M.PRIOR_MEMORY[-1]).smem == 274016 and M.prior_plan(M.PRIOR_MEMORY[-2]).smem == 138176


def test_prior_emulation_in_float64_is_the_reference():
    """The sliced data flow (halos, zeroed hidden positions, the gates) is the plain operator: in float64 the two agree to rounding."""
    for i in LIVE:
        c, inp, ref, _ = _prior(i)
        out = M.emulate_prior(inp, c, torch.float64)
        for k in PRIOR_KEYS:
            if k in out:
                assert float((out[k] - ref[k]).abs().max()) <= 1e-11 * max(1.0, float(ref[k].abs().max())), (c, k)


def test_prior_emulation_is_within_half_the_bound_at_every_case():
    for i in LIVE:
        c, inp, ref, bound = _prior(i)
        for flip in ORDERS:
            out = M.emulate_prior(inp, c, F32, flip)
            for k in bound:
                _half("prior " + k, out[k], ref[k], bound[k], f"prior {c[:7]} flip {flip} {k}")
            assert torch.equal(out["cat"][:, :c.P, :c.D], inp["prior"]) and bool((out["cat"][:, :, c.D:] == 0).all())
    _report(*("prior " + k for k in PRIOR_KEYS))


def test_prior_memory_inputs_let_the_gates_discriminate():
    """Conditions on the float64 reference alone: every SP sigmoid in [0.05, 0.95]; every TM softmax row has two weights >= 0.05 (chunk >= 2); the
    clips of a batch are coupled through the gram, so clip 0 of a batch differs from clip 0 alone by more than its bound (10 to 100 x at the TED-sized cases, 1.3 x at the BEAT shape, whose bound carries 2820-term sums)."""
    for i in LIVE:
        c, inp, ref, bound = _prior(i)
        if c.variant != 1:
            continue
        assert 0.05 <= float(ref["s"].min()) and float(ref["s"].max()) <= 0.95, (c, float(ref["s"].min()), float(ref["s"].max()))
        assert float(ref["s"].max() - ref["s"].min()) > 0.2, c
        second = ref["w"].topk(2, dim=1).values[:, 1]
        assert float(second.min()) >= 0.05, (c, float(second.min()))
        if c.B > 1:
            alone = dict(inp, prior=inp["prior"][:1].contiguous())
            one = M.prior_f64(alone, c._replace(B=1))
            assert M.worst(one["cat"], ref["cat"][:1], bound["cat"][:1]) > 1.2, c


PRIOR_FAULT_CASE = {
    "halo_wrong_side": dict(variant=0, D=128),
    "hidden_halo_from_bias": dict(variant=0, D=126),
    "affine_before_relu": dict(variant=0, D=63),
    "mem_first_chunk": dict(variant=1, P=6, chunk=4),
    "pe_ungated": dict(variant=1, B=4),
    "gram_own_clip": dict(variant=1, B=4),
    "row_times_w": dict(variant=1, B=1),
    "pad_unwritten": dict(variant=0, D=282),
}


@pytest.mark.parametrize("fault", M.PRIOR_FAULTS)
def test_prior_fault_exceeds_a_bound(fault):
    c, inp, ref, bound = _prior_named(**PRIOR_FAULT_CASE[fault])
    out = M.emulate_prior(inp, c, F32, False, fault)
    assert any(_exceeds(out[k], ref[k], bound[k]) for k in bound), f"{fault} stays inside every bound at {c}"
    if fault == "halo_wrong_side":          # and at the one-column slice, whose whole input is halo
        c, inp, ref, bound = _prior_named(variant=0, D=65)
        assert _exceeds(M.emulate_prior(inp, c, F32, False, fault)["cat"], ref["cat"], bound["cat"])
    if fault == "hidden_halo_from_bias":    # visible at the first and the last column only
        bad = (M.emulate_prior(inp, c, F32, False, fault)["cat"].double() - ref["cat"]).abs() > bound["cat"]
        cols = bad.nonzero()[:, 2].unique().tolist()
        assert cols == [0, c.D - 1], cols
    if fault == "mem_first_chunk":          # invisible where P == chunk
        c2, inp2, ref2, bound2 = _prior_named(variant=1, B=4)
        out2 = M.emulate_prior(inp2, c2, F32, False, fault)
        assert not any(_exceeds(out2[k], ref2[k], bound2[k]) for k in bound2)


# ---- contrastive loss -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _con(i, cls):
    case = M.CON_CASES[i]
    face, audio = M.con_inputs(case.n, case.d, cls)
    ref, bound = M.con_bounds(face, audio)
    return case, face, audio, ref, bound


def _con_all():
    for i, case in enumerate(M.CON_CASES):
        for cls in M.con_classes_for(case):
            yield _con(i, cls)


def _check_forward(out, ref, bound, what, half):
    """The GPU test's forward criterion on an emulation (half: at half the bounds, recording the worst)."""
    n = ref["cross"].shape[0]
    vac = bound["vacuous"]
    ok = ~vac
    ec = torch.where(vac, torch.zeros_like(bound["cross"]), bound["cross"])
    got = torch.where(ok, out["cross"].double(), ref["cross"])
    rows = bound["row_kind"] != 2
    if half:
        _half("con cross", got, ref["cross"], ec, what + " cross")
        _half("con rowloss", out["rowloss"][rows], ref["rowloss"][rows], bound["rowloss"][rows], what + " rowloss")
        if bound["loss"] != float("inf"):
            _half("con loss", out["loss"], ref["loss"], torch.tensor(bound["loss"]), what + " loss")
    bad = _exceeds(got, ref["cross"], ec) or _exceeds(out["rowloss"][rows], ref["rowloss"][rows], bound["rowloss"][rows])
    if bound["loss"] != float("inf"):
        bad = bad or _exceeds(out["loss"], ref["loss"], torch.tensor(bound["loss"]))
    bad = bad or not bool(torch.isfinite(out["loss"])) or not bool((out["cross"].double()[vac] >= bound["cross_floor"][vac]).all())
    dec = bound["decided"]
    bad = bad or not torch.equal(out["hit"][dec], ref["hit"][dec])
    return bad


def test_contrastive_forward_emulation_is_within_half_the_bound_at_every_case():
    kinds = set()
    for case, face, audio, ref, bound in _con_all():
        kinds |= set(bound["row_kind"].tolist())
        for flip in ORDERS:
            out = M.con_forward(face, audio, F32, flip)
            assert not _check_forward(out, ref, bound, f"contrastive {case.n}x{case.d} flip {flip}", True), (case, flip)
    assert kinds == {0, 1, 2}
    _report("con cross", "con rowloss", "con loss")


def test_contrastive_input_classes_are_what_they_claim():
    for i, case in enumerate(M.CON_CASES):
        if case.d == 1 or case.n == 1:
            continue
        _, face, audio, ref, bound = _con(i, "near")
        diag = ref["D"].diagonal()
        assert 5e-3 < float(diag.min()) and float(diag.max()) < 2e-2 and bool(bound["decided"].all()) and bool(ref["hit"].all())
        assert bool((bound["row_kind"] == 0).all()), "the near class must stay inside the bounded regime"
        _, face, audio, ref, bound = _con(i, "ties")
        for r, (j, j2) in M.con_tie_rows(case.n):
            c = ref["cross"][r]
            assert float(c[j]) == float(c[j2]) == float(c.max()) and bool(bound["decided"][r]) and bool(ref["hit"][r]) == (r == j), (case, r)
        _, face, audio, ref, bound = _con(i, "identical")
        assert float(ref["D"][-1, -1]) == 0.0 and int(bound["row_kind"][-1]) == 1 and bool(bound["vacuous"][-1, -1])
        _, face, audio, ref, bound = _con(i, "zero_row")
        assert float(face[case.n // 2].abs().max()) == 0.0 and float(ref["finv"][case.n // 2]) == 1e12
    assert any(len(M.con_tie_rows(c.n)) == 4 for c in M.CON_CASES), "no case with the two tied columns in one thread (256 apart)"


def _grad_cases():
    for i, case in enumerate(M.CON_CASES):
        if case in M.CON_GRAD_CASES:
            for cls in M.con_classes_for(case):
                yield _con(i, cls) + (cls,)


def _grad_fracs(got, ref, cls):
    tf, ta = M.con_grad_tols(ref, cls)
    return M.worst(got["gface"], ref["gface"], tf), M.worst(got["gaudio"], ref["gaudio"], ta)


def test_contrastive_closed_form_is_autograd_and_the_float32_cpu_error_is_current():
    """con_grads (float64) against torch's float64 autograd of the loss as the reference module states it; then torch's float32 autograd against
    float64 in units of con_grad_unit per class: the recorded figures are its own, not stale by more than 2 x."""
    seen = {}
    for i, case in enumerate(M.CON_CASES):
        if case not in M.CON_GRAD_MEASURE:
            continue
        for cls in M.con_classes_for(case):
            _, face, audio, ref, bound = _con(i, cls)
            g = M.con_grads(face, audio)
            loss, gf, ga = M.con_torch(face, audio, torch.float64)
            uf, ua = M.con_grad_units(g)
            assert float(((gf - g["gface"]).abs() / uf).max()) < 1e-6 and float(((ga - g["gaudio"]).abs() / ua).max()) < 1e-6, (case, cls)
            if cls == "near":
                assert float(g["gface"].abs().max()) < 1e-36 and float(g["gaudio"].abs().max()) < 1e-36
                continue
            assert abs(float(loss - ref["loss"])) <= 1e-12 * max(1.0, abs(float(ref["loss"])))
            _, gf32, ga32 = M.con_torch(face, audio, F32)
            e = max(float(((gf32.double() - g["gface"]).abs() / uf).max()), float(((ga32.double() - g["gaudio"]).abs() / ua).max()))
            seen[cls] = max(seen.get(cls, 0.0), e)
    print("float32 CPU autograd error per class (units of con_grad_unit):", {k: f"{v:.3g}" for k, v in seen.items()})
    for cls, rec in M.CON_GRAD_CPU_F32.items():
        assert rec / 2 <= seen[cls] <= rec * 2 or (rec >= seen[cls] and rec - seen[cls] < 1e-12), f"{cls}: measured {seen[cls]:.3g}, recorded {rec:.3g}"


def test_contrastive_gradient_emulation_is_within_half_the_tolerance_at_every_case():
    for case, face, audio, ref, bound, cls in _grad_cases():
        g = M.con_grads(face, audio)
        for flip in ORDERS:
            out = M.con_grads(face, audio, F32, flip, fma=flip)         # forwards with separate roundings, backwards with fused multiply-adds
            if cls == "near":
                assert float(out["gface"].abs().max()) <= M.CON_GRAD_NEAR_ABS and float(out["gaudio"].abs().max()) <= M.CON_GRAD_NEAR_ABS
                continue
            ff, fa = _grad_fracs(out, g, cls)
            assert ff <= HALF and fa <= HALF, f"contrastive gradients {case.n}x{case.d} {cls} flip {flip}: {ff:.3f} {fa:.3f} of the tolerance"
            WORST["con gface"], WORST["con gaudio"] = max(WORST.get("con gface", 0.0), ff), max(WORST.get("con gaudio", 0.0), fa)
            if cls == "identical":
                assert float(out["W"][-1, -1]) == 0.0 and float(g["W"][-1, -1]) == 0.0
    _report("con gface", "con gaudio")


CON_FAULT_CASE = {
    "argmax_last": ((12, 64), "ties"), "diag_minus_256": ((257, 3), "generic"), "no_max": ((12, 64), "near"),
    "no_projection": ((12, 64), "generic"), "through_zero": ((12, 64), "identical"), "factored_sum": ((12, 64), "ties"),
}


@pytest.mark.parametrize("fault", sorted(CON_FAULT_CASE))
def test_contrastive_fault_exceeds_a_bound(fault):
    (n, d), cls = CON_FAULT_CASE[fault]
    i = [k for k, c in enumerate(M.CON_CASES) if (c.n, c.d) == (n, d)][0]
    case, face, audio, ref, bound = _con(i, cls)
    if fault in ("no_projection", "through_zero", "factored_sum"):
        g = M.con_grads(face, audio)
        ff, fa = _grad_fracs(M.con_grads(face, audio, F32, False, fault), g, cls)
        assert ff > 1.0 and (fa > 1.0 or fault == "factored_sum"), (fault, ff, fa)      # the factored form loses 1 / D in the face rows next to an audio row
    else:
        out = M.con_forward(face, audio, F32, False, fault)
        assert _check_forward(out, ref, bound, fault, False), f"{fault} stays inside every bound at {case}"
        if fault == "argmax_last":          # both directions: a hit lost and a miss won; the 256-apart form at n = 300
            assert out["hit"][3].item() is False and out["hit"][6].item() is True
            _, f2, a2, r2, b2 = _con([k for k, c in enumerate(M.CON_CASES) if c.n == 300][0], "ties")
            o2 = M.con_forward(f2, a2, F32, False, fault)
            assert o2["hit"][1].item() is False and r2["hit"][1].item() is True and o2["hit"][263].item() is True and r2["hit"][263].item() is False


# ---- small linear, transposed convolution -----------------------------------------------------------------------------------------------------
def test_small_linear_and_transposed_convolution_emulations_are_within_half_the_bound():
    for case in M.SL_CASES:
        x, w, b = M.sl_inputs(case)
        ref, bound = M.sl_eval(x, w, b), M.sl_bound(x, w, b)
        for flip in ORDERS:
            _half("small_linear", M.sl_eval(x, w, b, F32, flip), ref, bound, f"small_linear {case} flip {flip}")
    for case in M.CT_CASES:
        a = M.ct_inputs(case)
        ref, bound = M.ct_f64(*a), M.ct_bound(*a)
        assert float((M.emulate_ct(*a, dt=torch.float64) - ref).abs().max()) < 1e-13, case
        for flip in ORDERS:
            _half("convt", M.emulate_ct(*a, dt=F32, flip=flip), ref, bound, f"convt {case} flip {flip}")
    _report("small_linear", "convt")


def test_small_linear_and_transposed_convolution_faults_exceed_their_bounds():
    for case in M.SL_CASES:
        x, w, b = M.sl_inputs(case)
        assert _exceeds(M.sl_eval(x, w, b, F32, False, "bias_per_lane"), M.sl_eval(x, w, b), M.sl_bound(x, w, b)), case
    for case in M.CT_CASES:
        a = M.ct_inputs(case)
        ref, bound = M.ct_f64(*a), M.ct_bound(*a)
        assert _exceeds(M.emulate_ct(*a, fault="parity"), ref, bound), case
        bad = (M.emulate_ct(*a, fault="keep_lin").double() - ref).abs() > bound
        assert bool(bad[:, :, -1].any()) and not bool(bad[:, :, :-1].any()), f"{case}: the kept li = lin term must show at the last output alone"


def test_embedding_inputs_hold_the_edges():
    for case in M.EMB_CASES:
        idx, table = M.emb_inputs(case)
        rows = M.emb_rows(idx, table)
        assert bool(torch.isfinite(rows).all()) and bool(torch.isnan(table).any())
        if case[0] >= 5:
            assert idx[:5].tolist() == [-1, 0, M.EMB_WORDS - 1, M.EMB_WORDS, 2 ** 40]
            assert torch.equal(rows[0], table[0]) and torch.equal(rows[3], table[-1]) and torch.equal(rows[4], table[-1])
