"""CPU checks of tests/grads_f64.py.  (1) The per-element bounds the GPU tests of the training backward kernels use are not violated by correct
arithmetic: the emulated split-bf16 / float32 data flow, in two summation orders, stays at or under half of them at EVERY case of every list.
(2) They are not vacuous: each single-site fault named in grads_f64's emulations, switched on, exceeds its bound at listed cases (a failing
assertion names tensor, slice and element through compare_sliced).  (3) The kernel route each case's comment states is the one the restated
planners (plan_lingrad, the XCD blocking, plan_gemm_tn, cpw_of, plan_c1w, ln_ex_rows_per_wave) give.  (4) The recorded error of torch's float32
CPU LayerNorm backward, which the dx tolerance is 4 x of, is re-measured and must not be stale by more than 2 x."""
import pytest
import torch

import grads_f64 as G

WORST = {}
HALF = 0.5


def _half(name, got, ref, bound, what, axes):
    el = G.compare_sliced(got, ref, bound, what, axes)[2]
    assert el <= HALF, f"{what}: correct arithmetic reaches {el:.3f} of the bound"
    WORST[name] = max(WORST.get(name, 0.0), el)


def _exceeds(got, ref, bound, axes):
    return G.sliced_errors(got, ref, bound, axes)[2][0] > 1.0


def _caught(got, ref, bound, what, axes):
    """The faulty result must fail compare_sliced, and the message must name a slice and an element."""
    with pytest.raises(AssertionError) as e:
        G.compare_sliced(got, ref, bound, what, axes)
    assert what in str(e.value) and "worst element" in str(e.value) and "worst slice" in str(e.value)


def _report(*names):
    print("; ".join(f"{n} {WORST[n]:.3f}" for n in names), "(worst element of correct arithmetic as a fraction of the bound)")
    for n in names:         # the figures grads_f64 records are these, rounded up
        assert WORST[n] <= G.WORST_OF_CORRECT_ARITHMETIC[n], f"{n}: {WORST[n]:.3f} against the recorded {G.WORST_OF_CORRECT_ARITHMETIC[n]}"


# ---- 1. correct arithmetic stays inside half the bounds -------------------------------------------------------------------------------------
def test_lingrad_emulation_is_within_half_the_bound_at_every_case():
    for c in G.WGRAD_CASES:
        dy, x = G.wgrad_inputs(c.rows, c.n, c.k)
        rw, rb = G.wgrad_f64(dy, x)
        bw, bb = G.wgrad_bounds(dy, x, G.E_X3, c.S)
        for order in ("forward", "reversed"):
            dw, db = G.emulate_lingrad(dy, x, order)
            what = f"lingrad {c.rows}x{c.n}x{c.k} {order}"
            _half("eg_linear_wgrad_mfma dW", dw, rw, bw, what + " dW", G.WG_AXES)
            _half("eg_linear_wgrad_mfma db", db, rb, bb, what + " db", ("column",))
    _report("eg_linear_wgrad_mfma dW", "eg_linear_wgrad_mfma db")


def test_gemm_tn_and_colsum_emulations_are_within_half_the_bound_at_every_case():
    for c in G.TN_CASES:
        if c.m * c.n * c.k > 1 << 28:
            continue                        # (512 x 512 x 4097 is there for the plan; its arithmetic is that of the other split cases)
        a, b, prev = G.gemm_tn_inputs(c.m, c.n, c.k)
        prev = prev if c.accumulate else None
        ref = G.wgrad_f64(a, b, prev)[0]
        bound = G.wgrad_bounds(a, b, 0.0, c.nz, prev)[0]
        for order in ("forward", "chunked"):
            _half("eg_gemm_tn", G.emulate_gemm_tn(a, b, prev, order), ref, bound, f"gemm_tn {c.m}x{c.n}x{c.k} acc {c.accumulate} {order}", G.WG_AXES)
    for rows, c, _, z in G.COLSUM_CASES:
        a, b = G.colsum_inputs(rows, c)
        b0, b1 = G.colsum_bounds(a, b, z)
        for flip in (False, True):
            af, bf = (a.flip(0), b.flip(0)) if flip else (a, b)
            _half("eg_colsum", af.float().sum(0), a.double().sum(0), b0, f"colsum {rows}x{c} sum a", ("column",))
            _half("eg_colsum", (af.float() * bf.float()).sum(0), (a.double() * b.double()).sum(0), b1, f"colsum {rows}x{c} sum a b", ("column",))
    _report("eg_gemm_tn", "eg_colsum")


def _att_case(c):
    q, k, v, do = G.att_train_inputs(c.lq, c.lk, c.cls)
    M = G.att_mask(c.lq, c.lk, c.p, c.offset)
    P = G.att_softmax_f32(q, k)
    return q, k, v, P, do, M


def test_attention_backward_emulation_is_within_half_the_bound_at_every_case():
    for c in G.ATT_TRAIN_CASES + G.ATT_CHAINED_CASES:
        args = _att_case(c)
        ref, bound = G.att_backward_f64(*args), G.att_backward_bounds(*args)
        for order in ("forward", "chunked"):
            got = dict(zip(("dq", "dk", "dv"), G.emulate_att_backward(*args, order=order)))
            for name, axes in (("dq", G.DQ_AXES), ("dk", G.DK_AXES), ("dv", G.DK_AXES)):
                _half(f"eg_attention_backward_train {name}", got[name], ref[name], bound[name], f"attention backward {c.lq}x{c.lk} p {c.p} {c.cls} {order} {name}", axes)
    _report(*(f"eg_attention_backward_train {n}" for n in ("dq", "dk", "dv")))


def test_attention_mask_is_a_dropout_mask():
    """M is 0 or fl32(1 / (1 - p)), keeps about 1 - p, and an offset above 2^32 gives another mask than its low word alone."""
    for p in (0.1, 0.5):
        M = G.att_mask(33, 65, p, 4096)
        vals = set(M.unique().tolist())
        assert len(vals) == 2 and 0.0 in vals and abs(max(vals) - 1 / (1 - p)) < 1e-6
        assert abs(float((M != 0).double().mean()) - (1 - p)) < 0.03
    assert not torch.equal(G.att_mask(20, 34, 0.1, (1 << 32) + 12345), G.att_mask(20, 34, 0.1, 12345))


def test_conv1d_cl_emulation_is_within_half_the_bound_at_every_case():
    for c in G.C1_CASES:
        r = G.c1_f64(c)
        for order in ("forward", "taps"):
            e = G.emulate_c1(c, order)
            what = f"conv1d_cl {tuple(c[:8])} {order}"
            _half("eg_conv1d_cl_forward", e["y"], r["y"], r["b_y"], what + " y", G.C1_AXES)
            _half("eg_conv1d_cl_backward_input", e["dx"], r["dx"], r["b_dx"], what + " dx", G.C1_AXES)
            _half("eg_conv1d_cl_backward_weight", e["dw"], r["dw"], r["b_dw"], what + " dw", ("output channel", "input channel", "tap"))
            _half("eg_conv1d_cl_backward_weight", e["db_dy"], r["db_dy"], r["b_db_dy"], what + " db_dy", ("channel",))
    _report("eg_conv1d_cl_forward", "eg_conv1d_cl_backward_input", "eg_conv1d_cl_backward_weight")


def test_layernorm_affine_emulation_is_within_half_the_bound_at_every_case():
    for rows, d, rw in G.LNB_EX_CASES:
        for cls in G.LNB_CLASSES:
            x, dy, g, row_cls = G.lnb_inputs(rows, d, cls)
            _, _, rg, rb = G.lnb_f64(x, dy, g)
            bg, bb = G.lnb_affine_bounds(x, dy, row_cls)
            for order in ("forward", "reversed"):
                if order == "reversed" and rows > 2049:
                    continue
                dg, db = G.emulate_lnb_affine(x, dy, rw, order)
                _half("layernorm dgamma", dg, rg, bg, f"layernorm_backward_ex {rows}x{d} {cls} {order} dgamma", ("column",))
                _half("layernorm dbeta", db, rb, bb, f"layernorm_backward_ex {rows}x{d} {cls} {order} dbeta", ("column",))
    _report("layernorm dgamma", "layernorm dbeta")


def test_layernorm_backward_cpu_float32_figures_are_current():
    """LN_BWD_CPU_F32, which the dx tolerance of the GPU tests is LN_BWD_FACTOR x of: re-measured, neither above the record nor below half of it."""
    for which in ("plain2", "plain", "ex"):
        for cls, (e, where) in G.measure_ln_bwd_cpu_f32(which).items():
            rec = G.LN_BWD_CPU_F32[which][cls]
            print(f"LN_BWD_CPU_F32 {which} {cls}: {e:.3g} at {where} (recorded {rec:.3g})")
            assert rec / 2 <= e <= rec * 2 and rec > 0, f"{which} {cls}: measured {e:.3g} at {where}, recorded {rec:.3g}"
    for cls, e in G.measure_ln_xhat_cpu_f32_d2().items():
        rec = G.LN_XHAT_CPU_F32_D2[cls]
        assert rec / 2 <= e <= rec * 2, f"LN_XHAT_CPU_F32_D2 {cls}: measured {e:.3g}, recorded {rec:.3g}"
    # at every other width torch's own float32 forward is inside a quarter of the forward tolerance the xhat and dgamma checks borrow, with room
    for which in ("plain", "ex"):
        for rows, d in G.ln_bwd_case_list(which):
            for cls in G.LNB_CLASSES:
                x, _, _, row_cls = G.lnb_inputs(rows, d, cls)
                z = G.TF.layer_norm(x.double(), (d,), None, None, G.LNB_EPS)
                e = (G.TF.layer_norm(x.float(), (d,), None, None, G.LNB_EPS).double() - z).abs()
                assert bool((e <= G.lnb_xhat_tol(x, row_cls) * 0.3).all()), (which, rows, d, cls)
    # the kernel's formula in float32 with the corrected mean stays inside the tolerance (4 x the CPU figure) at every case
    for which in ("plain2", "plain", "ex"):
        for rows, d in G.ln_bwd_case_list(which):
            for cls in G.LNB_CLASSES:
                x, dy, g, _ = G.lnb_inputs(rows, d, cls)
                e = float(((G.emulate_lnb_dx(x, dy, g, 1).double() - G.lnb_f64(x, dy, g)[0]).abs() / G.lnb_dx_scale(x, g)).max())
                assert e <= G.lnb_dx_tol(which, cls), f"{which} {rows}x{d} {cls}: the fp32 formula is at {e:.3g}, tolerance {G.lnb_dx_tol(which, cls):.3g}"


# ---- 2. single-site faults exceed the bounds ------------------------------------------------------------------------------------------------
def _lingrad_fault(c, fault):
    dy, x = G.wgrad_inputs(c.rows, c.n, c.k)
    (rw, rb), (bw, bb) = G.wgrad_f64(dy, x), G.wgrad_bounds(dy, x, G.E_X3, c.S)
    dw, db = G.emulate_lingrad(dy, x, "forward", fault)
    return (dw, rw, bw, G.WG_AXES), (db, rb, bb, ("column",))


def test_fault_lingrad_last_row_group_of_a_slice_dropped():
    seen = 0
    for c in G.WGRAD_CASES:
        if c.rows < 33 or c.layout != "dense":
            continue                    # (with one group only, dropping it leaves nothing: that is no subtle fault)
        w, _ = _lingrad_fault(c, "drop_group")
        assert _exceeds(*w), c
        seen += 1
    assert seen >= 20
    _caught(*_lingrad_fault(G.WGRAD_CASES[3], "drop_group")[0][:3], "rows 33 dW", G.WG_AXES)      # 33 rows: ONE row of one group is missing
    c = next(c for c in G.WGRAD_CASES if c.rows == 1025)
    assert _exceeds(*_lingrad_fault(c, "drop_group")[0]), "the one-row last slice of 1025 rows"


def test_fault_lingrad_lo_hi_term_missing_in_one_16x16_tile():
    """2^-8 relative in one tile of 16 (or more): invisible to a norm over the tensor, above E_bf16x3 per element while R is small."""
    seen = 0
    for c in G.WGRAD_CASES:
        if c.rows > 129 or c.layout != "dense" or c.rows < 4:
            continue
        (dw, rw, bw, axes), _ = _lingrad_fault(c, "lohi_tile")
        assert _exceeds(dw, rw, bw, axes), c
        assert float((dw.double() - rw).norm() / rw.norm()) < 2e-5 or c.n * c.k <= 64 * 64, c      # the existing global check would pass it
        seen += 1
    assert seen >= 20


def test_fault_lingrad_a_slice_left_out_of_the_fold_and_db_faults():
    split = [c for c in G.WGRAD_CASES if c.S > 1]
    assert len(split) >= 8
    for c in split:
        w, _ = _lingrad_fault(c, "fold_skip")
        assert _exceeds(*w), c
    for c in G.WGRAD_CASES:
        if c.rows >= 17 and c.layout != "nodb":
            _, b = _lingrad_fault(c, "db_rows")
            assert _exceeds(*b), c
    moved = [c for c in G.WGRAD_CASES if c.xcd != (0, 0) and any(
        G.lingrad_remap(0, by, G.cdiv(c.k, 64), G.cdiv(c.n, 64), *c.xcd) != (0, by) for by in range(G.cdiv(c.n, 64)))]
    assert moved, "no case whose remap moves a db tile"
    for c in moved:
        _, b = _lingrad_fault(c, "db_unremapped")
        assert _exceeds(*b), c
    _caught(*_lingrad_fault(moved[0], "db_unremapped")[1][:3], "db 256x256", ("column",))


@pytest.mark.parametrize("fault", ["rowsum_quarter", "mask_dv_only", "chunk_dk", "no_eighth_dk", "neighbour_mask"])
def test_fault_attention_backward(fault):
    seen = 0
    for c in G.ATT_TRAIN_CASES:
        qc = G.att_route(c.lk)[1]
        if (fault == "rowsum_quarter" and c.lk < 4) or (fault in ("mask_dv_only", "neighbour_mask") and c.p == 0) or (fault == "chunk_dk" and c.lq <= qc) \
                or (fault == "neighbour_mask" and c.lk % 16 == 0) or c.lk == 1:
            continue
        args = _att_case(c)
        if fault == "neighbour_mask" and torch.equal(args[5][..., c.lk - 1], args[5][..., c.lk - 2]):
            continue
        ref, bound = G.att_backward_f64(*args), G.att_backward_bounds(*args)
        got = dict(zip(("dq", "dk", "dv"), G.emulate_att_backward(*args, fault=fault)))
        hit = [n for n, axes in (("dq", G.DQ_AXES), ("dk", G.DK_AXES), ("dv", G.DK_AXES)) if _exceeds(got[n], ref[n], bound[n], axes)]
        assert hit, (fault, c)
        if fault in ("chunk_dk", "no_eighth_dk"):
            assert hit == ["dk"], (fault, c, hit)
        seen += 1
    assert seen >= 3, (fault, seen)


def test_fault_conv1d_cl():
    seam = [c for c in G.C1_CASES if G.c1_len_out(c.l, c.k, c.stride, c.pad, c.dil) > 64]
    assert len(seam) >= 8
    for c in seam:
        r, e = G.c1_f64(c), G.emulate_c1(c, "forward", "seam_tap")
        assert _exceeds(e["y"], r["y"], r["b_y"], G.C1_AXES), c
    _caught(G.emulate_c1(seam[0], "forward", "seam_tap")["y"], G.c1_f64(seam[0])["y"], G.c1_f64(seam[0])["b_y"], "seam y", G.C1_AXES)
    tiled = [c for c in G.C1_CASES if c.dw.startswith("dw_tiled")]
    assert len(tiled) >= 8
    for c in tiled:
        r, e = G.c1_f64(c), G.emulate_c1(c, "forward", "fold_tail")
        assert _exceeds(e["dw"], r["dw"], r["b_dw"], ("output channel", "input channel", "tap")), c
    for c in G.C1_CASES:
        r, e = G.c1_f64(c), G.emulate_c1(c, "forward", "bias_twice")
        assert _exceeds(e["dx"], r["dx"], r["b_dx"], G.C1_AXES), c


def test_fault_layernorm_backward():
    seen = 0
    for rows, d, rw in G.LNB_EX_CASES:
        if rows > 2049:
            continue
        for cls in G.LNB_CLASSES:
            x, dy, g, row_cls = G.lnb_inputs(rows, d, cls)
            rdx, _, rg, _ = G.lnb_f64(x, dy, g)
            bad = G.emulate_lnb_dx(x, dy, g, rw, "xhat_b_last_row")
            e = float(((bad.double() - rdx).abs() / G.lnb_dx_scale(x, g)).max())
            if not (cls == "constrow" and rows == 1):       # (a single constant row has xhat = 0: the term is zero anyway)
                assert e > G.lnb_dx_tol("ex", cls), (rows, d, cls, e)
            if cls == "constrow" and rw == 1 and rows // 2 == 1:
                continue                                    # (wave 1 holds the constant row alone: xhat = 0 there, nothing to miss)
            if rows >= 2 * rw and cls != "mean100":         # (the offset rows' forward tolerance, 1.3e-2 of sum |dy|, hides one wave among >= 1023 rows)
                bg, _ = G.lnb_affine_bounds(x, dy, row_cls)
                dg, _ = G.emulate_lnb_affine(x, dy, rw, "forward", "dgamma_wave")
                assert _exceeds(dg, rg, bg, ("column",)), (rows, d, cls)
                seen += 1
    assert seen >= 20


# ---- 3. the routes the case lists state -----------------------------------------------------------------------------------------------------
def test_case_lists_state_the_routes_the_planners_give():
    for c in G.WGRAD_CASES:
        assert G.plan_lingrad(c.rows, c.n, c.k) == (c.S, c.rows_per) and G.lingrad_xcd(c.n, c.k) == c.xcd, c
        assert (G.lingrad_workspace_floats(c.rows, c.n, c.k) > 0) == (c.S > 1)
    rows64 = {c.rows for c in G.WGRAD_CASES if (c.n, c.k) == (64, 64)}
    assert rows64 >= {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 640, 641, 768, 1025, 1100}
    assert {c.n for c in G.WGRAD_CASES if c.rows == 70} >= {1, 3, 4, 63, 64, 65, 66, 127, 128, 130} <= {c.k for c in G.WGRAD_CASES if c.rows == 70} | {63, 65}
    assert {c.k for c in G.WGRAD_CASES if c.rows == 70} >= {1, 3, 4, 63, 64, 65, 66, 127, 128, 130}
    assert (1025 - 4 * 256, 1025 // 256) == (1, 4)              # S = 5: the last slice of 1025 rows holds one row
    assert {(c.n, c.k) for c in G.WGRAD_CASES if c.xcd != (0, 0)} >= {(64, 512), (512, 64), (128, 256), (256, 256), (200, 100)}
    assert any(c.xcd != (0, 0) and c.S > 1 for c in G.WGRAD_CASES)
    for c in G.TN_CASES:
        splits, kps, nz = G.plan_gemm_tn(c.m, c.n, c.k)
        assert nz == c.nz and kps % 32 == 0 and (nz - 1) * kps < c.k <= nz * kps, c
    assert G.plan_gemm_tn(512, 512, 4097) == (16, 288, 15)
    assert {c.k for c in G.TN_CASES} >= {1, 31, 32, 33, 255, 256, 257, 513, 1000} and {c.m for c in G.TN_CASES} >= {1, 63, 64, 65, 130} <= {c.n for c in G.TN_CASES}
    assert {r[2] for r in G.COLSUM_CASES} == {"col_direct_kernel", "col_partial_fast_kernel", "col_partial_kernel"}
    for c in G.ATT_TRAIN_CASES + G.ATT_CHAINED_CASES:
        assert G.att_route(c.lk) == c.route and (c.layout != "qkv3" or c.lq == c.lk), c
    assert {c.lk for c in G.ATT_TRAIN_CASES if c.lq == 20} >= {1, 4, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128}
    assert {c.lq for c in G.ATT_TRAIN_CASES if c.lk == 34} >= {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130}
    assert {c.lq for c in G.ATT_TRAIN_CASES if c.lk == 120} >= {31, 32, 33, 65}
    assert {c.route for c in G.ATT_CHAINED_CASES} == {(3, 64), (4, 64), (8, 32)}
    for c in G.C1_CASES:
        lo = G.c1_len_out(c.l, c.k, c.stride, c.pad, c.dil)
        assert lo >= 1 and (lo - 1) * c.stride - c.pad + (c.k - 1) * c.dil <= c.l - 1 + c.pad, c
        got = (G.c1_forward_route(c.ci, c.co, c.k, c.stride, c.pad, c.dil), G.c1_input_route(c.ci, c.co, c.k, c.stride, c.pad, c.dil),
               G.c1_weight_route(c.b, c.ci, lo, c.co, c.k, c.stride, c.dil))
        assert got == (c.fwd, c.dx, c.dw), (c, got)
    edge = {1, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65}
    assert {c.co for c in G.C1_CASES} >= edge <= {c.ci for c in G.C1_CASES}
    assert {c.fwd for c in G.C1_CASES} == {"fwd_untiled"} | {f"fwd_tiled<{w}>" for w in (1, 2, 4, 8, 12, 16)}
    assert {c.dx for c in G.C1_CASES} == {"dx_untiled"} | {f"dx_tiled<{w}>" for w in (1, 2, 4, 8, 12, 16)}
    assert {c.dw.split("/")[0] for c in G.C1_CASES} == {"dw_one", "dw_tiled<8>", "dw_tiled<16>", "dw_tiled<36>"}
    assert {int(c.dw.split("/")[1]) for c in G.C1_CASES if "/" in c.dw} >= {4, 5, 13, 16, 17, 29}
    assert any(c.pad > (c.k - 1) * c.dil and c.fwd.startswith("fwd_tiled") and c.dx == "dx_untiled" for c in G.C1_CASES)
    assert all(G.c1_weight_route(c.b, c.ci, G.c1_len_out(c.l, c.k, c.stride, c.pad, c.dil), c.co, c.k, c.stride, c.dil, db_x=True) == "dw_one" for c in G.C1_DBX_CASES)
    assert [G.ln_ex_rows_per_wave(r) for r in (1, 1024, 1025, 2048, 2049, 8200)] == [1, 1, 2, 2, 3, 8]
    for rows, d, rw in G.LNB_EX_CASES:
        assert rw == G.ln_ex_rows_per_wave(rows) and d % 64 == 0 and d <= 1024
    assert {r for r, _, _ in G.LNB_EX_CASES} == set(G.LNB_EX_ROWS) and {d for _, d, _ in G.LNB_EX_CASES} == set(G.LNB_EX_D)
    assert G.cdiv(8200, 4 * 8) * 32 - 8200 == 24            # the last workgroup of 8200 rows: wave 0 holds 8 rows, waves 1 .. 3 none
