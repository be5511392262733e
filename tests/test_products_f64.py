"""CPU checks of tests/products_f64.py: the per-element bounds the GPU tests of the linear family and of attention use are not violated by correct
arithmetic (the emulated split-bf16 data flow and torch's float32 stay at or under half of them at every case of every list) and are not vacuous
(nine deliberately wrong restatements -- a split term lost in one 16-column tile's last K step, the last k of a row tile, a bias one column off, res2
in front of the first ReLU, a row shift across a sequence boundary, a key missing from the softmax sum, the mask row of query 0 for every query, a
zero V row, a wrong clamp of the mask row -- exceed them); and the eg_split_tiles slot map of images_of agrees with a second restatement."""
import numpy as np
import pytest
import torch

import products_f64 as P

WORST = {}          # (family, precision) -> worst element fraction of correct arithmetic, printed by the last test of each family


def _note(family, prec, el):
    WORST[(family, prec)] = max(WORST.get((family, prec), 0.0), el)


def _check_linear(what, x, w, bias, r1, r2, relu, shift, seq, prec):
    got = P.emulate_linear(x, w, bias, r1, r2, relu, shift, seq, prec)
    ref = P.linear_f64(x, w, bias, r1, r2, relu, shift, seq)
    _, _, el = P.compare_sliced(got, ref, P.linear_bound(x, w, bias, r1, r2, relu, shift, seq, prec), what, P.LIN_AXES)
    if prec == "bf16" and x.shape[1] == 4:
        # Half the bound cannot be asked here: E_bf16 is attained when the half-ulp errors of both operands align in each of only four products
        # (0.54 - 0.67 of the bound at the six K = 4 shapes).  What the half is for -- room for another summation order -- is asked directly: the
        # error stays inside the representation part E_bf16 S alone, so the order-dependent terms of the bound are untouched.
        S = P.shift_rows(x, shift, seq).double().abs() @ w.double().abs().T
        assert bool(((got.double() - ref).abs() <= P.E_PREC[prec] * S).all()), f"{what}: beyond the representation error"
        return
    assert el <= 0.5, f"{what}: correct arithmetic reaches {el:.3f} of the bound"
    _note("linear", prec, el)


# ---- a. correct arithmetic stays inside the bounds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", P.PRECISIONS)
def test_linear_emulation_is_within_half_the_bound_at_every_case(prec):
    for i, (m, n, k) in enumerate(P.LINEAR_SHAPES):
        _check_linear(f"linear {m}x{n}x{k} {prec}", *P.linear_inputs("lin", m, n, k, i), 0, 1, prec)
    for i, (m, seq, sh, n, k) in enumerate(P.CAUSAL_CASES):
        _check_linear(f"causal {m}/{seq}/{sh} {n}x{k} {prec}", *P.linear_inputs("cau", m, n, k, i), sh, seq, prec)
    for i, (m, n, k, splits) in enumerate(P.SPLITK_CASES):
        x, w, bias, _, _, _ = P.linear_inputs("spk", m, n, k, 1)
        _check_linear(f"split-K {m}x{n}x{k} {prec}", x, w, bias, None, None, True, 0, 1, prec)
    for i, (m, n, k) in enumerate(P.PRESPLIT_CASES):
        _check_linear(f"pre-split {m}x{n}x{k} {prec}", *P.linear_inputs("pre", m, n, k, i), 0, 1, prec)
    print(f"linear {prec}: worst element of correct arithmetic {WORST[('linear', prec)]:.3f} of the bound")


def _check_attention(what, q, k, v, heads, mask, prec):
    out, attn = P.emulate_attention(q, k, v, heads, mask, prec)
    ro, ra = P.attention_f64(q, k, v, heads, mask)
    bo, ba = P.attention_bounds(q, k, v, heads, mask, prec)
    el = max(P.compare_sliced(out, ro, bo, what + " out", P.OUT_AXES)[2], P.compare_sliced(attn, ra, ba, what + " attn", P.ATTN_AXES)[2])
    assert el <= 0.5, f"{what}: correct arithmetic reaches {el:.3f} of the bound"
    _note("attention", prec, el)


@pytest.mark.parametrize("prec", P.PRECISIONS)
def test_attention_emulation_is_within_half_the_bound_at_every_case(prec):
    for lq, lk in P.ATT_SHAPES:
        for heads in P.ATT_HEADS:
            _check_attention(f"attention {lq}x{lk} h{heads} {prec}", *P.attention_inputs(lq, lk, heads), heads, None, prec)
    for lq, lk in P.ATT_CLASS_SHAPES:
        for cls in ("peaked", "flat"):
            _check_attention(f"attention {lq}x{lk} {cls} {prec}", *P.attention_inputs(lq, lk, 2, cls), 2, None, prec)
    for lq, lk in P.ATT_MASK_SHAPES:
        q, k, v = P.attention_inputs(lq, lk, 2)
        for name, mask in P.attention_masks(lq, lk, q.shape[0]).items():
            _check_attention(f"attention {lq}x{lk} mask {name} {prec}", q, k, v, 2, mask, prec)
    print(f"attention {prec}: worst element of correct arithmetic {WORST[('attention', prec)]:.3f} of the bound")


def test_attention_input_classes_are_what_they_are_for():
    for lq, lk in P.ATT_CLASS_SHAPES:
        q, k, v = P.attention_inputs(lq, lk, 2, "peaked")
        s = (P._heads(q.double(), 2) / 8.0) @ P._heads(k.double(), 2).transpose(2, 3)
        top = s.topk(2, dim=-1).values
        assert float((top[..., 0] - top[..., 1]).min()) >= P.PEAK_LEAD
        _, attn = P.attention_f64(q, k, v, 2)
        assert float(attn.max(dim=-1).values.min()) == 1.0 and float(attn.min()) < P.FLT_MIN       # one-hot, and below what fp32 holds elsewhere
        ds = (P.E_PREC["bf16x3"] + 77 * P.U) * (P._heads(q.double(), 2).abs() / 8.0) @ P._heads(k.double(), 2).abs().transpose(2, 3) + P.U * s.abs()
        assert 2 * float(ds.max()) <= 0.05              # the first-order form of attn_bound is good to 3 % (module docstring)
        q, k, v = P.attention_inputs(lq, lk, 2, "flat")
        out, attn = P.attention_f64(q, k, v, 2)
        assert torch.equal(attn, torch.full_like(attn, 1.0 / lk))
        assert float((out - v.double().view(v.shape[0], lk, 2, 64).mean(1).reshape(v.shape[0], 1, 128)).abs().max()) < 1e-15
    for lq, lk in P.ATT_MASK_SHAPES:
        dead = P.attention_masks(lq, lk, 2)["dead_rows"]
        assert int(dead[:, lq - 1].sum()) == 0 and int(dead[:, 0].sum()) == 0      # the last query row is fully masked (query 16 of 17)
        _, attn = P.attention_f64(*P.attention_inputs(lq, lk, 2), 2, dead)
        assert torch.equal(attn[:, :, lq - 1], torch.full_like(attn[:, :, lq - 1], 1.0 / lk))


# ---- b. deliberately wrong restatements exceed the bounds ------------------------------------------------------------------------------------
def _exceeds(got, ref, bound):
    return P.sliced_errors(got, ref, bound, P.LIN_AXES)[2][0] > 1.0


SHALLOW = [(m, n, k) for (m, n, k) in P.LINEAR_SHAPES if k <= 64]


def test_mutation_i_split_term_lost_in_the_last_k_step_of_one_column_tile():
    """x_hi w_lo dropped from the last 32-deep step of columns 16..31 (bf16x3)."""
    cases = [(i, c) for i, c in enumerate(P.LINEAR_SHAPES) if c[2] <= 64 and c[1] >= 32] + [(0, (65, 33, 36)), (0, (65, 130, 64))]
    assert len(cases) >= 8
    for i, (m, n, k) in cases:
        x, w, bias, r1, r2, relu = P.linear_inputs("lin", m, n, k, i)
        terms = P.split_terms(x, w, "bf16x3")
        terms[-1, 1, :, 16:32] = 0.0
        got = P.epilogue(P.accumulate(terms), bias, r1, r2, relu)
        assert _exceeds(got, P.linear_f64(x, w, bias, r1, r2, relu), P.linear_bound(x, w, bias, r1, r2, relu, 0, 1, "bf16x3")), (m, n, k)


@pytest.mark.parametrize("prec", P.PRECISIONS)
def test_mutation_ii_last_k_left_out_for_the_last_row_tile(prec):
    for i, (m, n, k) in enumerate(SHALLOW):
        x, w, bias, r1, r2, relu = P.linear_inputs("lin", m, n, k, i)
        xm = x.clone()
        xm[(m - 1) // 16 * 16:, k - 1] = 0.0
        got = P.emulate_linear(xm, w, bias, r1, r2, relu, 0, 1, prec)
        assert _exceeds(got, P.linear_f64(x, w, bias, r1, r2, relu), P.linear_bound(x, w, bias, r1, r2, relu, 0, 1, prec)), (m, n, k)


@pytest.mark.parametrize("prec", P.PRECISIONS)
def test_mutation_iii_bias_of_the_last_column_from_its_neighbour(prec):
    seen = 0
    for i, (m, n, k) in enumerate(SHALLOW):
        x, w, bias, r1, r2, relu = P.linear_inputs("lin", m, n, k, i)
        if bias is None or n < 2:
            continue
        bm = bias.clone()
        bm[n - 1] = bias[n - 2]
        got = P.emulate_linear(x, w, bm, r1, r2, relu, 0, 1, prec)
        assert _exceeds(got, P.linear_f64(x, w, bias, r1, r2, relu), P.linear_bound(x, w, bias, r1, r2, relu, 0, 1, prec)), (m, n, k)
        seen += 1
    assert seen >= 20


@pytest.mark.parametrize("prec", P.PRECISIONS)
def test_mutation_iv_res2_added_before_the_first_relu(prec):
    seen = 0
    for i, (m, n, k) in enumerate(SHALLOW):
        x, w, bias, r1, r2, relu = P.linear_inputs("lin", m, n, k, i)
        if r2 is None or not relu or m * n < 16:       # (a handful of elements may all have a positive pre-activation, where the two orders agree)
            continue
        acc = P.emulate_linear(x, w, None, None, None, False, 0, 1, prec)
        got = (acc + bias + r1 + r2).clamp_min(0).clamp_min(0)
        assert _exceeds(got, P.linear_f64(x, w, bias, r1, r2, relu), P.linear_bound(x, w, bias, r1, r2, relu, 0, 1, prec)), (m, n, k)
        seen += 1
    assert seen >= 4


@pytest.mark.parametrize("prec", P.PRECISIONS)
def test_mutation_v_row_shift_across_the_sequence_boundary(prec):
    for i, (m, seq, sh, n, k) in enumerate(P.CAUSAL_CASES):
        if k > 64:
            continue
        x, w, bias, r1, r2, relu = P.linear_inputs("cau", m, n, k, i)
        xs = x[(torch.arange(m) - sh) % m]               # x[m - a_shift] whatever m % a_seq is (wrapping at row 0)
        got = P.emulate_linear(xs, w, bias, r1, r2, relu, 0, 1, prec)
        assert _exceeds(got, P.linear_f64(x, w, bias, r1, r2, relu, sh, seq), P.linear_bound(x, w, bias, r1, r2, relu, sh, seq, prec)), (m, seq, sh, n, k)


def _attention_mutant(q, k, v, heads, mask, kind):
    """attention_f64 with one fault."""
    b, lq, d = q.shape
    lk = k.shape[1]
    s = (P._heads(q.double(), heads) / 8.0) @ P._heads(k.double(), heads).transpose(2, 3)
    vh = P._heads(v.double(), heads).clone()
    if mask is not None:
        rows = mask if mask.shape[1] > 1 else mask.expand(b, lq, lk)
        if kind == "vii":
            rows = rows[:, :1].expand(b, lq, lk)
        if kind == "ix":
            rows = rows[:, torch.arange(lq) % 16]
        s = s.masked_fill((rows == 0)[:, None], -1e9)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    den = e.sum(-1, keepdim=True) if kind != "vi" else e[..., :lk - 1].sum(-1, keepdim=True)
    p = e / den
    if kind == "viii":
        vh[:, :, lk - 1] = 0.0
    return (p @ vh).transpose(1, 2).reshape(b, lq, d), p


def _attention_mutation_seen(kind, lq, lk, mask_name, prec):
    q, k, v = P.attention_inputs(lq, lk, 2)
    mask = None if mask_name is None else P.attention_masks(lq, lk, q.shape[0])[mask_name]
    out, attn = _attention_mutant(q, k, v, 2, mask, kind)
    ro, ra = P.attention_f64(q, k, v, 2, mask)
    bo, ba = P.attention_bounds(q, k, v, 2, mask, prec)
    return max(P.sliced_errors(out, ro, bo, P.OUT_AXES)[2][0], P.sliced_errors(attn, ra, ba, P.ATTN_AXES)[2][0]) > 1.0


# plain bf16's bound (2^-7 per product, through the exponential) cannot see a fault of the order of one probability: the parity-grade modes must
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_mutations_vi_and_viii_last_key_left_out_of_the_sum_or_its_v_row_zero(prec):
    for lq, lk in P.ATT_SHAPES:
        if lk == 1:
            continue                                    # (a sum without its only key is no softmax at all)
        assert _attention_mutation_seen("vi", lq, lk, None, prec), (lq, lk)
        assert _attention_mutation_seen("viii", lq, lk, None, prec), (lq, lk)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_mutations_vii_and_ix_wrong_mask_row(prec):
    for lq, lk in P.ATT_MASK_SHAPES:
        if lq > 1:
            assert _attention_mutation_seen("vii", lq, lk, "causal", prec), (lq, lk)       # sq ignored: the mask row of query 0 for every query
        if lq > 16:
            assert _attention_mutation_seen("ix", lq, lk, "causal", prec), (lq, lk)        # q % 16 for min(q, Lq - 1)
    assert sum(lq > 16 for lq, _ in P.ATT_MASK_SHAPES) >= 3


# ---- c. the image slot map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", [(1, 4), (65, 36), (130, 68)])
def test_images_of_agrees_with_the_index_formula(m, k):
    x = P.T(f"img{m}x{k}", (m, k))
    xp = P.padded_k(x)
    assert torch.equal(P.images_of(xp), P.slot_map_by_formula(x, xp.shape[1]))


def test_case_lists_cover_what_they_name():
    ms, ns, ks = ({c[i] for c in P.LINEAR_SHAPES} for i in range(3))
    assert ms >= set(P.LIN_M) and ns >= set(P.LIN_N) and ks >= set(P.LIN_K)
    for m in P.LIN_M:
        assert len({c[1] for c in P.LINEAR_SHAPES if c[0] == m}) >= 2 and len({c[2] for c in P.LINEAR_SHAPES if c[0] == m}) >= 2, m
    for n in P.LIN_N:
        assert len({c[0] for c in P.LINEAR_SHAPES if c[1] == n}) >= 2, n
    for k in P.LIN_K:
        assert len({c[0] for c in P.LINEAR_SHAPES if c[2] == k}) >= 2, k
    assert 55 <= len(P.LINEAR_SHAPES) <= 70
    assert [P.splitk_slices(k, s) for (_, _, k, s) in P.SPLITK_CASES] == [(64, 2), (64, 3), (128, 2), (64, 4), (64, 2)]
    assert np.all([k % 32 == 0 for (_, _, k) in P.PRESPLIT_CASES])
