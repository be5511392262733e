"""The attention training pair on the GPU -- eg_attention_train (attention_mfma_kernel<F32, KT, DROP>) and eg_attention_backward_train
(attention_bwd_mfma_kernel<KT, QC, DROP>: KT = 3 / 4 with query chunks of 64, KT = 8 with chunks of 32) of csrc/attention.hip -- called through the C
ABI.  The backward takes P as an argument: dq, dk and dv are compared per ELEMENT with the float64 polynomial in (q, k, v, P, dO, M) of
tests/grads_f64.py within its a-priori bounds (derivation, case list with the route of each case there; tests/test_grads_f64.py shows on the CPU that
the bounds reject a row sum over a quarter of the keys, a mask on dV but not on dA, a query chunk missing from dK, a missing 1 / 8 and a key of the
last tile with its neighbour's mask).  P given: the fp32 rounding of a float64 softmax; P chained: the attn output of eg_attention_train on the
same inputs, as production does.  M is built on the CPU from oracle.dropout_keep_mask and cross-checked once against eg_dropout_dev.

q / k / v are read dense, as slices of one [rows, 3 D] buffer, or with k / v as slices of a [rows, 2 D] buffer (the two forms functional.py uses),
gaps holding NaN; dq / dk / dv are rows 1 .. of buffers with three different pitches (D + 1, D + 6, D + 4) filled with one NaN bit pattern, every
slot outside the result checked after the call."""
import pytest
import torch

import grads_f64 as G

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5
GUARD = 256
BAD_ARG, UNSUPPORTED, ALIGN = -1, -2, -5
B, H, D = G.ATB, G.ATH, G.ATD


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, _stream(dev())


def nan_rows(t, ld):
    buf = torch.full((t.shape[0], ld), float("nan"), device=dev())
    buf[:, :t.shape[1]] = t.to(dev())
    return buf


def operands(q, k, v, layout):
    """-> ((q view, ldq), (k view, ldk), (v view, ldv)) on the device."""
    lq, lk = q.shape[1], k.shape[1]
    q2, k2, v2 = q.reshape(B * lq, D), k.reshape(B * lk, D), v.reshape(B * lk, D)
    if layout == "dense":
        return tuple((t.to(dev()).contiguous(), D) for t in (q2, k2, v2))
    if layout == "qkv3":            # one projection output [rows, 3 D]: q | k | v column blocks (self-attention)
        buf = torch.cat([q2, k2, v2], dim=1).to(dev())
        return (buf, 3 * D), (buf[:, D:], 3 * D), (buf[:, 2 * D:], 3 * D)
    if layout == "kv2":             # q from its own projection (rows padded, the gap NaN), k | v from one [rows, 2 D] buffer (cross-attention)
        kv = torch.cat([k2, v2], dim=1).to(dev())
        return (nan_rows(q2, D + 8), D + 8), (kv, 2 * D), (kv[:, D:], 2 * D)
    raise ValueError(layout)


def canary2(rows, ld):
    buf = torch.full((rows + 2, ld), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[1:]


def result2(buf, rows, cols, shape, what):
    b = buf.cpu()
    out = b[1:rows + 1, :cols].clone()
    b[1:rows + 1, :cols] = SENTINEL
    bad = (b != SENTINEL).nonzero()
    assert bad.numel() == 0, f"{what}: stores outside the result, first at buffer row {int(bad[0, 0]) - 1}, column {int(bad[0, 1])}"
    return out.view(torch.float32).view(shape)


def run_backward(c, q, k, v, P, do, dense_out=False):
    """One eg_attention_backward_train call -> dq [B, Lq, D], dk, dv [B, Lk, D] (CPU), canaries checked."""
    L, lib, _ptr, st = _api()
    what = f"eg_attention_backward_train {c.lq}x{c.lk} KT {c.route[0]} QC {c.route[1]} p {c.p} {c.cls} {c.layout}"
    (qd, ldq), (kd, ldk), (vd, ldv) = operands(q, k, v, c.layout)
    ldo = D + 4
    dod = nan_rows(do.reshape(B * c.lq, D), ldo)
    Pd = P.to(dev()).contiguous()
    ldq_, ldk_, ldv_ = (D, D, D) if dense_out else (D + 1, D + 6, D + 4)
    qbuf, dq = canary2(B * c.lq, ldq_)
    kbuf, dk = canary2(B * c.lk, ldk_)
    vbuf, dv = canary2(B * c.lk, ldv_)
    L.check(lib.eg_attention_backward_train(_ptr(qd), ldq, _ptr(kd), ldk, _ptr(vd), ldv, _ptr(Pd), _ptr(dod), ldo, _ptr(dq), ldq_, _ptr(dk), ldk_,
                                            _ptr(dv), ldv_, B, H, c.lq, c.lk, 64, c.p, G.AT_SEED, c.offset, None, st), what)
    torch.cuda.synchronize()
    return (result2(qbuf, B * c.lq, D, (B, c.lq, D), what + " dq"), result2(kbuf, B * c.lk, D, (B, c.lk, D), what + " dk"),
            result2(vbuf, B * c.lk, D, (B, c.lk, D), what + " dv"), what)


def check_backward(c, q, k, v, P, do):
    M = G.att_mask(c.lq, c.lk, c.p, c.offset)
    ref, bound = G.att_backward_f64(q, k, v, P, do, M), G.att_backward_bounds(q, k, v, P, do, M)
    dq, dk, dv, what = run_backward(c, q, k, v, P, do)
    worst = {}
    for name, got, axes in (("dq", dq, G.DQ_AXES), ("dk", dk, G.DK_AXES), ("dv", dv, G.DK_AXES)):
        worst[name] = G.compare_sliced(got, ref[name], bound[name], f"{what} {name}", axes)[2]
        print(f"FRACTION eg_attention_backward_train {name} {worst[name]:.3f}")
    return dq, dk, dv


IDS = lambda cases: [f"{c.lq}x{c.lk}-p{c.p}-{c.cls}-{c.layout}" + ("-bigoffset" if c.offset > 1 << 32 else "") for c in cases]


@pytest.mark.parametrize("c", G.ATT_TRAIN_CASES, ids=IDS(G.ATT_TRAIN_CASES))
def test_attention_backward_with_p_given(c):
    """P = the fp32 rounding of the float64 softmax.  Two runs bitwise equal; dense output pitches give the same bits as the padded ones."""
    q, k, v, do = G.att_train_inputs(c.lq, c.lk, c.cls)
    P = G.att_softmax_f32(q, k)
    dq, dk, dv = check_backward(c, q, k, v, P, do)
    dq2, dk2, dv2, what = run_backward(c, q, k, v, P, do, dense_out=True)
    for a, b, name in ((dq, dq2, "dq"), (dk, dk2, "dk"), (dv, dv2, "dv")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: {name} depends on the output pitch or differs between two runs"


def run_forward(c, q, k, v):
    """eg_attention_train -> out [B, Lq, D], attn [B, H, Lq, Lk] (CPU), canaries checked."""
    L, lib, _ptr, st = _api()
    what = f"eg_attention_train {c.lq}x{c.lk} p {c.p} {c.layout}"
    (qd, ldq), (kd, ldk), (vd, ldv) = operands(q, k, v, c.layout)
    ldo = D + 4
    obuf, out = canary2(B * c.lq, ldo)
    n = B * H * c.lq * c.lk
    abuf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    L.check(lib.eg_attention_train(_ptr(qd), ldq, _ptr(kd), ldk, _ptr(vd), ldv, _ptr(out), ldo, _ptr(abuf[GUARD:]), B, H, c.lq, c.lk, 64, c.p,
                                   G.AT_SEED, c.offset, None, st), what)
    torch.cuda.synchronize()
    ab = abuf.cpu()
    assert bool((ab[:GUARD] == SENTINEL).all()) and bool((ab[GUARD + n:] == SENTINEL).all()), f"{what}: stores around attn"
    return result2(obuf, B * c.lq, D, (B, c.lq, D), what + " out"), ab[GUARD:GUARD + n].clone().view(torch.float32).view(B, H, c.lq, c.lk), what


@pytest.mark.parametrize("c", G.ATT_CHAINED_CASES, ids=IDS(G.ATT_CHAINED_CASES))
def test_attention_forward_with_dropout_and_backward_with_p_chained(c):
    """eg_attention_train with p > 0: `attn` holds the UNMASKED probabilities (attn_bound of products_f64), `out` = (P o M) V (its out-bound with
    A = P o M in place of P).  Then the backward on that very P, the reference taking it as its input."""
    q, k, v, do = G.att_train_inputs(c.lq, c.lk, c.cls)
    M = G.att_mask(c.lq, c.lk, c.p, c.offset)
    out, attn, what = run_forward(c, q, k, v)
    ro, ra, bo, ba = G.att_forward_f64(q, k, v, M)
    print(f"FRACTION eg_attention_train attn {G.compare_sliced(attn, ra, ba, what + ' attn', ('clip', 'head', 'query', 'key'))[2]:.3f}")
    print(f"FRACTION eg_attention_train out {G.compare_sliced(out, ro, bo, what + ' out', G.DQ_AXES)[2]:.3f}")
    check_backward(c, q, k, v, attn, do)


@pytest.mark.parametrize("c", [c for c in G.ATT_TRAIN_CASES if c.p > 0][::4], ids=lambda c: f"{c.lq}x{c.lk}-p{c.p}")
def test_attention_forward_with_dropout(c):
    """The forward alone at more (Lq, Lk, p) edges, the large offset among them."""
    q, k, v, _ = G.att_train_inputs(c.lq, c.lk, c.cls)
    out, attn, what = run_forward(c, q, k, v)
    ro, ra, bo, ba = G.att_forward_f64(q, k, v, G.att_mask(c.lq, c.lk, c.p, c.offset))
    print(f"FRACTION eg_attention_train attn {G.compare_sliced(attn, ra, ba, what + ' attn', ('clip', 'head', 'query', 'key'))[2]:.3f}")
    print(f"FRACTION eg_attention_train out {G.compare_sliced(out, ro, bo, what + ' out', G.DQ_AXES)[2]:.3f}")


@pytest.mark.parametrize("p,offset", [(0.1, 4096), (0.5, 4096), (0.1, (1 << 32) + 12345)])
def test_cpu_mask_is_the_library_mask(p, offset):
    """The reference's M (oracle.dropout_keep_mask, which the reference does not take from the library) against eg_dropout_dev on ones: bitwise."""
    L, lib, _ptr, st = _api()
    lq, lk = 33, 65
    n = B * H * lq * lk
    ones = torch.ones(n, device=dev())
    got = torch.empty_like(ones)
    L.check(lib.eg_dropout_dev(_ptr(ones), _ptr(got), n, p, G.AT_SEED, offset, None, st), "eg_dropout_dev")
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().double().view(B, H, lq, lk), G.att_mask(lq, lk, p, offset))


def test_attention_train_refusals_leave_the_outputs_untouched():
    """Lk = 129 and d_k = 32 -> EG_ERR_UNSUPPORTED; a pitch not a multiple of 4 and a misaligned base -> EG_ERR_ALIGN; p = 1 and (forward) a null attn
    -> EG_ERR_BAD_ARG; all before any launch."""
    L, lib, _ptr, st = _api()
    lq, lk_big = 17, 129
    q = torch.zeros(B * lq * (D + 8) + 4, device=dev())
    kv = torch.zeros(B * lk_big, D, device=dev())
    P = torch.zeros(B * H * lq * lk_big, device=dev())
    bufs = [torch.full((B * lk_big, D), SENTINEL, dtype=torch.int32, device=dev()) for _ in range(4)]
    o, dq, dk, dv = bufs
    abuf = torch.full((B * H * lq * lk_big,), SENTINEL, dtype=torch.int32, device=dev())

    def fwd(lk=49, dk_=64, ldq=D, qoff=0, p=0.1, attn=_ptr(abuf)):
        return lib.eg_attention_train(_ptr(q[qoff:]), ldq, _ptr(kv), D, _ptr(kv), D, _ptr(o), D, attn, B, H, lq, lk, dk_, p, 1, 0, None, st)

    def bwd(lk=49, dk_=64, ldq=D, qoff=0, p=0.1):
        return lib.eg_attention_backward_train(_ptr(q[qoff:]), ldq, _ptr(kv), D, _ptr(kv), D, _ptr(P), _ptr(q), D, _ptr(dq), D, _ptr(dk), D, _ptr(dv), D,
                                               B, H, lq, lk, dk_, p, 1, 0, None, st)

    for what, rcs, want in (("Lk = 129", (fwd(lk=lk_big), bwd(lk=lk_big)), UNSUPPORTED), ("d_k = 32", (fwd(dk_=32), bwd(dk_=32)), UNSUPPORTED),
                            ("ldq = D + 2", (fwd(ldq=D + 2), bwd(ldq=D + 2)), ALIGN), ("q one float off", (fwd(qoff=1), bwd(qoff=1)), ALIGN),
                            ("p = 1", (fwd(p=1.0), bwd(p=1.0)), BAD_ARG), ("attn = NULL", (fwd(attn=None),), BAD_ARG)):
        assert all(rc == want for rc in rcs), f"{what}: status {rcs}, expected {want} ({lib.eg_last_error().decode()})"
        torch.cuda.synchronize()
        assert all(bool((b == SENTINEL).all()) for b in bufs + [abuf]), f"{what}: something was written"
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
