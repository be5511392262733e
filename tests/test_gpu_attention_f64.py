"""ScaledDotProductAttention of csrc/attention.hip on the GPU -- eg_attention and eg_attention_masked, attention_mfma_kernel<PREC, KT> in its four
key-tile instantiations -- called through the C ABI: every element of `out` and of `attn` against the float64 restatement of
tests/products_f64.py within its a-priori bound (reference, bounds, case lists and input classes are there; tests/test_products_f64.py shows on the CPU
that the bounds reject a key missing from the softmax sum, a zero V row and a wrong mask row).

`out` is rows 1 .. B Lq of a [B Lq + 2, D + 4] buffer and `attn` the middle of a longer one, both filled with one NaN bit pattern: after a call every
slot outside the result -- the guard rows, columns D .. D + 3 of every out row, the slots around attn -- must still hold it.  q, k and v are read
dense and strided (one packed [B L, 3 D] buffer as the generator holds them where Lq == Lk, else rows padded to D + 8), the gaps holding NaN."""
import pytest
import torch

import products_f64 as P

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5
GUARD = 256


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _api():
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    return L, L.load(), _ptr, _stream(dev())


def operands(q, k, v, layout):
    """-> ((q view, ldq), (k view, ldk), (v view, ldv)) on the device; the views' first element is the pointer to pass."""
    b, lq, d = q.shape
    lk = k.shape[1]
    q2, k2, v2 = q.reshape(b * lq, d), k.reshape(b * lk, d), v.reshape(b * lk, d)
    if layout == "dense":
        return tuple((t.to(dev()).contiguous(), d) for t in (q2, k2, v2))
    if lq == lk:                # one packed buffer [B L, 3 D]: q | k | v column blocks
        buf = torch.empty(b * lq, 3 * d, device=dev())
        buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:] = q2.to(dev()), k2.to(dev()), v2.to(dev())
        return (buf, 3 * d), (buf[:, d:], 3 * d), (buf[:, 2 * d:], 3 * d)
    out = []
    for t in (q2, k2, v2):
        buf = torch.full((t.shape[0], d + 8), float("nan"), device=dev())
        buf[:, :d] = t.to(dev())
        out.append((buf, d + 8))
    return tuple(out)


def run_attention(q, k, v, heads, prec, layout="dense", mask=None, want_attn=True, what=""):
    """One call -> (rc, out [B, Lq, D], attn [B, H, Lq, Lk] or None) on the CPU, canaries checked.  mask: None or (device bytes, sb, sq)."""
    L, lib, _ptr, st = _api()
    b, lq, d = q.shape
    lk = k.shape[1]
    (qd, ldq), (kd, ldk), (vd, ldv) = operands(q, k, v, layout)
    ldo = d + 4
    obuf = torch.full((b * lq + 2, ldo), SENTINEL, dtype=torch.int32, device=dev())
    n_attn = b * heads * lq * lk
    abuf = torch.full((GUARD + n_attn + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    out_p = _ptr(obuf[1:])
    attn_p = _ptr(abuf[GUARD:]) if want_attn else None
    code = L.precision_code(prec)
    if mask is None:
        rc = lib.eg_attention(_ptr(qd), ldq, _ptr(kd), ldk, _ptr(vd), ldv, out_p, ldo, attn_p, b, heads, lq, lk, 64, code, st)
    else:
        mb, sb, sq = mask
        rc = lib.eg_attention_masked(_ptr(qd), ldq, _ptr(kd), ldk, _ptr(vd), ldv, _ptr(mb), sb, sq, out_p, ldo, attn_p, b, heads, lq, lk, 64, code, st)
    L.check(rc, what)
    torch.cuda.synchronize()
    ob, ab = obuf.cpu(), abuf.cpu()
    out = ob[1:b * lq + 1, :d].contiguous().view(torch.float32).view(b, lq, d)
    ob[1:b * lq + 1, :d] = SENTINEL
    bad = (ob != SENTINEL).nonzero()
    assert bad.numel() == 0, f"{what}: stores outside out, first at buffer row {int(bad[0, 0]) - 1}, column {int(bad[0, 1])}"
    attn = None
    if want_attn:
        assert bool((ab[:GUARD] == SENTINEL).all()) and bool((ab[-GUARD:] == SENTINEL).all()), f"{what}: stores around attn"
        attn = ab[GUARD:GUARD + n_attn].view(torch.float32).view(b, heads, lq, lk)
    else:
        assert bool((ab == SENTINEL).all()), f"{what}: attn written without being asked for"
    return out, attn


def check_attention(q, k, v, heads, prec, what, mask_bytes=None, mask_arg=None, layouts=("dense", "strided")):
    """Both layouts against the float64 reference; row sums; the call without attn.  -> (worst element fraction, out, attn of the dense call)."""
    lk = k.shape[1]
    ro, ra = P.attention_f64(q, k, v, heads, mask_bytes)
    bo, ba = P.attention_bounds(q, k, v, heads, mask_bytes, prec)
    worst, first = 0.0, None
    for layout in layouts:
        w = f"{what} {prec} {layout}"
        out, attn = run_attention(q, k, v, heads, prec, layout, mask_arg, True, w)
        worst = max(worst, P.compare_sliced(out, ro, bo, w + " out", P.OUT_AXES)[2], P.compare_sliced(attn, ra, ba, w + " attn", P.ATTN_AXES)[2])
        dev_sum = float((attn.double().sum(-1) - 1.0).abs().max())
        assert dev_sum <= (lk + 8) * P.U, f"{w}: a row of attn sums to 1 +- {dev_sum:.3g}"
        out2, _ = run_attention(q, k, v, heads, prec, layout, mask_arg, False, w + " (no attn)")
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), f"{w}: out differs without the attn output"
        first = first or (out, attn)
    return worst, first[0], first[1]


def report(entry, prec, worst):
    print(f"FRACTION {entry} {prec} {worst:.3f}")


# ---- eg_attention -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", P.PRECISIONS)
@pytest.mark.parametrize("lq,lk", P.ATT_SHAPES)
def test_attention_matches_float64_per_element(lq, lk, prec):
    """launch_att_kt: Lk <= 48 -> KT = 3 (bf16 modes pair the last key tile with zeros), <= 64 -> 4, <= 128 -> 8, else 16; ceil(Lq / 64) workgroups per
    (head, clip), one wave per 16-query tile, ragged tiles on both axes.  heads 1 and 2, uniform q, k in (-2, 2)."""
    worst = 0.0
    for heads in P.ATT_HEADS:
        q, k, v = P.attention_inputs(lq, lk, heads)
        worst = max(worst, check_attention(q, k, v, heads, prec, f"eg_attention {lq}x{lk} h{heads}")[0])
    report("eg_attention", prec, worst)


@pytest.mark.parametrize("prec", P.PRECISIONS)
@pytest.mark.parametrize("cls", ["peaked", "flat"])
@pytest.mark.parametrize("lq,lk", P.ATT_CLASS_SHAPES)
def test_attention_input_classes(lq, lk, cls, prec):
    """peaked: one score per row leads by >= 60 -- the softmax is one-hot, exp underflows elsewhere; flat: k = 0 -- attn is 1 / Lk and out the mean
    of v, to the roundings of the sum alone (the bound has no score term left)."""
    q, k, v = P.attention_inputs(lq, lk, 2, cls)
    worst, out, attn = check_attention(q, k, v, 2, prec, f"eg_attention {lq}x{lk} {cls}")
    if cls == "peaked":
        pick = (7 * torch.arange(lq) + 3) % lk
        assert bool((attn.argmax(-1) == pick).all()) and float(attn.max(-1).values.min()) >= 1.0 - (lk + 8) * P.U
    report(f"eg_attention[{cls}]", prec, worst)


# ---- eg_attention_masked ------------------------------------------------------------------------------------------------------------------------
def mask_arg(mask, pad=0, batch_gap=0, fill=0):
    """mask bytes [B, 1 or Lq, Lk] (CPU) -> (device bytes, sb, sq) with rows padded by `pad` bytes and clips by `batch_gap` more, gaps = fill."""
    b, rows, lk = mask.shape
    sq = lk + pad
    sb = rows * sq + batch_gap
    buf = torch.full((b, sb), fill, dtype=torch.uint8)
    buf[:, :rows * sq].view(b, rows, sq)[:, :, :lk] = mask
    return buf.to(dev()), sb, (sq if rows > 1 else 0)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("lq,lk", P.ATT_MASK_SHAPES)
def test_attention_masked(lq, lk, prec):
    """eg_attention_masked against attention_f64 with the mask: a padding mask (sq = 0), a per-query causal mask (sq = Lk), fully masked rows --
    among them the last query, whose tile is ragged at 17 and 65 queries and whose mask row the kernel's min(q, Lq - 1) clamp also serves to the
    lanes behind it -- and the all-ones mask, bitwise the unmasked call.  The causal mask again with sq = Lk + 7 and sb > Lq sq, the gap bytes 0
    and then 1: bitwise the same result."""
    heads = 2
    q, k, v = P.attention_inputs(lq, lk, heads)
    masks = P.attention_masks(lq, lk, q.shape[0])
    worst, res = 0.0, {}
    for name, m in masks.items():
        w, out, attn = check_attention(q, k, v, heads, prec, f"eg_attention_masked {lq}x{lk} {name}", m, mask_arg(m))
        worst, res[name] = max(worst, w), (out, attn)
    out0, attn0 = run_attention(q, k, v, heads, prec, "dense", None, True, "unmasked")
    assert torch.equal(res["ones"][0], out0) and torch.equal(res["ones"][1], attn0), "the all-ones mask differs from the unmasked call"
    for fill in (0, 1):
        out, attn = run_attention(q, k, v, heads, prec, "dense", mask_arg(masks["causal"], 7, 13, fill), True, f"padded mask rows, gaps {fill}")
        assert torch.equal(out, res["causal"][0]) and torch.equal(attn, res["causal"][1]), f"gap bytes {fill} of a padded mask change the result"
    dead = res["dead_rows"][1][:, :, lq - 1]
    assert float((dead.double() - 1.0 / lk).abs().max()) <= (lk + 8) * P.U / lk
    report("eg_attention_masked", prec, worst)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_attention_refusals_leave_the_output_untouched():
    """Lk = 257 and d_k = 32 -> EG_ERR_UNSUPPORTED, ldq = D + 2 -> EG_ERR_ALIGN, mask_query_stride = Lk - 1 -> EG_ERR_BAD_ARG: each refused on the host
    before any launch (include/emogest.h), the sentinel-filled out untouched."""
    L, lib, _ptr, st = _api()
    b, heads, lq, d = 1, 2, 17, 128
    lk_big = 257
    q = torch.zeros(b * lq, d + 8, device=dev())
    kv = torch.zeros(b * lk_big, d, device=dev())
    mask = torch.ones(b * lq * lk_big, dtype=torch.uint8, device=dev())
    out = torch.full((b * lq, d), SENTINEL, dtype=torch.int32, device=dev())
    code = L.precision_code("bf16x3")

    def plain(lk=49, dk=64, ldq=d):
        return lib.eg_attention(_ptr(q), ldq, _ptr(kv), d, _ptr(kv), d, _ptr(out), d, None, b, heads, lq, lk, dk, code, st)

    def masked(lk=49, dk=64, ldq=d, sq=49):
        return lib.eg_attention_masked(_ptr(q), ldq, _ptr(kv), d, _ptr(kv), d, _ptr(mask), lq * lk_big, sq, _ptr(out), d, None, b, heads, lq, lk, dk, code, st)

    UNSUPPORTED, ALIGN, BAD_ARG = -2, -5, -1
    for what, rc, want in (("Lk = 257", plain(lk=lk_big), UNSUPPORTED), ("Lk = 257, masked", masked(lk=lk_big, sq=lk_big), UNSUPPORTED),
                           ("d_k = 32", plain(dk=32), UNSUPPORTED), ("d_k = 32, masked", masked(dk=32), UNSUPPORTED),
                           ("ldq = D + 2", plain(ldq=d + 2), ALIGN), ("ldq = D + 2, masked", masked(ldq=d + 2), ALIGN),
                           ("mask_query_stride = Lk - 1", masked(sq=48), BAD_ARG)):
        assert rc == want, f"{what}: status {rc}, expected {want} ({lib.eg_last_error().decode()})"
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), f"{what}: out was written"
    assert plain() == 0 and masked() == 0           # the same buffers are accepted once the argument is right
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.view(torch.float32)).all())
