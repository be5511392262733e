"""Test-side float64 restatements of the linear family (csrc/gemm.hip: eg_linear, eg_linear_splitk, eg_split_tiles, eg_linear_presplit) and of
ScaledDotProductAttention (csrc/attention.hip: eg_attention, eg_attention_masked), the a-priori bounds every output ELEMENT is held to, the case
lists of the GPU tests, and CPU emulations of the split-bf16 arithmetic that show the bounds are neither violated by correct arithmetic nor
vacuous (tests/test_products_f64.py).  A helper module (not collected: no test_ prefix); CPU only, it imports nothing that touches a GPU.
compare_sliced, T, U, split_bf16, images_of and image_rows are those of tests/small_ops_f64.py.

Linear reference.  linear_f64 is the epilogue of include/emogest.h step by step in float64:
    acc[m, n] = sum_k X[src(m), k] W[n, k],   src(m) = m - a_shift, the row taken as zero where (m % a_seq) < a_shift
    v = acc + bias[n] + res1[m, n];   if relu: v = max(v, 0);   if res2: v = max(v + res2[m, n], 0)

Linear bound, per output element, nothing measured.  With S = sum_k |x||w| and mag = |bias| + S + |res1| + |res2|:
    bound = (E_prec + (K + 8) 2^-24) S + 4 2^-24 mag + 2^-24 |ref|
  * (K + 8) 2^-24 S: K additions into an fp32 accumulator whose partial sums are at most S, in ANY order (tile choice, the K steps dealt over the
    waves of the skinny kernel, split-K and its fold only permute the additions and add at most 4 more: the + 8);
  * 4 2^-24 mag: the bias, res1 and res2 additions of the epilogue, each a rounding of a value of at most mag;
  * 2^-24 |ref|: the rounding of the stored value.  ReLU is 1-Lipschitz: it does not enlarge an error.
  * E_prec, the representation error of one product, with u = 2^-8 (bf16 has 8 significant bits: |x - hi| <= u |x|, and since lo = bf16(x - hi),
    |lo| <= u |x| and the residual r = x - hi - lo has |r| <= u^2 |x|):
      f32     0: v_mfma_f32_16x16x4_f32 multiplies fp32 values exactly.
      bf16x3  x w - (xh wh + xh wl + xl wh) = xl wl + rx w + x rw - rx rw, so |.| <= (u^2 + u^2 + u^2 + u^4) |x||w|:  E = 3 2^-16 + 2^-32.
      bf16    x w - xh wh = (x - xh) w + xh (w - wh), so |.| <= (u + (1 + u) u) |x||w|:                                E = 2 2^-8 + 2^-16.
    (A bf16 x bf16 product has 16 significant bits and is exact in fp32.)

Attention reference.  attention_f64 is Full_model/Modules.py:13-23 in float64: q / 8 first, masked_fill(mask == 0, -1e9) with the literal, softmax
over the keys, then P V; a fully masked row softmaxes to uniform.

Attention bounds, the same way.  Per score, the linear bound with K = 64 on (q / 8) . k (mag = S_s = sum_d |q_d / 8||k_d|, no epilogue operands) plus one
rounding of the pre-scale:
    ds = (E_prec + 72 2^-24) S_s + 4 2^-24 S_s + 2^-24 |s| + 2^-24 S_s;          ds = 0 at a masked score (both sides hold the literal -1e9)
  * attn_bound = p (2 max_row ds + (Lk + 8) 2^-24) + 2^-126.  Scores off by at most d = max_row ds move exp(s_j - m) / sum_i exp(s_i - m) by a factor
    within exp(+-2 d), 2 d to first order (the form the bound is stated in; at the scores of these tests 2 d <= 0.05 in bf16x3 and the factor
    (exp(2 d) - 1) / 2 d is below 1.03, far inside the slack between a worst-case and an observed rounding error; plain bf16's 2 d reaches the order
    of 1, where its bound says little -- bf16 is not the parity-grade mode); the rounding of s - m and of expf are below 2^-24 (2 |s| + 2) <= ds; the
    row sum, the reciprocal and the product add (Lk + 8) 2^-24.  2^-126 is the smallest normal fp32: below it a probability may be flushed to zero
    (the "peaked" inputs put most probabilities there).  A fully masked row has equal scores, ds = 0: 1 / Lk up to (Lk + 8) 2^-24.
  * out_bound = sum_j attn_bound_j |v_j| + (E_prec + (Lk + 8) 2^-24) sum_j p_j |v_j| + 2^-24 |out|: the error of P carried through the second
    product, plus the linear bound of that product (K = Lk) on the true P.

Emulations (CPU checks only).  emulate_linear / emulate_attention split both operands with split_bf16 exactly as the kernels do, form the products
of a 32-deep K step in float64 (they are exact in fp32 and the matrix pipe adds them with at most the roundings the bound already counts) and round
the accumulator to fp32 once per step; the epilogue and the softmax run in fp32.  The f32 mode is torch's own float32 CPU arithmetic.

Worst element of correct arithmetic as a fraction of its bound, re-measured by tests/test_products_f64.py over every case list below (it holds each
to at most 0.5; the issue's own figures, 0.06 / 0.26 at 65 x 33 x 36 and 65 x 130 x 64, are the deep shapes -- the worst here are the K = 4 ones):
    linear     f32 0.24     bf16x3 0.26     bf16 0.30
    attention  f32 0.03     bf16x3 0.16     bf16 0.43      (the worse of out and attn)
Plain bf16 at K = 4 is outside that list: E_bf16 is attained when the half-ulp errors of both operands align in each of only four products, and
correct arithmetic reaches 0.54 - 0.67 of the bound at the six K = 4 shapes.  There the CPU check asks instead that the error stay inside the
representation part E_bf16 S alone, which leaves every order-dependent term of the bound to the kernel.
"""
import numpy as np
import torch

from small_ops_f64 import T, U, compare_sliced, image_rows, images_of, sliced_errors, split_bf16  # noqa: F401  (re-exported for the tests)

PRECISIONS = ("f32", "bf16x3", "bf16")
UB = 2.0 ** -8                  # bf16: 8 significant bits
E_PREC = {"f32": 0.0, "bf16x3": 3 * UB ** 2 + UB ** 4, "bf16": 2 * UB + UB ** 2}
FLT_MIN = 2.0 ** -126
LIN_AXES = ("row", "column")
OUT_AXES = ("clip", "query", "column")
ATTN_AXES = ("clip", "head", "query", "key")


# ---- linear: reference, bound ----------------------------------------------------------------------------------------------------------
def shift_rows(x, a_shift, a_seq):
    """The causal row shift: row m reads row m - a_shift, zero where (m % a_seq) < a_shift."""
    if not a_shift:
        return x
    m = torch.arange(x.shape[0])
    ok = (m % a_seq) >= a_shift
    xs = torch.zeros_like(x)
    xs[ok] = x[m[ok] - a_shift]
    return xs


def epilogue(acc, bias=None, res1=None, res2=None, relu=False):
    """include/emogest.h in acc's dtype: v = acc + bias + res1; relu; then max(v + res2, 0) when res2 is given."""
    v = acc
    if bias is not None:
        v = v + bias.to(v.dtype)
    if res1 is not None:
        v = v + res1.to(v.dtype)
    if relu:
        v = v.clamp_min(0)
    if res2 is not None:
        v = (v + res2.to(v.dtype)).clamp_min(0)
    return v


def linear_f64(x, w, bias=None, res1=None, res2=None, relu=False, a_shift=0, a_seq=1):
    return epilogue(shift_rows(x, a_shift, a_seq).double() @ w.double().T, bias, res1, res2, relu)


def linear_bound(x, w, bias=None, res1=None, res2=None, relu=False, a_shift=0, a_seq=1, precision="f32"):
    K = x.shape[1]
    S = shift_rows(x, a_shift, a_seq).double().abs() @ w.double().abs().T
    mag = S.clone()
    for t in (bias, res1, res2):
        if t is not None:
            mag = mag + t.double().abs()
    ref = linear_f64(x, w, bias, res1, res2, relu, a_shift, a_seq)
    return (E_PREC[precision] + (K + 8) * U) * S + 4 * U * mag + U * ref.abs()


# ---- linear: emulation of the split arithmetic ---------------------------------------------------------------------------------------------
def _bf(bits):
    return bits.view(torch.bfloat16).double()


def split_terms(x, w, precision):
    """-> P [steps, 3, M, N] float64: per 32-deep K step the three product sums (x_hi w_hi, x_hi w_lo, x_lo w_hi) of the kernels' MFMA triple.
    bf16: the first only; f32: the exact fp32 products in the first."""
    M, K = x.shape
    N = w.shape[0]
    steps = (K + 31) // 32
    xp, wp = torch.zeros(M, steps * 32), torch.zeros(N, steps * 32)
    xp[:, :K], wp[:, :K] = x.float(), w.float()
    if precision == "f32":
        xh, wh, xl, wl = xp.double(), wp.double(), None, None
    else:
        (xhb, xlb), (whb, wlb) = split_bf16(xp), split_bf16(wp)
        xh, wh = _bf(xhb), _bf(whb)
        xl, wl = (_bf(xlb), _bf(wlb)) if precision == "bf16x3" else (None, None)
    P = torch.zeros(steps, 3, M, N, dtype=torch.float64)
    for s in range(steps):
        k = slice(32 * s, 32 * s + 32)
        P[s, 0] = xh[:, k] @ wh[:, k].T
        if xl is not None:
            P[s, 1] = xh[:, k] @ wl[:, k].T
            P[s, 2] = xl[:, k] @ wh[:, k].T
    return P


def accumulate(P):
    """The fp32 accumulator: rounded once per 32-deep step."""
    acc = torch.zeros(P.shape[2], P.shape[3], dtype=torch.float32)
    for s in range(P.shape[0]):
        acc = (acc.double() + P[s].sum(0)).float()
    return acc


def emulate_linear(x, w, bias=None, res1=None, res2=None, relu=False, a_shift=0, a_seq=1, precision="bf16x3"):
    xs = shift_rows(x, a_shift, a_seq)
    if precision == "f32":
        acc = torch.nn.functional.linear(xs.float(), w.float())
    else:
        acc = accumulate(split_terms(xs, w, precision))
    return epilogue(acc, bias, res1, res2, relu)


# ---- linear: cases -----------------------------------------------------------------------------------------------------------------------
LIN_M = (1, 15, 16, 17, 33, 48, 49, 63, 64, 65, 129)       # 64 / 65: both sides of SKINNY_ROWS; 16 / 17 / 33 / 49 select RT = 1 .. 4
LIN_N = (1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130)
LIN_K = (4, 28, 32, 36, 64, 68, 128, 132)
# epilogue options: (bias, res1, relu, res2)
OPTIONS = ((0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 1, 1, 1), (0, 0, 0, 1))


def linear_shapes():
    """Every M with two N and two K, every N with two M, every K with two M (not the full product), plus the two shapes the issue quotes figures
    for; duplicates removed, order fixed."""
    nm, nn, nk = len(LIN_M), len(LIN_N), len(LIN_K)
    s = []
    for i, m in enumerate(LIN_M):
        s += [(m, LIN_N[(2 * i) % nn], LIN_K[i % nk]), (m, LIN_N[(2 * i + 7) % nn], LIN_K[(i + 3) % nk])]
    for j, n in enumerate(LIN_N):
        s += [(LIN_M[j % nm], n, LIN_K[(j + 1) % nk]), (LIN_M[(j + 5) % nm], n, LIN_K[(j + 4) % nk])]
    for l, k in enumerate(LIN_K):
        s += [(LIN_M[(3 * l) % nm], LIN_N[(5 * l + 2) % nn], k), (LIN_M[(3 * l + 6) % nm], LIN_N[(5 * l + 9) % nn], k)]
    s += [(65, 33, 36), (65, 130, 64)]
    return list(dict.fromkeys(s))


LINEAR_SHAPES = linear_shapes()
# (M, a_seq, a_shift); the last one makes every row zero-sourced: the output is the epilogue of 0
CAUSAL_CASES = [(m, seq, sh, n, k) for (m, seq, sh) in ((60, 60, 1), (68, 34, 4), (130, 65, 64), (34, 34, 33), (20, 5, 5)) for n in (17, 64) for k in (36, 128)]
# (M, N, K, splits): (6, 17, 132, 2) has a short last slice; (3, 8, 68, 34) asks for more splits than there are 64-deep slices
SPLITK_CASES = [(6, 64, 128, 2), (6, 65, 192, 3), (6, 17, 132, 2), (65, 33, 256, 4), (3, 8, 68, 34)]
SPLIT_TILES_CASES = [(1, 4), (63, 28), (64, 64), (65, 36), (130, 68), (129, 132)]
# K walks past one and two ring turns of both pre-split kernels' LDS slots (4 x 32 and 3 x 32 deep)
PRESPLIT_CASES = [(64, 64, 32), (65, 65, 64), (129, 130, 96), (130, 17, 128), (200, 192, 160), (70, 129, 192), (257, 130, 256), (66, 66, 448)]


def splitk_slices(k, splits):
    """-> (k_per_split, nsplit) as launch_splitk derives them (csrc/gemm.hip): slices are rounded up to 64."""
    per = ((k + splits - 1) // splits + 63) // 64 * 64
    return per, (k + per - 1) // per


def layouts(n, k):
    """(name, lda, ldr, ldc): dense; every stride padded, ldc odd (the scalar-store branch with a full quad); ldc = N + 4 where the 16-byte store
    then runs next to a gap."""
    out = [("dense", k, n, n), ("strided", k + 4, n + 3, n + 5)]
    if n % 4 == 0:
        out.append(("gap4", k, n, n + 4))
    return out


def linear_weight(n, k):
    """One weight per (N, K): (-1, 1) / sqrt(K)."""
    return T(f"lw{n}x{k}", (n, k)) / float(np.sqrt(k))


def linear_inputs(key, m, n, k, option):
    """-> x, w, bias, res1, res2, relu for one case and one epilogue option (index into OPTIONS)."""
    hb, h1, relu, h2 = OPTIONS[option % len(OPTIONS)]
    key = f"{key}.{m}x{n}x{k}"
    return (T(key + "x", (m, k)), linear_weight(n, k), T(key + "b", (n,)) if hb else None, T(key + "r1", (m, n)) if h1 else None,
            T(key + "r2", (m, n)) if h2 else None, bool(relu))


def slot_map_by_formula(x, kpad):
    """The eg_split_tiles layout restated from the index formula of include/emogest.h element by element (independent of images_of's
    view / permute): images [2][ceil(M/64)][Kpad/8][64][8] int16, element (m, k) of image i at [i][m // 64][k // 8][m % 64][k % 8], zero elsewhere."""
    m_rows, k_cols = x.shape
    mt, ko = (m_rows + 63) // 64, kpad // 8
    hi, lo = split_bf16(x)
    out = np.zeros(2 * mt * ko * 64 * 8, dtype=np.int16)
    hi, lo = hi.numpy(), lo.numpy()
    for m in range(m_rows):
        for k in range(k_cols):
            slot = (((m // 64) * ko + k // 8) * 64 + m % 64) * 8 + k % 8
            out[slot] = hi[m, k]
            out[mt * ko * 512 + slot] = lo[m, k]
    return torch.from_numpy(out).view(2, mt, ko, 64, 8)


def padded_k(x):
    """x [M, K] zero padded along K to the next multiple of 64 (what images_of wants)."""
    m, k = x.shape
    out = torch.zeros(m, (k + 63) // 64 * 64)
    out[:, :k] = x
    return out


# ---- attention: reference, bounds ------------------------------------------------------------------------------------------------------
def _heads(t, heads):
    b, l, d = t.shape
    return t.reshape(b, l, heads, d // heads).transpose(1, 2)          # [B, H, L, 64]


def _mask4(mask):
    """mask bytes [B, 1 or Lq, Lk] -> bool [B, 1, 1 or Lq, Lk], True = masked."""
    return (mask == 0)[:, None]


def attention_f64(q, k, v, heads, mask=None):
    """-> (out [B, Lq, D], attn [B, H, Lq, Lk]) in float64 (Full_model/Modules.py:13-23)."""
    b, lq, d = q.shape
    s = (_heads(q.double(), heads) / 8.0) @ _heads(k.double(), heads).transpose(2, 3)
    if mask is not None:
        s = s.masked_fill(_mask4(mask), -1e9)
    p = torch.softmax(s, dim=-1)
    return (p @ _heads(v.double(), heads)).transpose(1, 2).reshape(b, lq, d), p


def attention_bounds(q, k, v, heads, mask=None, precision="f32"):
    """-> (out_bound [B, Lq, D], attn_bound [B, H, Lq, Lk]); see the module docstring."""
    b, lq, d = q.shape
    lk = k.shape[1]
    E = E_PREC[precision]
    qh, kh, vh = _heads(q.double(), heads) / 8.0, _heads(k.double(), heads), _heads(v.double(), heads)
    s = qh @ kh.transpose(2, 3)
    Ss = qh.abs() @ kh.abs().transpose(2, 3)
    ds = (E + (64 + 8) * U) * Ss + 4 * U * Ss + U * s.abs() + U * Ss
    if mask is not None:
        ds = ds.masked_fill(_mask4(mask).expand_as(ds), 0.0)
    out, p = attention_f64(q, k, v, heads, mask)
    attn_bound = p * (2 * ds.max(dim=-1, keepdim=True).values + (lk + 8) * U) + FLT_MIN
    ob = attn_bound @ vh.abs() + (E + (lk + 8) * U) * (p @ vh.abs())
    return ob.transpose(1, 2).reshape(b, lq, d) + U * out.abs(), attn_bound


def emulate_attention(q, k, v, heads, mask=None, precision="bf16x3"):
    """The kernel's data flow on the CPU: scores by the split product of (q * 0.125, fp32) with k, the literal -1e9, an fp32 softmax (max, exp, sum,
    one reciprocal), P V by the split product.  f32: torch's own float32 arithmetic."""
    b, lq, d = q.shape
    lk = k.shape[1]
    qh, kh, vh = _heads(q.float(), heads) * 0.125, _heads(k.float(), heads), _heads(v.float(), heads)
    out = torch.zeros(b, heads, lq, d // heads)
    attn = torch.zeros(b, heads, lq, lk)
    for i in range(b):
        for h in range(heads):
            s = qh[i, h] @ kh[i, h].T if precision == "f32" else accumulate(split_terms(qh[i, h], kh[i, h], precision))
            if mask is not None:
                s = s.masked_fill(mask[i] == 0, -1.0e9)
            e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
            p = e * (1.0 / e.sum(dim=-1, keepdim=True))
            attn[i, h] = p
            out[i, h] = p @ vh[i, h] if precision == "f32" else accumulate(split_terms(p, vh[i, h].T.contiguous(), precision))
    return out.transpose(1, 2).reshape(b, lq, d), attn


# ---- attention: cases ----------------------------------------------------------------------------------------------------------------------
# (Lq, Lk): Lk on both sides of 16 / 48 / 64 / 128 / 256 (KT = 3 / 4 / 8 / 16, the odd KT = 3 pairing its last key tile with zeros); Lq on both sides
# of the 16-query tile and the ATT_QC = 64 chunk; the workload's own lengths
ATT_SHAPES = ([(17, lk) for lk in (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256)]
              + [(lq, 49) for lq in (1, 15, 16, 17, 63, 64, 65, 129) if lq != 17] + [(60, 60), (34, 34), (120, 120)])
ATT_CLASS_SHAPES = [(17, 49), (65, 65), (64, 129)]
ATT_MASK_SHAPES = [(17, 49), (65, 65), (16, 48), (1, 1), (34, 130)]
ATT_HEADS = (1, 2)
PEAK_LEAD = 60.0


def att_batch(lk):
    return 1 if lk >= 255 else 2


def attention_inputs(lq, lk, heads, cls="uniform"):
    """-> q [B, Lq, D], k, v [B, Lk, D].  uniform: q, k in (-2, 2); peaked: every query is 32 x one key of its head (key (7 i + 3) % Lk for query
    i), so that key's score leads the row by >= PEAK_LEAD, the softmax is one-hot and exp underflows elsewhere; flat: k = 0, attn = 1 / Lk, out =
    the mean of v."""
    b, d = att_batch(lk), heads * 64
    key = f"att{lq}x{lk}h{heads}"
    q, k, v = T(key + "q", (b, lq, d), -2, 2), T(key + "k", (b, lk, d), -2, 2), T(key + "v", (b, lk, d))
    if cls == "flat":
        k = torch.zeros_like(k)
    elif cls == "peaked":
        pick = (7 * torch.arange(lq) + 3) % lk
        q = 32.0 * k[:, pick]
    elif cls != "uniform":
        raise ValueError(cls)
    return q, k, v


def attention_masks(lq, lk, b):
    """-> {name: mask bytes [B, 1 or Lq, Lk]} (0 = masked): a padding mask (one key row per clip), a per-query causal mask, a mask with fully masked
    rows (query 0 and the last query -- query 16 of 17: the last row of a ragged 16-row tile) and the all-ones mask."""
    j, i = torch.arange(lk)[None, None, :], torch.arange(lq)[None, :, None]
    pad = torch.tensor([min(lk - 1, 3 * c + 1) for c in range(b)])[:, None, None]
    causal = (j <= i).expand(b, lq, lk).clone()
    dead = causal.clone()
    dead[:, 0] = False
    dead[:, lq - 1] = False
    if b > 1:
        dead[1, lq // 2] = False
    return {"padding": (j < lk - pad).to(torch.uint8).contiguous(), "causal": causal.to(torch.uint8), "dead_rows": dead.to(torch.uint8),
            "ones": torch.ones(b, lq, lk, dtype=torch.uint8)}
