"""Test-side float64 restatements of the training backward kernels outside the audio tower, the bounds every ELEMENT of their results is held
to, the case lists of the GPU tests (a reason per case, the kernel route it takes stated and checked), and CPU emulations of the kernels' fp32 /
split-bf16 arithmetic that show the bounds are neither violated by correct arithmetic nor vacuous (tests/test_grads_f64.py).  A helper module (not
collected: no test_ prefix); CPU only, it imports nothing that touches a GPU.  T, U, compare_sliced, split_bf16 and E_PREC are those of
tests/small_ops_f64.py and tests/products_f64.py.

1. Weight-gradient products: eg_linear_wgrad_mfma (csrc/lingrad.hip), eg_gemm_tn and eg_colsum (csrc/train.hip)
    reference   dW = dY^T X,  db = sum_r dY,  C = A^T B (+ C_prev when accumulate), in float64.
    bound       with S = sum_r |dy||x|, R the contraction length and Z the number of row / K slices the plan makes, nothing measured:
        dW   (E + (R + Z + 8) 2^-24) S + 2^-24 |ref|      E = E_bf16x3 = 3 2^-16 + 2^-32 for eg_linear_wgrad_mfma, which forms Xl DYh + Xh DYl + Xh DYh
                                                          (the representation argument of products_f64.py), E = 0 for eg_gemm_tn (exact fp32 products);
        db   (R + Z + 8) 2^-24 sum_r |dy| + 2^-24 |ref|   (also eg_colsum's column sums);
        accumulate adds 2 2^-24 (|C_prev| + S).
      R additions into fp32 accumulators whose partial sums are at most S, in any order; the fold of Z partials adds Z more; + 8 covers the order
      inside an MFMA and the row-lane combine of db; 2^-24 |ref| is the rounding of the stored value.  The columns of dY are scaled over three
      decades (logspace(-2, 1)): the bound is per element, so a small-magnitude column cannot hide behind a large one.

2. eg_attention_train / eg_attention_backward_train (csrc/attention.hip)
    The backward takes P as an ARGUMENT, so its contract is a polynomial in (q, k, v, P, dO, M) and no softmax error enters.  In float64, with
    M = keep * fl32(1 / (1 - p)) (the mask as the kernels apply it; keep from oracle.dropout_keep_mask at the flat index
    offset + ((b H + h) Lq + q) Lk + k):
        A = P o M;  dV = A^T dO;  dA = (dO V^T) o M;  rs = rowsum(dA o P);  dS = P o (dA - rs);  dQ = dS K / 8;  dK = dS^T Q / 8.
    Bounds by forward error analysis, fp32 products exact (v_mfma_f32_16x16x4_f32), accumulation in any order, u = 2^-24:
        dV     (Lq + 10) u sum_q A |dO| + u |ref|             Lq additions of exact products of A (one rounding, inside the + 10) with dO;
        e_dA   72 u M sum_d |dO||V| + u |dA|                  64 additions (+ 8) of exact products, then one rounding of the product with M;
        e_rs   sum_k P e_dA + (Lk + 8) u sum_k |dA| P         the error of dA carried through the sum, plus the sum's own Lk additions;
        e_dS   P (e_dA + e_rs + 2 u (|dA| + |rs|))            the subtraction rounds once (<= u (|dA| + |rs|)) and so does the product with P;
        dQ     sum_k e_dS |K| / 8 + (Lk + 10) u sum_k |dS||K| / 8 + u |ref|       the error of dS carried through, the product's Lk additions, the
        dK     the same over the queries with Q (Lq + 10)                        exact scaling by 1 / 8 and the rounding of the stored value.
    Forward with p > 0: `attn` (unmasked) is held to products_f64's attn_bound, `out` to its out-bound with A = P o M in place of P (f32).

3. eg_conv1d_cl_forward / _backward_input / _backward_weight (csrc/conv1d_train.hip)
    reference   torch conv1d and its autograd in float64 on the transposed layout; nn.ConvTranspose1d's roles follow the kernel file's header
                (its forward is backward_input WITH the layer's bias, its bias gradient is db_x).
    bound       (terms + 8) 2^-24 sum |a||b| + 2 2^-24 (|bias| + |ref|), as conv1d_bound of small_ops_f64.py: terms = Ci k (forward), Co k (input
                gradient), B Lo + 16 (weight gradient and db_dy; B L + 16 for db_x): the 16 covers both fold levels.

4. eg_layernorm_backward / eg_layernorm_backward_ex (csrc/train.hip)
    reference   float64 autograd of layer_norm: dx and xhat (plain entry); dx, dgamma, dbeta (_ex), dx_dropped BITWISE oracle.dropout_keep_mask applied
                to the returned dx with the fp32 scale 1 / (1 - p).
    dx          suffers cancellation: no useful a-priori bound.  As LN_TOL of small_ops_f64.py: LN_BWD_FACTOR = 4 x the error of torch's own float32
                CPU layer_norm backward on the same inputs against float64, per element in layernorm_scale units, recorded in LN_BWD_CPU_F32 per
                case list and input class (tests/test_grads_f64.py re-measures them and fails when a figure is stale by more than 2 x).
    dbeta       (rows + 12) 2^-24 sum_r |dy| + 2^-24 |ref|, a priori.
    dgamma      the same on sum_r |dy xhat|, plus sum_r |dy| e_xhat with e_xhat the forward tolerance LN_TOL of small_ops_f64.py per ROW class times
                max(1, |xhat|): a constant row is held to xhat = 0 exactly, as the forward kernels are held to y = beta there.
    xhat        (plain entry) e_xhat.

Emulations (CPU checks only).  emulate_lingrad splits both operands with split_bf16 as the kernel does, forms the three products of a 32-row group in
float64 (bf16 x bf16 is exact in fp32) and rounds each into the fp32 accumulator; slices are folded in fp32.  The others run torch's float32.  Every
emulation has a second summation order (reversed groups / chunked as the kernel chunks).  Over every case of every list the worst element of correct
arithmetic stays at or under 0.5 of its bound (tests/test_grads_f64.py; its figures are in WORST_OF_CORRECT_ARITHMETIC below), with no exception.

Worst element seen on the MI355X as a fraction of its bound (the GPU tests print theirs as FRACTION lines):
    eg_linear_wgrad_mfma (bf16x3)   dW 0.45 (rows = 1: the representation error alone)   db 0.02        eg_gemm_tn (f32) 0.22      eg_colsum 0.09
    eg_attention_backward_train     dq 0.02   dk 0.02   dv 0.20                          eg_attention_train, p > 0    out 0.01   attn 0.02
    eg_conv1d_cl_forward 0.19       _backward_input 0.27      _backward_weight 0.05 (dw, db_dy, db_x)
    eg_layernorm_backward           dx 0.21   xhat 0.17 (of their tolerances)            eg_layernorm_backward_ex     dx 0.36   dgamma 0.10   dbeta 0.12
The constant-row class found a defect: both LayerNorm backward kernels took the mean in one fp32 sum, whose few-ulp error rstd = 1 / sqrt(eps)
multiplied into xhat ~ 1e-4 where it is 0 (dgamma 1.3e3 x its bound at 3 x 576, xhat unbounded); they now take the two-step mean of the forward.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import emogest_oracle as O
from products_f64 import E_PREC, FLT_MIN, attention_bounds, attention_f64, _heads  # noqa: F401
from small_ops_f64 import LN_TOL, T, U, compare_sliced, layernorm_scale, sliced_errors, split_bf16  # noqa: F401  (re-exported for the tests)

E_X3 = E_PREC["bf16x3"]

# Worst element of correct arithmetic (the emulations, both summation orders) as a fraction of its bound, over every case of every list, as
# tests/test_grads_f64.py measures and prints them (it holds each to <= 0.5):
WORST_OF_CORRECT_ARITHMETIC = {
    "eg_linear_wgrad_mfma dW": 0.46, "eg_linear_wgrad_mfma db": 0.04, "eg_gemm_tn": 0.22, "eg_colsum": 0.09,
    "eg_attention_backward_train dq": 0.03, "eg_attention_backward_train dk": 0.03, "eg_attention_backward_train dv": 0.21,
    "eg_conv1d_cl_forward": 0.22, "eg_conv1d_cl_backward_input": 0.15, "eg_conv1d_cl_backward_weight": 0.05,
    "layernorm dgamma": 0.10, "layernorm dbeta": 0.13,
}


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


def _bf(bits):
    return bits.view(torch.bfloat16).double()


# =========================================================================================================================================
# 1. weight-gradient products
# =========================================================================================================================================
WG_AXES = ("output row n", "column k")


def plan_lingrad(rows, n, k):
    """plan_lingrad of csrc/lingrad.hip -> (S, rows_per): the rows are split when they exceed 640 and the 64 x 64 tiles alone cannot fill the chip."""
    tiles = cdiv(n, 64) * cdiv(k, 64)
    s = 1
    if rows > 640 and tiles < 384:
        s = max(1, min(cdiv(384, tiles), cdiv(rows, 256)))
    rows_per = round_up(cdiv(rows, s), 64)
    return cdiv(rows, rows_per), rows_per


def lingrad_xcd(n, k):
    """The XCD blocking lingrad_launch chooses -> (xa, xb), (0, 0) = launch order: gx gy % 8 == 0, xa | gx, xb | gy, the first smallest gx/xa + gy/xb."""
    gx, gy = cdiv(k, 64), cdiv(n, 64)
    best, pick = 1 << 30, (0, 0)
    if (gx * gy) % 8 == 0:
        for xa in (1, 2, 4, 8):
            xb = 8 // xa
            if gx % xa or gy % xb:
                continue
            if gx // xa + gy // xb < best:
                best, pick = gx // xa + gy // xb, (xa, xb)
    return pick


def lingrad_remap(bx, by, gx, gy, xa, xb):
    """Workgroup (blockIdx.x, blockIdx.y) -> the (k tile, n tile) it computes."""
    if not xa:
        return bx, by
    lin = by * gx + bx
    xcd, j = lin & 7, lin >> 3
    bw, bh = gx // xa, gy // xb
    return (xcd % xa) * bw + j % bw, (xcd // xa) * bh + j // bw


def lingrad_workspace_floats(rows, n, k):
    s, _ = plan_lingrad(rows, n, k)
    return s * n * round_up(k, 4) + s * n if s > 1 else 0


# layout name -> (ldy - N, ldx - K, lddw - K as functions of the shape, base offset of dY and X in floats, db asked for)
def wg_layout(name, n, k):
    """-> (ldy, ldx, lddw, base offset in floats, with_db)."""
    if name == "dense":
        return n, k, k, 0, True
    if name == "pad4":                  # every pitch padded AND a multiple of 4: the 16-byte paths next to a gap
        return round_up(n, 4) + 4, round_up(k, 4) + 8, round_up(k, 4) + 4, 0, True
    if name == "odd":                   # N + 1 / K + 3: the scalar staging path and the scalar / narrow stores
        return n + 1, k + 3, k + 3, 0, True
    if name == "off1":                  # dense pitches, dY / X one float past a 16-byte boundary: the scalar staging path
        return n, k, k, 1, True
    if name == "nodb":
        return n, k, k, 0, False
    raise ValueError(name)


WG = namedtuple("WG", "rows n k layout S rows_per xcd why")
_r64 = lambda r: round_up(r, 64)
WGRAD_CASES = (
    # rows at N = K = 64: one tile, S = 1; a stage is 64 rows, an MFMA group 32
    [WG(r, 64, 64, "dense", 1, _r64(r), (0, 0), why) for r, why in (
        (1, "one row: 31 zero rows in the only group"), (31, "one short group"), (32, "exactly one group"), (33, "second group holds one row"),
        (63, "one short stage"), (64, "exactly one stage"), (65, "second stage holds one row (the double buffer turns once)"),
        (127, "two stages, the last short"), (128, "two full stages"), (129, "three stages: both LDS buffers reused"))]
    # N and K at rows = 70: ragged tiles on both axes; N or K % 4 != 0 takes the scalar staging path and the narrow stores
    + [WG(70, n, k, "dense", 1, 128, (0, 0), why) for n, k, why in (
        (1, 130, "a single output row; K % 4 == 2: scalar X staging, three k tiles"), (3, 66, "N % 4 == 3 and K % 4 == 2"),
        (4, 127, "one column quad of dY; K % 4 == 3, lddw odd: scalar stores"), (63, 64, "ragged N: the scalar dY path, the vector X path"),
        (64, 63, "ragged K: the vector dY path, the scalar X path"), (65, 128, "N one past a tile: a second n tile with one row"),
        (66, 1, "K = 1: one column of dW"), (127, 3, "K = 3"), (128, 65, "K one past a tile"), (130, 4, "N % 4 == 2, K = 4: one quad"),
        (130, 66, "both ragged, six tiles"))]
    # the row split: rows > 640 and tiles < 384
    + [WG(640, 64, 64, "dense", 1, 640, (0, 0), "the last row count without the split"),
       WG(641, 64, 64, "dense", 3, 256, (0, 0), "the split starts: S = 3, the last slice holds 129 rows"),
       WG(768, 64, 64, "dense", 3, 256, (0, 0), "three full slices"),
       WG(1025, 64, 64, "dense", 5, 256, (0, 0), "S = 5 and the LAST SLICE HOLDS ONE ROW"),
       WG(1100, 64, 64, "dense", 5, 256, (0, 0), "S = 5, the last slice 76 rows"),
       WG(1100, 66, 130, "dense", 5, 256, (0, 0), "ragged partial tiles through the fold (partials at pitch 132, the reduce kernel's narrow store)"),
       WG(1025, 66, 130, "odd", 5, 256, (0, 0), "the same with odd pitches: scalar staging in every slice, narrow stores in the fold")]
    # the XCD remap: gx gy % 8 == 0
    + [WG(70, 64, 512, "dense", 1, 128, (8, 1), "8 x 1 tiles: blocks of one tile (the remap is the identity)"),
       WG(70, 512, 64, "dense", 1, 128, (1, 8), "1 x 8 tiles: db from eight workgroups"),
       WG(70, 128, 256, "dense", 1, 128, (4, 2), "4 x 2 tiles"),
       WG(70, 256, 256, "dense", 1, 128, (2, 4), "4 x 4 tiles in 2 x 1 blocks: the remap moves tiles; db comes from the workgroups whose REMAPPED tx is 0"),
       WG(70, 200, 100, "dense", 1, 128, (2, 4), "2 x 4 ragged tiles under the remap"),
       WG(70, 256, 256, "nodb", 1, 128, (2, 4), "the remap without db"),
       WG(1100, 128, 256, "dense", 5, 256, (4, 2), "the split on top of the remap (partials and db partials per slice)")]
    # pitches and pointers
    + [WG(70, n, k, lay, 1, 128, (0, 0), why) for n, k in ((64, 64), (66, 130)) for lay, why in (
        ("pad4", "ldy > N, ldx > K, lddw > K, all multiples of 4"), ("odd", "ldy = N + 1, ldx = K + 3, lddw = K + 3"),
        ("off1", "dY and X one float past a 16-byte boundary"), ("nodb", "db = NULL"))]
    + [WG(1100, 64, 64, lay, 5, 256, (0, 0), "split rows, " + lay) for lay in ("pad4", "off1", "nodb")]
)


def wgrad_inputs(rows, n, k):
    """-> dY [rows, N] with its columns scaled over three decades, X [rows, K] (fp32)."""
    key = f"wg{rows}x{n}x{k}"
    return T(key + "dy", (rows, n)) * torch.logspace(-2, 1, n), T(key + "x", (rows, k))


def wgrad_f64(dy, x, prev=None):
    dw = dy.double().T @ x.double()
    return (dw if prev is None else dw + prev.double()), dy.double().sum(0)


def wgrad_bounds(dy, x, E, Z, prev=None):
    """-> (dW bound [N, K], db bound [N]); see the module docstring."""
    R = dy.shape[0]
    S = dy.double().abs().T @ x.double().abs()
    dw, db = wgrad_f64(dy, x, prev)
    bw = (E + (R + Z + 8) * U) * S + U * dw.abs()
    if prev is not None:
        bw = bw + 2 * U * (prev.double().abs() + S)
    return bw, (R + Z + 8) * U * dy.double().abs().sum(0) + U * db.abs()


def emulate_lingrad(dy, x, order="forward", fault=None):
    """linear_wgrad_bf16_kernel + linear_wgrad_reduce_kernel on the CPU -> (dW fp32 [N, K], db fp32 [N]).  order: "forward" / "reversed" (the 32-row
    groups of a slice, the row lanes of db and the slices of the fold walked backwards).  fault: None or one of
      "drop_group"     the last 32-row group of the last slice is not contracted;
      "lohi_tile"      the Xl DYh term is missing in the 16 x 16 tile n 0..15, k 0..15;
      "fold_skip"      the last slice's partial is left out of the fold (S > 1);
      "db_rows"        db misses the first 16 rows of slice 0 in column quad 0;
      "db_unremapped"  db is written by the workgroups whose LAUNCH blockIdx.x is 0 instead of those whose remapped tx is 0."""
    rows, n = dy.shape
    k = x.shape[1]
    S, rows_per = plan_lingrad(rows, n, k)
    (dhb, dlb), (xhb, xlb) = split_bf16(dy), split_bf16(x)
    dh, dl, xh, xl = _bf(dhb), _bf(dlb), _bf(xhb), _bf(xlb)
    rev = order == "reversed"
    parts, dbparts = [], []
    for z in range(S):
        r0, r1 = z * rows_per, min(rows, (z + 1) * rows_per)
        groups = list(range(r0, r1, 32))
        if fault == "drop_group" and z == S - 1:
            groups = groups[:-1]
        acc = torch.zeros(n, k, dtype=torch.float32)
        for g0 in (groups[::-1] if rev else groups):
            sl = slice(g0, min(g0 + 32, r1))
            lohi = dh[sl].T @ xl[sl]
            if fault == "lohi_tile":
                lohi[:16, :16] = 0.0
            for term in (lohi, dl[sl].T @ xh[sl], dh[sl].T @ xh[sl]):
                acc = (acc.double() + term).float()
        parts.append(acc)
        # db: row lane rr of a column adds rows r0 + rr + 16 i in order; the 16 lanes are combined in order
        blk = torch.zeros(round_up(r1 - r0, 16), n, dtype=torch.float32)
        blk[:r1 - r0] = dy[r0:r1].float()
        if fault == "db_rows" and z == 0:
            blk[:16, :4] = 0.0
        blk = blk.view(-1, 16, n)
        lane = torch.zeros(16, n, dtype=torch.float32)
        for i in (range(blk.shape[0] - 1, -1, -1) if rev else range(blk.shape[0])):
            lane = lane + blk[i]
        s = torch.zeros(n, dtype=torch.float32)
        for j in (range(15, -1, -1) if rev else range(16)):
            s = s + lane[j]
        dbparts.append(s)
    if fault == "fold_skip":
        parts = parts[:-1]
    if rev:
        parts, dbparts = parts[::-1], dbparts[::-1]
    dw, db = parts[0], dbparts[0]
    for p in parts[1:]:
        dw = dw + p
    for p in dbparts[1:]:
        db = db + p
    if fault == "db_unremapped":
        gx, gy = cdiv(k, 64), cdiv(n, 64)
        xa, xb = lingrad_xcd(n, k)
        wrong = torch.zeros_like(db)            # a tile nobody writes keeps what the buffer held
        for by in range(gy):
            tx, ty = lingrad_remap(0, by, gx, gy, xa, xb)
            wrong[64 * ty:64 * ty + 64] = db[64 * ty:64 * ty + 64]
        db = wrong
    return dw, db


# ---- eg_gemm_tn ----------------------------------------------------------------------------------------------------------------------------
def plan_gemm_tn(m, n, k):
    """eg_gemm_tn_workspace_floats / launch_gemm_tn of csrc/train.hip -> (splits, kps, nz): the split starts above k = 256; kps is rounded up to 32,
    so nz = ceil(k / kps) can be smaller than splits."""
    tiles = cdiv(m, 64) * cdiv(n, 64)
    splits = 1 if tiles >= 512 else cdiv(1024, tiles)
    splits = max(1, min(splits, cdiv(k, 256)))
    kps = round_up(cdiv(k, splits), 32)
    return splits, kps, cdiv(k, kps)


def gemm_tn_workspace_floats(m, n, k):
    splits = plan_gemm_tn(m, n, k)[0]
    return splits * m * n if splits > 1 else 0


TN = namedtuple("TN", "m n k layout accumulate nz why")
_TN_MN = (1, 63, 64, 65, 130)
_TN_K = ((1, 1, "a single k"), (31, 1, "one short K step"), (32, 1, "exactly one K step"), (33, 1, "second step holds one k"),
         (255, 1, "the last k below the split"), (256, 1, "the last k without the split"), (257, 2, "the split starts: slices of 160 and 97"),
         (513, 3, "three slices of 192 / 192 / 129"), (1000, 4, "four slices of 256 / 256 / 256 / 232"))
TN_CASES = (
    # every k with m, n rotating through the tile edges; accumulate and the layout alternate
    [TN(_TN_MN[i % 5], _TN_MN[(2 * i + 1) % 5], k, ("dense", "odd", "pad4")[i % 3], i % 2, nz, why) for i, (k, nz, why) in enumerate(_TN_K)]
    # every (m, n) edge pair once at a split and once at an unsplit depth
    + [TN(m, n, 257 if (i + j) % 2 else 33, ("odd", "dense")[(i + j) % 2], (i + j + 1) % 2, 2 if (i + j) % 2 else 1, "tile edge pair")
       for i, m in enumerate(_TN_MN) for j, n in enumerate(_TN_MN)]
    + [TN(130, 130, 1000, "odd", 1, 4, "nine tiles, four slices, accumulate on odd pitches"),
       TN(512, 512, 4097, "dense", 0, 15, "64 tiles ask for 16 splits; kps = 288 leaves nz = 15 < splits (the workspace is sized for 16)")]
)


def tn_layout(name, m, n):
    """-> (lda, ldb, ldc)."""
    if name == "dense":
        return m, n, n
    if name == "odd":
        return m + 1, n + 3, n + 5
    if name == "pad4":
        return round_up(m, 4) + 4, round_up(n, 4) + 8, round_up(n, 4) + 4
    raise ValueError(name)


def gemm_tn_inputs(m, n, k):
    """-> A [k, m] with its columns scaled over three decades, B [k, n], C_prev [m, n]."""
    key = f"tn{m}x{n}x{k}"
    return T(key + "a", (k, m)) * torch.logspace(-2, 1, m), T(key + "b", (k, n)), T(key + "c", (m, n), -3, 3)


def emulate_gemm_tn(a, b, prev=None, order="forward"):
    """torch float32 per K slice, the slices folded in fp32 (order "chunked": 32-deep steps walked backwards inside a slice, slices backwards)."""
    k, m = a.shape
    n = b.shape[1]
    _, kps, nz = plan_gemm_tn(m, n, k)
    parts = []
    for z in range(nz):
        k0, k1 = z * kps, min(k, (z + 1) * kps)
        if order == "forward":
            parts.append(a[k0:k1].float().T @ b[k0:k1].float())
        else:
            acc = torch.zeros(m, n)
            for s in range(k0 + (cdiv(k1 - k0, 32) - 1) * 32, k0 - 1, -32):
                acc = acc + a[s:min(s + 32, k1)].float().T @ b[s:min(s + 32, k1)].float()
            parts.append(acc)
    if order != "forward":
        parts = parts[::-1]
    c = parts[0]
    for p in parts[1:]:
        c = c + p
    return c if prev is None else prev.float() + c


# ---- eg_colsum -----------------------------------------------------------------------------------------------------------------------------
COLSUM_ROWS = (1, 255, 256, 257, 1030)
COLSUM_C = (1, 63, 64, 65)


def colsum_route(rows, c):
    """col_sums of csrc/train.hip for 16-byte aligned operands -> (kernel, number of row blocks)."""
    if c % 4 == 0 and rows <= 1024:
        return "col_direct_kernel", 1
    fast = c >= 4 and 1024 % c == 0
    nblk = max(1, min(2048, cdiv(rows * c, 16384) if fast else cdiv(rows, 128)))
    return ("col_partial_fast_kernel" if fast else "col_partial_kernel"), cdiv(rows, cdiv(rows, nblk))


# (rows, c) -> route; c = 64 up to 1024 rows: one launch; c = 64 at 1030 rows: the 16-byte stream + double fold; c = 1 / 63 / 65: the generic kernel
COLSUM_CASES = [(r, c) + colsum_route(r, c) for r in COLSUM_ROWS for c in COLSUM_C]


def colsum_inputs(rows, c):
    key = f"cs{rows}x{c}"
    return T(key + "a", (rows, c)) * torch.logspace(-2, 1, c), T(key + "b", (rows, c))


def colsum_bounds(a, b, z):
    """-> (bound of sum_r a, bound of sum_r a b): the db bound, on |a| and on |a b|."""
    R = a.shape[0]
    ad, pd = a.double(), a.double() * b.double()
    return ((R + z + 8) * U * ad.abs().sum(0) + U * ad.sum(0).abs(), (R + z + 8) * U * pd.abs().sum(0) + U * pd.sum(0).abs())


# =========================================================================================================================================
# 2. attention training pair
# =========================================================================================================================================
ATB, ATH = 2, 2                     # clips and heads of every case: a clip or head index error shows
ATD = ATH * 64
DQ_AXES = ("clip", "query", "column")
DK_AXES = ("clip", "key", "column")
AT_SEED = 20231


def att_route(lk):
    """eg_attention_backward_train -> (KT, QC): key tiles of 16 resident in LDS, queries walked in chunks of QC."""
    return (3, 64) if lk <= 48 else ((4, 64) if lk <= 64 else (8, 32))


AT = namedtuple("AT", "lq lk p offset cls layout route why")
_O = 4096
ATT_TRAIN_CASES = (
    [AT(20, lk, (0.0, 0.1)[i % 2], _O, "normal", ("dense", "kv2")[i % 2], att_route(lk), why) for i, (lk, why) in enumerate((
        (1, "one key: P = 1, dS = 0"), (4, "one key quad"), (15, "ragged first key tile"), (16, "one key tile"), (17, "second tile holds one key"),
        (47, "KT = 3, last tile ragged"), (48, "KT = 3 full"), (49, "KT = 4 starts, its last tile holds one key"), (63, "KT = 4 ragged"),
        (64, "KT = 4 full"), (65, "KT = 8 / QC = 32 starts"), (127, "KT = 8 ragged"), (128, "KT = 8 full: the largest Lk")))]
    + [AT(lq, 34, (0.1, 0.0)[i % 2], _O, "normal", "dense" if i % 3 else "kv2", (3, 64), why) for i, (lq, why) in enumerate((
        (1, "one query"), (15, "ragged query tile"), (16, "one query tile"), (17, "second tile holds one query"), (31, "two tiles, ragged"),
        (32, "two tiles"), (33, "third wave holds one query"), (63, "chunk of 64 ragged"), (64, "exactly one chunk"),
        (65, "CHUNK SEAM: the second chunk holds one query"), (130, "two seams: 64 + 64 + 2")))]
    + [AT(lq, 120, 0.1, _O, "normal", "dense", (8, 32), why) for lq, why in (
        (31, "chunk of 32 ragged"), (32, "exactly one chunk of 32"), (33, "seam at 32"), (65, "two seams: 32 + 32 + 1"))]
    + [AT(34, 34, 0.1, _O, "normal", "qkv3", (3, 64), "q / k / v as slices of one [rows, 3 D] buffer (self-attention as functional.py holds it)"),
       AT(60, 60, 0.1, _O, "normal", "qkv3", (4, 64), "the same at KT = 4"),
       AT(120, 120, 0.0, _O, "normal", "qkv3", (8, 32), "the same at KT = 8, no dropout"),
       AT(17, 49, 0.5, _O, "normal", "kv2", (4, 64), "p = 0.5 with the mask at the last key tile, which holds ONE key"),
       AT(33, 65, 0.5, _O, "normal", "dense", (8, 32), "p = 0.5, the last key tile holds one key, query seam at 32"),
       AT(20, 34, 0.1, (1 << 32) + 12345, "normal", "dense", (3, 64), "offset > 2^32: the counter's high word enters the hash"),
       AT(65, 34, 0.1, _O, "peaked", "dense", (3, 64), "q scaled by 6: most P near zero"),
       AT(33, 120, 0.1, _O, "peaked", "kv2", (8, 32), "peaked at KT = 8")]
)
# P chained: P is the attn output of eg_attention_train on the same inputs, one per route
ATT_CHAINED_CASES = [AT(20, 47, 0.1, _O, "normal", "kv2", (3, 64), "chained, KT = 3"), AT(65, 64, 0.1, _O, "normal", "dense", (4, 64), "chained, KT = 4"),
                     AT(33, 120, 0.5, _O, "normal", "kv2", (8, 32), "chained, KT = 8"), AT(60, 60, 0.1, _O, "normal", "qkv3", (4, 64), "chained, packed qkv")]


def att_train_inputs(lq, lk, cls="normal"):
    """-> q [B, Lq, D], k, v [B, Lk, D], dO [B, Lq, D]: standard normal (seeded by the shape); peaked: q scaled by 6."""
    g = torch.Generator().manual_seed(1000 * lq + lk)
    q, k, v, do = (torch.randn(ATB, l, ATD, generator=g) for l in (lq, lk, lk, lq))
    if cls == "peaked":
        q = 6.0 * q
    elif cls != "normal":
        raise ValueError(cls)
    return q, k, v, do


def att_mask(lq, lk, p, offset, seed=AT_SEED):
    """-> M [B, H, Lq, Lk] float64 = keep * fl32(1 / (1 - p)), keep from oracle.dropout_keep_mask at offset + ((b H + h) Lq + q) Lk + k."""
    if p == 0:
        return torch.ones(ATB, ATH, lq, lk, dtype=torch.float64)
    keep = O.dropout_keep_mask(seed, offset, ATB * ATH * lq * lk, p)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(keep.astype(np.float64) * float(inv)).view(ATB, ATH, lq, lk)


def att_softmax_f32(q, k):
    """P given: the fp32 rounding of the float64 softmax."""
    return attention_f64(q, k, k, ATH)[1].float()


def _unheads(t):
    b, h, l, d = t.shape
    return t.transpose(1, 2).reshape(b, l, h * d)


def att_backward_f64(q, k, v, P, do, M):
    """-> dict of dq [B, Lq, D], dk, dv [B, Lk, D] and the intermediates (float64, head-split [B, H, L, .])."""
    qh, kh, vh, dh = (_heads(t.double(), ATH) for t in (q, k, v, do))
    P = P.double()
    A = P * M
    dA = (dh @ vh.transpose(2, 3)) * M
    rs = (dA * P).sum(-1, keepdim=True)
    dS = P * (dA - rs)
    return {"dq": _unheads(dS @ kh / 8.0), "dk": _unheads(dS.transpose(2, 3) @ qh / 8.0), "dv": _unheads(A.transpose(2, 3) @ dh),
            "A": A, "dA": dA, "rs": rs, "dS": dS}


def att_backward_bounds(q, k, v, P, do, M):
    """-> dict of the dq / dk / dv bounds; see the module docstring for the chain."""
    lq, lk = q.shape[1], k.shape[1]
    qh, kh, vh, dh = (_heads(t.double(), ATH) for t in (q, k, v, do))
    r = att_backward_f64(q, k, v, P, do, M)
    P = P.double()
    A, dA, rs, dS = r["A"], r["dA"], r["rs"], r["dS"]
    e_dA = 72 * U * M * (dh.abs() @ vh.abs().transpose(2, 3)) + U * dA.abs()
    e_rs = (P * e_dA).sum(-1, keepdim=True) + (lk + 8) * U * (dA.abs() * P).sum(-1, keepdim=True)
    e_dS = P * (e_dA + e_rs + 2 * U * (dA.abs() + rs.abs()))
    bq = _unheads(e_dS @ kh.abs() / 8.0 + (lk + 10) * U * (dS.abs() @ kh.abs()) / 8.0) + U * r["dq"].abs()
    bk = _unheads(e_dS.transpose(2, 3) @ qh.abs() / 8.0 + (lq + 10) * U * (dS.abs().transpose(2, 3) @ qh.abs()) / 8.0) + U * r["dk"].abs()
    bv = _unheads((lq + 10) * U * (A.transpose(2, 3) @ dh.abs())) + U * r["dv"].abs()
    return {"dq": bq, "dk": bk, "dv": bv}


def att_forward_f64(q, k, v, M):
    """-> (out [B, Lq, D] = (P o M) V, attn [B, H, Lq, Lk] unmasked, out bound, attn bound): products_f64's f32 bounds with A = P o M in place of P."""
    lk = k.shape[1]
    _, P = attention_f64(q, k, v, ATH)
    _, ba = attention_bounds(q, k, v, ATH, None, "f32")
    vh = _heads(v.double(), ATH)
    out = _unheads((P * M) @ vh)
    bo = _unheads((ba * M) @ vh.abs() + (lk + 8) * U * ((P * M) @ vh.abs())) + U * out.abs()
    return out, P, bo, ba


def emulate_att_backward(q, k, v, P, do, M, order="forward", fault=None):
    """attention_bwd_mfma_kernel in torch float32 -> dq, dk, dv.  order "forward": whole-tensor float32 products; "chunked": the queries in chunks of
    QC accumulated into dK / dV as the kernel does, the row sum over the keys backwards.  fault: None or one of
      "rowsum_quarter"  the row sum of query 0 runs over the first quarter of the keys only;
      "mask_dv_only"    M is applied to A (dV) but not to dA;
      "chunk_dk"        the last query chunk's contribution to dK is missing;
      "no_eighth_dk"    1 / 8 omitted on dK;
      "neighbour_mask"  the last key takes the mask of the key before it."""
    lq, lk = q.shape[1], k.shape[1]
    qc = att_route(lk)[1]
    qh, kh, vh, dh = (_heads(t.float(), ATH) for t in (q, k, v, do))
    P, Mf = P.float(), M.float()
    if fault == "neighbour_mask" and lk > 1:
        Mf = Mf.clone()
        Mf[..., lk - 1] = Mf[..., lk - 2]
    A = P * Mf
    dA = dh @ vh.transpose(2, 3)
    if fault != "mask_dv_only":
        dA = dA * Mf
    prod = dA * P
    if order == "forward":
        rs = prod.sum(-1, keepdim=True)
    else:
        rs = torch.zeros(ATB, ATH, lq, 1)
        for j in range(lk - 1, -1, -1):
            rs = rs + prod[..., j:j + 1]
    if fault == "rowsum_quarter":
        rs = rs.clone()
        rs[:, :, 0] = prod[:, :, 0, :max(1, lk // 4)].sum(-1, keepdim=True)
    dS = P * (dA - rs)
    dq = (dS @ kh) * 0.125
    chunks = [slice(c, min(c + qc, lq)) for c in range(0, lq, qc)]
    if order == "forward" and fault != "chunk_dk":
        dk, dv = dS.transpose(2, 3) @ qh, A.transpose(2, 3) @ dh
    else:
        dk, dv = torch.zeros(ATB, ATH, lk, 64), torch.zeros(ATB, ATH, lk, 64)
        for i, c in enumerate(chunks):
            if not (fault == "chunk_dk" and i == len(chunks) - 1):
                dk = dk + dS[:, :, c].transpose(2, 3) @ qh[:, :, c]
            dv = dv + A[:, :, c].transpose(2, 3) @ dh[:, :, c]
    if fault != "no_eighth_dk":
        dk = dk * 0.125
    return _unheads(dq), _unheads(dk), _unheads(dv)


# =========================================================================================================================================
# 3. channels-last conv1d of the training path
# =========================================================================================================================================
C1_AXES = ("sample", "position", "channel")
C1_LDS_CAP = 64 * 1024


def cpw_of(channels):
    """Channels per wave of the tiled forward / input-gradient kernels, 0 = too wide (more than 64 channels): the untiled kernel."""
    need = cdiv(channels, 4)
    for o in (1, 2, 4, 8, 12, 16):
        if need <= o:
            return o
    return 0


def c1_len_out(l, k, stride, pad, dil):
    return (l + 2 * pad - dil * (k - 1) - 1) // stride + 1


def c1_forward_route(ci, co, k, stride, pad, dil):
    """-> "fwd_tiled<CPW>" or "fwd_untiled" (eg_conv1d_cl_forward's launch condition)."""
    cpw = cpw_of(co)
    span = 63 * stride + (k - 1) * dil + 1
    lds = 4 * (((span * (ci + 1) + 3) & ~3) + ci * k * 4 * cpw)
    return f"fwd_tiled<{cpw}>" if cpw and lds <= C1_LDS_CAP else "fwd_untiled"


def c1_input_route(ci, co, k, stride, pad, dil):
    """-> "dx_tiled<CPW>" or "dx_untiled": tiled needs pad <= (k - 1) dil besides the channel count and the LDS cap."""
    cpw = cpw_of(ci)
    rows_cap = (63 + (k - 1) * dil) // stride + 2
    lds = 4 * (((rows_cap * (co + 1) + 3) & ~3) + co * k * 4 * cpw)
    return f"dx_tiled<{cpw}>" if cpw and lds <= C1_LDS_CAP and pad <= (k - 1) * dil else "dx_untiled"


def plan_c1w(ci, lo, co, k, stride, dil):
    """plan_c1w -> (cob, lds bytes, nchunk); cob 0 = the shape takes the one-launch kernel."""
    cob = 8 if co <= 8 else (16 if co <= 16 else (36 if co <= 36 else 0))
    span, ncol = 127 * stride + (k - 1) * dil + 1, ci * k + 1
    tiles = ((span * (ci + 1) + 3) & ~3) + 128 * cob
    fold = (256 // ncol) * ncol * (cob + 1) if ncol <= 256 else 0
    lds = 4 * max(tiles, fold)
    if ncol > 256 or lds > C1_LDS_CAP:
        cob = 0
    return cob, lds, cdiv(lo, 128)


def c1_weight_workspace_floats(b, ci, lo, co, k, stride, dil):
    cob, _, nchunk = plan_c1w(ci, lo, co, k, stride, dil)
    return 0 if not cob or b * lo < 512 else b * nchunk * co * (ci * k + 1)


def c1_weight_route(b, ci, lo, co, k, stride, dil, db_x=False):
    """-> "dw_one" (conv1d_cl_bwd_weight_kernel) or "dw_tiled<COB>/P" with P partials for the fold; db_x always takes the one-launch kernel."""
    if db_x or not c1_weight_workspace_floats(b, ci, lo, co, k, stride, dil):
        return "dw_one"
    cob, _, nchunk = plan_c1w(ci, lo, co, k, stride, dil)
    return f"dw_tiled<{cob}>/{b * nchunk}"


C1 = namedtuple("C1", "b l ci co k stride pad dil fwd dx dw why")
C1_CASES = [
    # the six CPW instantiations at both ends (channels 1 .. 64) and 65 untiled: Co drives the forward's CPW, Ci the input gradient's
    C1(2, 34, 1, 1, 3, 1, 1, 1, "fwd_tiled<1>", "dx_tiled<1>", "dw_one", "a single channel on both sides"),
    C1(2, 34, 4, 5, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<1>", "dw_one", "Ci = 4: the last of CPW 1; Co = 5: the first of CPW 2"),
    C1(2, 34, 5, 4, 3, 1, 2, 1, "fwd_tiled<1>", "dx_tiled<2>", "dw_one", "the transpose of it; pad = (k - 1) dil"),
    C1(2, 34, 8, 9, 5, 2, 2, 1, "fwd_tiled<4>", "dx_tiled<2>", "dw_one", "8 | 9: CPW 2 -> 4; stride 2"),
    C1(2, 34, 9, 8, 5, 2, 0, 1, "fwd_tiled<2>", "dx_tiled<4>", "dw_one", "pad 0"),
    C1(2, 34, 16, 17, 3, 1, 0, 2, "fwd_tiled<8>", "dx_tiled<4>", "dw_one", "16 | 17: CPW 4 -> 8; dilation 2"),
    C1(2, 34, 17, 16, 3, 3, 1, 1, "fwd_tiled<4>", "dx_tiled<8>", "dw_one", "stride 3"),
    C1(2, 34, 32, 33, 1, 1, 0, 1, "fwd_tiled<12>", "dx_tiled<8>", "dw_one", "32 | 33: CPW 8 -> 12; k = 1"),
    C1(2, 34, 33, 32, 1, 2, 0, 1, "fwd_tiled<8>", "dx_tiled<12>", "dw_one", "k = 1 at stride 2: every second input position gets no gradient but the bias"),
    C1(2, 34, 48, 49, 3, 1, 1, 1, "fwd_tiled<16>", "dx_tiled<12>", "dw_one", "48 | 49: CPW 12 -> 16"),
    C1(2, 34, 49, 48, 3, 2, 1, 2, "fwd_tiled<12>", "dx_tiled<16>", "dw_one", "stride 2 with dilation 2"),
    C1(2, 34, 64, 65, 1, 1, 0, 1, "fwd_untiled", "dx_tiled<16>", "dw_one", "Co = 65: the untiled forward; Ci = 64: the widest tiled input gradient (k = 1 keeps it under the LDS cap)"),
    C1(2, 34, 65, 64, 1, 1, 0, 1, "fwd_tiled<16>", "dx_untiled", "dw_one", "Ci = 65: the untiled input gradient; Co = 64: the widest tiled forward"),
    C1(2, 34, 6, 64, 3, 1, 1, 1, "fwd_tiled<16>", "dx_tiled<2>", "dw_one", "Co = 64 at k = 3"),
    C1(2, 34, 64, 6, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<16>", "dw_one", "Ci = 64 at k = 3"),
    # positions: one 64-position tile and its seam
    C1(2, 1, 6, 7, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "L = Lo = 1"),
    C1(2, 63, 6, 7, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "L = Lo = 63"),
    C1(2, 64, 6, 7, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "L = Lo = 64: exactly one tile"),
    C1(2, 65, 6, 7, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "L = Lo = 65: the taps at positions 63 -> 64 cross the tile seam"),
    C1(2, 129, 6, 7, 5, 1, 2, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "L = Lo = 129: three tiles, k = 5 across both seams"),
    C1(3, 129, 5, 6, 8, 2, 7, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "k = 8, stride 2, pad = k - 1: Lo = 68, a seam at 64 on both sides"),
    C1(2, 130, 3, 4, 3, 3, 0, 2, "fwd_tiled<1>", "dx_tiled<1>", "dw_one", "stride 3 with dilation 2 over three input tiles"),
    C1(2, 70, 6, 7, 5, 1, 8, 2, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "pad = (k - 1) dil = 8: the largest pad of the tiled input gradient"),
    C1(2, 70, 6, 7, 3, 1, 4, 1, "fwd_tiled<2>", "dx_untiled", "dw_one", "pad > (k - 1) dil: the input gradient goes untiled while the forward stays tiled"),
    C1(1, 140, 64, 6, 8, 3, 0, 2, "fwd_untiled", "dx_tiled<16>", "dw_one", "Ci = 64, k = 8, stride 3, dilation 2: the forward's tile is over the 64 KiB LDS cap"),
    C1(1, 140, 17, 64, 8, 1, 7, 2, "fwd_tiled<16>", "dx_untiled", "dw_one", "Ci = 17 (CPW 8), Co = 64, k = 8: the input gradient's tile is over the cap, the forward's is not"),
    # weight gradient: one launch below B Lo = 512, tiled from there on
    C1(7, 73, 6, 8, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_one", "B Lo = 511: the last one-launch size"),
    C1(8, 64, 6, 8, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<2>", "dw_tiled<8>/8", "B Lo = 512: tiled, COB 8, 8 partials"),
    C1(4, 128, 6, 9, 3, 1, 1, 1, "fwd_tiled<4>", "dx_tiled<2>", "dw_tiled<16>/4", "Co = 9: COB 16; Lo = 128: one full chunk per clip; 4 partials (one per wave of the fold)"),
    C1(5, 128, 5, 16, 5, 1, 2, 2, "fwd_tiled<4>", "dx_tiled<2>", "dw_tiled<16>/5", "Co = 16; 5 partials: the fold's tail"),
    C1(13, 129, 4, 17, 3, 2, 1, 1, "fwd_tiled<8>", "dx_tiled<1>", "dw_tiled<36>/13", "Co = 17: COB 36; Lo = 65 at stride 2; 13 partials"),
    C1(8, 129, 4, 36, 3, 1, 1, 1, "fwd_tiled<12>", "dx_tiled<1>", "dw_tiled<36>/16", "Co = 36: the widest COB; Lo = 129: a second chunk of one row; 16 partials: one unrolled fold turn"),
    C1(4, 129, 4, 37, 3, 1, 1, 1, "fwd_tiled<12>", "dx_tiled<1>", "dw_one", "Co = 37: too wide for the tiled weight gradient"),
    C1(17, 40, 3, 5, 3, 1, 1, 1, "fwd_tiled<2>", "dx_tiled<1>", "dw_tiled<8>/17", "17 partials: one unrolled fold turn and a tail of one"),
    C1(29, 30, 3, 5, 2, 1, 0, 1, "fwd_tiled<2>", "dx_tiled<1>", "dw_tiled<8>/29", "29 partials; even k"),
    C1(2, 257, 51, 4, 5, 1, 2, 1, "fwd_tiled<1>", "dx_tiled<16>", "dw_tiled<8>/6", "Ci k + 1 = 256: one row group fills the workgroup; Lo = 257: three chunks, the last one row"),
    C1(2, 257, 64, 4, 4, 1, 2, 1, "fwd_tiled<1>", "dx_tiled<16>", "dw_one", "Ci k + 1 = 257: one column too many for the tiled weight gradient"),
]
# weight gradient with db_x (the ConvTranspose1d bias gradient: always the one-launch kernel) and with db_dy = NULL, on tiled-size shapes
C1_DBX_CASES = [c for c in C1_CASES if c.dw in ("dw_tiled<8>/8", "dw_tiled<36>/16")]


def c1_inputs(case):
    """-> x [B, L, Ci], w [Co, Ci, k], bias_y [Co], bias_x [Ci], dy [B, Lo, Co] (fp32, channels-last), Lo."""
    key = "c1cl" + "_".join(str(v) for v in case[:8])
    lo = c1_len_out(case.l, case.k, case.stride, case.pad, case.dil)
    a = 1.0 / np.sqrt(case.ci * case.k)
    return (T(key + "x", (case.b, case.l, case.ci)), T(key + "w", (case.co, case.ci, case.k), -a, a), T(key + "b", (case.co,), -0.2, 0.2),
            T(key + "bx", (case.ci,), -0.2, 0.2), T(key + "dy", (case.b, lo, case.co)), lo)


def _c1_grads(x, w, dy, case):
    """float64 autograd on the transposed layout -> (y [B, Lo, Co] without bias, dx [B, L, Ci], dw [Co, Ci, k])."""
    xt = x.double().transpose(1, 2).contiguous().requires_grad_(True)
    wd = w.double().clone().requires_grad_(True)
    y = TF.conv1d(xt, wd, None, stride=case.stride, padding=case.pad, dilation=case.dil)
    y.backward(dy.double().transpose(1, 2))
    return y.detach().transpose(1, 2), xt.grad.transpose(1, 2), wd.grad


def c1_f64(case):
    """-> dict: y (with bias_y), dx (with bias_x: the ConvTranspose1d forward), dx0 (no bias), dw, db_dy, db_x and the bound of each."""
    x, w, by, bx, dy, lo = c1_inputs(case)
    y, dx, dw = _c1_grads(x, w, dy, case)
    ya, dxa, dwa = _c1_grads(x.abs(), w.abs(), dy.abs(), case)
    tf, tx, tw = case.ci * case.k, case.co * case.k, case.b * lo + 16
    r = {"y": y + by.double(), "y0": y, "dx": dx + bx.double(), "dx0": dx, "dw": dw, "db_dy": dy.double().sum((0, 1)), "db_x": x.double().sum((0, 1))}
    r["b_y"] = (tf + 8) * U * ya + 2 * U * (by.double().abs() + r["y"].abs())
    r["b_y0"] = (tf + 8) * U * ya + 2 * U * y.abs()
    r["b_dx"] = (tx + 8) * U * dxa + 2 * U * (bx.double().abs() + r["dx"].abs())
    r["b_dx0"] = (tx + 8) * U * dxa + 2 * U * dx.abs()
    r["b_dw"] = (tw + 8) * U * dwa + 2 * U * dw.abs()
    r["b_db_dy"] = (tw + 8) * U * dy.double().abs().sum((0, 1)) + 2 * U * r["db_dy"].abs()
    r["b_db_x"] = (case.b * case.l + 16 + 8) * U * x.double().abs().sum((0, 1)) + 2 * U * r["db_x"].abs()
    return r


def _c1_gather(x, case, lo, j):
    """x [B, L, Ci] -> [B, Lo, Ci]: the input rows tap j reads (zero outside the input)."""
    li = torch.arange(lo) * case.stride - case.pad + j * case.dil
    ok = (li >= 0) & (li < case.l)
    out = torch.zeros(x.shape[0], lo, x.shape[2], dtype=x.dtype)
    out[:, ok] = x[:, li[ok]]
    return out


def emulate_c1(case, order="forward", fault=None):
    """The three products in float32 -> dict y, dx, dw, db_dy.  order "forward": torch's float32 conv1d and autograd; "taps": the forward as the
    kernels walk it (bias first, then ci outer, tap inner, one fp32 addition each), the weight gradient as per-chunk partials of 128 output rows
    folded in the fold kernel's order.  fault: None or one of
      "seam_tap"     output position 64 reads tap 0 one input row to the right (the wrong side of the tile seam);
      "fold_tail"    the last partial chunk (last clip, rows from the last multiple of 128 on) is left out of the weight fold;
      "bias_twice"   the bias is added twice in the ConvTranspose1d forward (dx)."""
    x, w, by, bx, dy, lo = c1_inputs(case)
    xt = x.float().transpose(1, 2).contiguous().requires_grad_(True)
    wf = w.float().clone().requires_grad_(True)
    y = TF.conv1d(xt, wf, None, stride=case.stride, padding=case.pad, dilation=case.dil)
    y.backward(dy.float().transpose(1, 2))
    out = {"y": (y.detach().transpose(1, 2) + by), "dx": xt.grad.transpose(1, 2) + bx, "dw": wf.grad, "db_dy": dy.float().sum((0, 1))}
    taps = [_c1_gather(x.float(), case, lo, j) for j in range(case.k)]
    if fault == "seam_tap":
        shifted = torch.zeros_like(x)
        shifted[:, :-1] = x[:, 1:]
        taps[0] = taps[0].clone()
        taps[0][:, 64] = _c1_gather(shifted.float(), case, lo, 0)[:, 64]
    if order == "taps" or fault == "seam_tap":
        acc = by.float().expand(case.b, lo, case.co).clone()
        for ci in range(case.ci):
            for j in range(case.k):
                acc = acc + taps[j][:, :, ci:ci + 1] * w[:, ci, j].float()
        out["y"] = acc
    if order == "taps" or fault == "fold_tail":
        parts = []
        for b in range(case.b):
            for c0 in range(0, lo, 128):
                sl = slice(c0, min(c0 + 128, lo))
                parts.append(torch.stack([dy[b, sl].float().T @ taps[j][b, sl] for j in range(case.k)], dim=2))      # [Co, Ci, k]
        if fault == "fold_tail":
            parts = parts[:-1]
        waves = []
        for wv in range(4):                     # wave wv sums partials wv, wv + 4, ...: four chains of every fourth of those, then the tail
            mine = parts[wv::4]
            full = len(mine) // 4 * 4 if len(mine) >= 4 else 0
            s = [sum(mine[c:full:4], torch.zeros_like(parts[0])) for c in range(4)]
            for p in mine[full:]:
                s[0] = s[0] + p
            waves.append((s[0] + s[1]) + (s[2] + s[3]))
        out["dw"] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    if fault == "bias_twice":
        out["dx"] = out["dx"] + bx
    return out


# =========================================================================================================================================
# 4. LayerNorm backward
# =========================================================================================================================================
LNB_AXES = ("row", "column")
LNB_EPS = 1e-6
LNB_CLASSES = ("uniform", "mean100", "constrow")
LNB_SEED, LNB_OFFSET = 7, 8192
LNB_PLAIN_ROWS = (1, 3, 4, 5, 9)                 # a workgroup is 4 rows (one wave each): one ragged, one full, one into the second and third
LNB_PLAIN_D = (2, 63, 64, 65, 126, 512, 1000)    # fewer columns than lanes; both sides of one lane stride; 126 = the pose width; many strides
LNB_PLAIN_CASES = [(r, d) for d in LNB_PLAIN_D for r in LNB_PLAIN_ROWS]
LNB_EX_D = (64, 128, 448, 512, 576, 1024)        # NV = 2 partial (one quad in 16 lanes / 32 lanes / 112 quads) and full; NV = 4 partial and full
LNB_EX_ROWS = (1, 3, 4, 5, 1023, 1024, 1025, 2049, 8200)


def ln_ex_rows_per_wave(rows):
    return max(1, min(8, cdiv(rows, 4 * 256)))


def ln_ex_workspace_floats(rows, d):
    return cdiv(rows, 4 * ln_ex_rows_per_wave(rows)) * 2 * d


def lnb_ex_cases():
    """(rows, D, rw): every row count at D = 64 and 576, every D at 1, 5 and 1025 rows; 8200 rows (the clamp at 8 rows per wave, the last workgroup's
    waves 1 .. 3 without rows) at D = 64 only."""
    c = [(r, d) for r in LNB_EX_ROWS[:-1] for d in (64, 576)] + [(r, d) for d in LNB_EX_D for r in (1, 5, 1025)] + [(8200, 64)]
    return [(r, d, ln_ex_rows_per_wave(r)) for (r, d) in dict.fromkeys(c)]


LNB_EX_CASES = lnb_ex_cases()


def lnb_inputs(rows, d, cls):
    """-> x, dy, gamma (fp32) and the row classes for the forward tolerance.  uniform: x in (-3, 3); mean100: 100 + (-0.5, 0.5), a large common mean;
    constrow: uniform with the middle row one constant (variance 0: rstd = 1 / sqrt(eps))."""
    key = f"lnb{rows}x{d}"
    dy, g = T(key + "dy", (rows, d)), T(key + "g", (d,), 0.5, 1.5)
    x = T(key + "x", (rows, d), -3, 3)
    row_cls = ["uniform"] * rows
    if cls == "mean100":
        x = 100.0 + T(key + "x", (rows, d), -0.5, 0.5)
        row_cls = ["offset"] * rows
    elif cls == "constrow":
        x[rows // 2] = float(T(key + "c", (1,), 1.0, 3.0))
        row_cls[rows // 2] = "constant"
    elif cls != "uniform":
        raise ValueError(cls)
    return x, dy, g, row_cls


def lnb_f64(x, dy, g, eps=LNB_EPS):
    """float64 autograd -> dx, xhat, dgamma, dbeta."""
    d = x.shape[1]
    xd = x.double().clone().requires_grad_(True)
    gd = g.double().clone().requires_grad_(True)
    bd = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    TF.layer_norm(xd, (d,), gd, bd, eps).backward(dy.double())
    return xd.grad, TF.layer_norm(x.double(), (d,), None, None, eps), gd.grad, bd.grad


def lnb_f32_cpu(x, dy, g, eps=LNB_EPS):
    """torch's float32 CPU layer_norm backward -> dx, dgamma, dbeta."""
    d = x.shape[1]
    xf = x.float().clone().requires_grad_(True)
    gf = g.float().clone().requires_grad_(True)
    bf = torch.zeros(d, requires_grad=True)
    TF.layer_norm(xf, (d,), gf, bf, eps).backward(dy.float())
    return xf.grad, gf.grad, bf.grad


def lnb_dx_scale(x, g, eps=LNB_EPS):
    return layernorm_scale(x, g, torch.zeros_like(g), eps)


# Worst |F.layer_norm(float32, CPU, no affine) - float64| / max(1, |xhat|) at D = 2 per input class (re-measured by tests/test_grads_f64.py).  LN_TOL was
# measured at D >= 3 widths; a row of two values a few ulp apart is outside it (torch's own float32 forward is 9 x over LN_TOL["uniform"] at 9 x 2),
# so at D = 2 xhat is held to 4 x these figures instead, a constant row still to 0.
LN_XHAT_CPU_F32_D2 = {"uniform": 1.10e-5, "mean100": 1.91e-3, "constrow": 1.10e-5}


def measure_ln_xhat_cpu_f32_d2():
    out = {}
    for cls in LNB_CLASSES:
        worst = 0.0
        for rows, d in ln_bwd_case_list("plain2"):
            x = lnb_inputs(rows, d, cls)[0]
            z = TF.layer_norm(x.double(), (d,), None, None, LNB_EPS)
            worst = max(worst, float(((TF.layer_norm(x.float(), (d,), None, None, LNB_EPS).double() - z).abs() / torch.clamp(z.abs(), min=1.0)).max()))
        out[cls] = worst
    return out


def lnb_xhat_tol(x, row_cls, eps=LNB_EPS, cls=None):
    """e_xhat per element: the forward tolerance of small_ops_f64.py for the row's class times max(1, |xhat|); at D = 2 (pass the input class)
    LN_BWD_FACTOR x LN_XHAT_CPU_F32_D2."""
    z = TF.layer_norm(x.double(), (x.shape[1],), None, None, eps)
    if x.shape[1] == 2:
        tol = torch.tensor([0.0 if c == "constant" else LN_BWD_FACTOR * LN_XHAT_CPU_F32_D2[cls] for c in row_cls], dtype=torch.float64)[:, None]
    else:
        tol = torch.tensor([LN_TOL[c] for c in row_cls], dtype=torch.float64)[:, None]
    return tol * torch.clamp(z.abs(), min=1.0)


def lnb_affine_bounds(x, dy, row_cls, eps=LNB_EPS):
    """-> (dgamma bound [D], dbeta bound [D])."""
    rows = x.shape[0]
    _, xhat, dg, db = lnb_f64(x, dy, torch.ones(x.shape[1]), eps)
    dyd = dy.double()
    bb = (rows + 12) * U * dyd.abs().sum(0) + U * db.abs()
    bg = (rows + 12) * U * (dyd * xhat).abs().sum(0) + U * dg.abs() + (dyd.abs() * lnb_xhat_tol(x, row_cls, eps)).sum(0)
    return bg, bb


# Worst |torch float32 CPU layer_norm backward dx - float64| / layernorm_scale per case list and input class (tests/test_grads_f64.py re-measures
# them; worst case in brackets as rows x D).  Every rounding of dx is multiplied by rstd: 1e3 at a constant row, and at D = 2 whatever the distance
# of a row's two values makes it (mean100 at D = 2 has rows whose values differ by one ulp of 100: the class says nothing there but "finite").
#   plain2  uniform 4.57e-4 (9 x 2)      mean100 0.511 (9 x 2)         constrow 4.57e-4 (9 x 2)
#   plain   uniform 1.44e-7 (5 x 1000)   mean100 7.12e-5 (4 x 63)      constrow 2.03e-4 (3 x 1000)
#   ex      uniform 1.70e-7 (2049 x 64)  mean100 1.24e-4 (1025 x 64)   constrow 1.98e-4 (1 x 1024)
LN_BWD_CPU_F32 = {
    "plain2": {"uniform": 4.57e-4, "mean100": 0.511, "constrow": 4.57e-4},
    "plain": {"uniform": 1.44e-7, "mean100": 7.12e-5, "constrow": 2.03e-4},
    "ex": {"uniform": 1.70e-7, "mean100": 1.24e-4, "constrow": 1.98e-4},
}
LN_BWD_FACTOR = 4.0


def ln_bwd_case_list(which):
    """The case lists the dx tolerance is taken per: "plain2" (the plain entry at D = 2, where the two values of a row can lie arbitrarily close and
    rstd, which multiplies every rounding, is large), "plain" (its other widths), "ex"."""
    if which == "ex":
        return [(r, d) for (r, d, _) in LNB_EX_CASES]
    return [(r, d) for (r, d) in LNB_PLAIN_CASES if (d == 2) == (which == "plain2")]


def lnb_dx_tol(which, cls):
    return LN_BWD_FACTOR * LN_BWD_CPU_F32[which][cls]


def measure_ln_bwd_cpu_f32(which):
    """-> {class: (worst error in layernorm_scale units, (rows, D))} of torch's float32 CPU backward over one case list."""
    cases = ln_bwd_case_list(which)
    out = {}
    for cls in LNB_CLASSES:
        worst = (0.0, None)
        for rows, d in cases:
            x, dy, g, _ = lnb_inputs(rows, d, cls)
            e = float(((lnb_f32_cpu(x, dy, g)[0].double() - lnb_f64(x, dy, g)[0]).abs() / lnb_dx_scale(x, g)).max())
            if e > worst[0]:
                worst = (e, (rows, d))
        out[cls] = worst
    return out


def emulate_lnb_affine(x, dy, rw, order="forward", fault=None, eps=LNB_EPS):
    """ln_bwd_ex_kernel's affine sums in float32 -> (dgamma, dbeta): a wave adds its RW rows, four waves fold into a workgroup partial, the partials
    are folded (the kernel folds them in double; fp32 here is the harsher order).  order "reversed" walks rows, waves and partials backwards.
    fault: "xhat_b_last_row" is a dx fault (see emulate_lnb_dx); "dgamma_wave": the rows of wave 1 of workgroup 0 are missing from dgamma."""
    rows, d = x.shape
    xf = x.float()
    mean = xf.mean(1, keepdim=True)
    mean = mean + (xf - mean).mean(1, keepdim=True)
    xc = xf - mean
    xhat = xc * (1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps))
    prod = dy.float() * xhat
    rev = order == "reversed"
    nwave = cdiv(rows, rw)
    wg_g, wg_b = [], []
    for blk in range(cdiv(nwave, 4)):
        pg, pb = [], []
        for wv in range(4):
            r0 = (blk * 4 + wv) * rw
            r1 = min(rows, r0 + rw)
            sg, sb = torch.zeros(d), torch.zeros(d)
            for r in (range(r1 - 1, r0 - 1, -1) if rev else range(r0, r1)):
                sb = sb + dy[r].float()
                if not (fault == "dgamma_wave" and blk == 0 and wv == 1):
                    sg = sg + prod[r]
            pg.append(sg)
            pb.append(sb)
        if rev:
            pg, pb = pg[::-1], pb[::-1]
        wg_g.append(((pg[0] + pg[1]) + pg[2]) + pg[3])
        wg_b.append(((pb[0] + pb[1]) + pb[2]) + pb[3])
    if rev:
        wg_g, wg_b = wg_g[::-1], wg_b[::-1]
    dg, db = torch.stack(wg_g), torch.stack(wg_b)
    return dg.cumsum(0)[-1], db.cumsum(0)[-1]


def emulate_lnb_dx(x, dy, g, rw, fault=None, eps=LNB_EPS):
    """dx in float32 by the kernel's formula (g dy - a - xhat b) rstd; fault "xhat_b_last_row": the xhat b term is omitted for the last row of every
    wave's walk (rows r with r % rw == rw - 1, and the last row)."""
    xf, d = x.float(), x.shape[1]
    mean = xf.mean(1, keepdim=True)
    mean = mean + (xf - mean).mean(1, keepdim=True)
    xc = xf - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xhat = xc * rstd
    gd = g.float() * dy.float()
    a, b = gd.mean(1, keepdim=True), (gd * xhat).mean(1, keepdim=True)
    xb = xhat * b
    if fault == "xhat_b_last_row":
        last = (torch.arange(x.shape[0]) % rw == rw - 1) | (torch.arange(x.shape[0]) == x.shape[0] - 1)
        xb[last] = 0.0
    return (gd - a - xb) * rstd
