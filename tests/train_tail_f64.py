"""Test-side float64 restatements of the rest of csrc/train.hip -- train-mode BatchNorm (five entry points), the losses, eg_kld and
eg_reparameterize, the two memory gates, Adam, the bf16 payload conversion and the segment operators -- with the bound every ELEMENT of their
results is held to, the case lists of the GPU tests (a reason per case, the kernel route it takes stated and checked against a restatement of
col_reduce / col_sums / launch_bn_apply / launch_adam), and CPU emulations of the kernels' fp32 arithmetic in two summation orders
(tests/test_train_tail_f64.py).  A helper module (not collected: no test_ prefix); CPU only.  T, U, compare_sliced, sliced_errors are those of
tests/small_ops_f64.py.  The reference is always torch float64 on the CPU of the same fp32 inputs; scalar hyper-parameters enter it as the fp32
values the ABI receives (f32()).  u = 2^-24 below; "fn" = 4 u is the allowance for one expf / logf / powf (2 ulp).  A single rounding can reach u |ref|
on its own, and correct arithmetic is asked to stay at HALF of every bound, so where roundings are counted one by one (the elementwise results, the
value stored last) each enters as 2 u.

1. BatchNorm, train mode (x [rows, C], channel statistics over the rows)
    plan        bn_plan restates col_reduce: fast (C >= 4, C | 1024, 16-byte aligned) or generic, nblk, rows_per, and from them the longest fp32
                chain L (the additions one thread makes plus the lane combine) and the number of folded partials Z; bwd_plan restates col_sums
                (col_direct when C % 4 == 0, rows <= 1024, aligned).  K = L + Z + 8 everywhere below.
    mean        2 u |mean| + K u sum|x - mean| / rows.  The kernels take the mean in two steps (first-pass mean m0 from fp32 chains, then the sum of
                the residuals x - m0 in the centred pass corrects it): the error scales with the spread, not with the magnitude, and a constant
                channel gets its value to the rounding.  One-step arithmetic (mean = sum / rows from the fp32 chains) misses this bound: a constant
                100.3 over 3712 rows of the generic route comes out 100.300026, 4 ulp off, i.e. y - beta = -7e-3 gamma where float64 has 0.
    var         (K + 8) u (var + e0^2) + u var, e0 = K u sum|x| / rows the error of m0 (second order): sum of squares of the residuals, no
                cancellation.  rstd carries it to first order with its remainder: e_rstd = 0.5 rstd^3 e_var (1 + 2 t) + 2 u rstd (_rstd_err).
    running     unbiased variance var rows / (rows - 1) (rows = 1: the biased one), momentum in fp32:
                e = mom e_stat + 4 u (|(1 - mom) old| + |mom stat|) + u |ref|.
    y, aff_*    e_y = |gamma| (rstd e_mean + |x - mean| e_rstd) + 5 u |gamma| rstd |x - mean| + 2 u |y| + u |beta|; aff_scale = gamma rstd and
                aff_shift = beta - mean aff_scale carry e_mean and e_rstd the same way.
    dbeta       K u sum|dy| + u |ref|;   dgamma = rstd sum dy (x - mean): rstd K u sum|dy (x - mean)| + 2 u |ref|  (save_mean / save_rstd are INPUTS
                of the backward: the float64 reference uses the fp32 values the kernel is given).
    dx          suffers cancellation (dy - mean(dy) - xhat mean(dy xhat)); as for the LayerNorm backward (grads_f64.py) the tolerance is
                BN_DX_FACTOR = 4 x the error of torch's own float32 CPU batch-norm backward against float64 on the same inputs, per input class, in
                units of |gamma| rstd rms_rows(dy) (BN_DX_CPU_F32; tests/test_train_tail_f64.py re-measures it and fails when stale by > 2 x).  It is
                measured against the reference, never against the kernel.  With relu_mask = 1, dx is +0 bitwise wherever x <= 0.
    _gap        the first-pass mean comes from the caller's per-tile sums; the centred pass corrects it, so the bounds are those above.
    _sq, stats  no pass over the map, no correction possible.  The test makes the per-tile sums and sums of squares in float64 and rounds each
                ONCE to fp32 (relative u); everything after is double in the kernels.  So e_mean = 2 u sum|gap| / rows + u |mean| and
                e_var = 2 u (sum|gap_sq| + 2 |mean| sum|gap|) / rows + u var = ~2 u var (1 + 3 mean^2 / var): the conditioning the kernels' header
                states (~1e-6 (1 + mean^2 / var)), with the constant derived from one rounding per tile sum (x 2 so that correct arithmetic, whose
                single rounding may reach u at one tile, stays at half).
2. eg_smooth_l1   inputs on the dyadic grid 1/64, so d = pred - target is exact and elements with |d| = beta, d = 0 and d = -0 exist.
                dpred 4 u |ref| (two roundings: scale / n and the product; d / beta is exact on the grid);  loss (L + 12) u sum|term| |scale| / n + 2 u |ref|, L = the per-thread
                chain + the 8-level tree.  NOTE: at |d| = beta both branches give the same value AND the same derivative (0.5 beta; +-1): torch's `<`
                and a `<=` are bitwise indistinguishable on any input (test_smooth_l1_branch_at_beta_is_value_neutral shows it on the grid), so no
                test can demand the linear branch there; the detectable single-site fault of this operator is a threshold that ignores beta.
3. eg_cross_entropy   rho_i = fn + u |z_i - m| (an argument error is a relative error of exp), rho_se = max_i rho_i + (ceil(C / 64) + 8) u,
                e_logp = 2 u |z_y - m| + rho_se + fn |log se| + 2 u |logp|;  e_pt = pt (e_logp + fn);  the cancellation of 1 - pt is carried
                explicitly: e_om = 2 u + e_pt (absolute);  w = om^gamma: e_w = gamma om^(gamma-1) e_om + e_om^2 [gamma = 2] + fn w;
                row loss a (e_w ce + w e_logp) + 4 u |loss|;  dce and dlogits carry the same terms through the product rule (ce_bounds).
                In the pt -> 1 class (label 30 above the rest) fp32 has se = 1, logp = 0, 1 - pt = 0 exactly where float64 has ~C e^-30: the focal
                row loss is 0 against ~1e-24, a RELATIVE error of 1.0, and inside the absolute bound above -- which correct fp32 arithmetic of the
                reference formula (1 - exp(logp)) meets with the same zero, so -expm1f(logp) is not needed and the kernel keeps the formula.
4. eg_kld / eg_reparameterize   term = 1 + l - m^2 - e^l with A = 1 + |l| + m^2 + e^l: loss 0.5 |k| (L + 16) u sum A + 3 u |ref| (one workgroup:
                L = ceil(n d / 256) + 8); dmu 4 u |ref| (two roundings); dlogvar 0.5 |k| (5 u e^l + u) + 4 u |ref|; z = eps e^(l/2) + mu: 7 u |eps| e^(l/2) + 2 u |z| + u |mu|.
                (There is no reparameterisation-backward entry point: the training layer composes it from eg_elementwise.)
5. gates        sp: e_dot = (ceil(D/64) + 14) u sum|m p|; e_s = s (1 - s) (e_dot + fn) + 3 u s + 2^-126 (a flushed denormal); out, and in the
                backward (gate is an INPUT) ds, dscore, dp, dm by the product rule (sp_bounds, sp_bwd_bounds).  tm: softmax as in 3 with a
                sequential chain over chunk; dscore = w (dw - sum w dw), and sum_c dscore = 0 within sum_c e_dscore.
6. Adam         one step in float64 with fp32 hyper-parameters and the exact bias corrections of those; e_g = 2 u (|g| + |wd p|);
                e_m = (1 - b1) e_g + 4 u (|b1 m| + |(1 - b1) g'|); e_v = 2 (1 - b2) |g'| e_g + 5 u (b2 v + (1 - b2) g'^2); the step carries them through
                sqrt, the two divisions and lr / bc1 (adam_bounds).  adam_plan restates launch_adam: float4 kernel when the four slices share a
                16-byte phase and n >= 8 (head / n4 / tail / workgroups), else the scalar kernel.
7. bf16 payload   bitwise torch's cast on every finite value and +-inf; NaN must stay NaN.  bf16_rne_bits restates csrc/common.h f32_to_bf16_rne.
8. segment ops    seg_mean / seg_dot: (L + Z + 8) u sum|terms| |scale| + 2 u |ref| with L, Z from seg_plan; se_scale: 2 u |a g| + 2 u |y|.

Worst element of correct arithmetic (the emulations, both orders) as a fraction of its bound: WORST_OF_CORRECT_ARITHMETIC below.

Worst element seen on the MI355X as a fraction of its bound or tolerance (the GPU tests print theirs as FRACTION lines; also GPU_WORST_FRACTIONS):
    eg_bn_train_forward      save_mean 0.33   save_rstd 0.35   running_mean 0.36   running_var 0.42   y 0.33
    eg_bn_train_backward     dx 0.26 (of 4 x the float32 CPU error)   dgamma 0.09   dbeta 0.11
    eg_bn_train_forward_gap  save_mean 0.30   save_rstd 0.35   running_mean 0.26   running_var 0.34   y 0.30   clip_sum 0.17
    eg_bn_train_forward_sq   save_mean 0.49   save_rstd 0.36 (0.36 in the variance domain)   running_mean 0.40   running_var 0.40   y 0.30
    eg_bn_train_stats_sq     aff_scale 0.42   aff_shift 0.34
    eg_smooth_l1 loss 0.05, dpred 0.42      eg_cross_entropy rowloss 0.26, loss 0.18, dlogits 0.38      eg_kld loss 0.04, dmu 0.43, dlogvar 0.40
    eg_reparameterize 0.33                  eg_sp_gate out 0.48, gate 0.22, dpred 0.16, dmem 0.09       eg_tm_scale out 0.45, w 0.40, dpred 0.42, dscore 0.04
    eg_adam_step / _dev p 0.50, m 0.27, v 0.31 (p: the one rounding of the stored value against its 2 u)           eg_seg_mean 0.09, eg_seg_dot 0.07, eg_se_scale 0.49
Defects these tests found, both confirmed on the device and fixed: f32_to_bf16_rne had no NaN case (0x7FFFFFFF -> -0, 0xFFFFFFFF -> +0,
0x7F800001 -> +inf; test_gpu_segment_ops_f64.py::test_f32_to_bf16_keeps_nan); the BatchNorm forward took a one-step mean (see `mean` above: save_mean
1.9 x its bound on the constant channel of every generic case from 127 rows up and 1.2-1.3 x on the mean-100 class of the fast path;
test_gpu_batchnorm_f64.py::test_two_pass_forward_matches_float64_per_element).
"""
from collections import namedtuple

import numpy as np
import torch

from small_ops_f64 import T, U, compare_sliced, sliced_errors  # noqa: F401  (re-exported for the tests)

FN = 4.0 * U
FLT_MIN = 2.0 ** -126
COL_MAX_PART = 2048

# Worst element of correct arithmetic as a fraction of its bound over every case (tests/test_train_tail_f64.py measures, prints and holds each
# to <= 0.5 and to these figures, which are its own rounded up):
WORST_OF_CORRECT_ARITHMETIC = {
    "bn mean": 0.33, "bn rstd": 0.35, "bn running_mean": 0.36, "bn running_var": 0.42, "bn y": 0.35, "bn dbeta": 0.11, "bn dgamma": 0.10, "bn dx": 0.29,
    "bn_gap mean": 0.30, "bn_gap rstd": 0.35, "bn_sq mean": 0.49, "bn_sq rstd": 0.36, "bn_sq var": 0.36, "bn_sq running_mean": 0.40,
    "bn_sq running_var": 0.40, "bn_sq y": 0.35, "bn_sq aff": 0.42,
    "smooth_l1 loss": 0.05, "smooth_l1 dpred": 0.42, "ce rowloss": 0.26, "ce loss": 0.12, "ce dlogits": 0.37,
    "kld loss": 0.04, "kld grads": 0.43, "reparam": 0.33, "sp out": 0.48, "sp gate": 0.22, "sp dp": 0.29, "sp dm": 0.10,
    "tm out": 0.45, "tm w": 0.40, "tm dp": 0.42, "tm dscore": 0.06, "adam p": 0.50, "adam m": 0.36, "adam v": 0.41,
    "seg_mean": 0.11, "seg_dot": 0.12, "se_scale": 0.49,
}
# Worst element on the MI355X as a fraction of its bound / tolerance, per operator (the FRACTION lines of the GPU modules):
GPU_WORST_FRACTIONS = {
    "bn_forward save_mean": 0.33, "bn_forward save_rstd": 0.35, "bn_forward running_mean": 0.36, "bn_forward running_var": 0.42, "bn_forward y": 0.33,
    "bn_backward dx": 0.26, "bn_backward dgamma": 0.09, "bn_backward dbeta": 0.11,
    "bn_gap save_mean": 0.30, "bn_gap save_rstd": 0.35, "bn_gap running_mean": 0.26, "bn_gap running_var": 0.34, "bn_gap y": 0.30, "bn_gap clip_sum": 0.17,
    "bn_sq save_mean": 0.49, "bn_sq save_rstd": 0.36, "bn_sq rstd as variance": 0.36, "bn_sq running_mean": 0.40, "bn_sq running_var": 0.40, "bn_sq y": 0.30,
    "bn_stats_sq aff_scale": 0.42, "bn_stats_sq aff_shift": 0.34,
    "smooth_l1 loss": 0.05, "smooth_l1 dpred": 0.42, "cross_entropy rowloss": 0.26, "cross_entropy loss": 0.18, "cross_entropy dlogits": 0.38,
    "kld loss": 0.04, "kld dmu": 0.43, "kld dlogvar": 0.40, "reparameterize": 0.33,
    "sp_gate out": 0.48, "sp_gate gate": 0.22, "sp_gate dpred": 0.16, "sp_gate dmem": 0.09,
    "tm_scale out": 0.45, "tm_scale w": 0.40, "tm_scale dpred": 0.42, "tm_scale dscore": 0.04,
    "adam p": 0.50, "adam m": 0.27, "adam v": 0.31, "seg_mean": 0.09, "seg_dot": 0.07, "se_scale": 0.49,
}


def cdiv(a, b):
    return -(-a // b)


def f32(v):
    """The fp32 value the C ABI receives for a float argument, as a Python float."""
    return float(np.float32(v))


def worst(got, ref, bound):
    """Worst element of |got - ref| as a fraction of its bound (inf for a non-finite result)."""
    if torch.as_tensor(ref).numel() == 0:
        return 0.0
    if not bool(torch.isfinite(torch.as_tensor(got).double()).all()):
        return float("inf")
    return sliced_errors(torch.as_tensor(got), torch.as_tensor(ref), torch.as_tensor(bound), [f"axis {i}" for i in range(torch.as_tensor(ref).dim())])[2][0]


# =========================================================================================================================================
# 1. BatchNorm
# =========================================================================================================================================
BN_AXES = ("row", "channel")
BN_CLASSES = ("uniform", "offset", "decades", "const_zero")
BN_EPS = 1e-5
ColPlan = namedtuple("ColPlan", "route nblk rows_per lanes L Z")


def bn_plan(rows, c, aligned=True, nseg=1):
    """col_reduce of csrc/train.hip -> ColPlan.  fast: thread t of a block reads the float4 stream at t, t + 256, ...: the rows j, j + 1024 / C, ...
    of its channel quad (lanes = 1024 / C row lanes per block, combined one after the other); generic: four waves take rows w, w + 4, ...
    (lanes = 4).  L = chain + lane combine, Z = partials folded (in double)."""
    fast = c >= 4 and 1024 % c == 0 and aligned
    cap = max(1, COL_MAX_PART // nseg)
    nblk = cdiv(rows * c, 16384) if fast else cdiv(rows, 128)
    nblk = max(1, min(nblk, cap))
    rows_per = cdiv(rows, nblk)
    nblk = cdiv(rows, rows_per)
    lanes = 1024 // c if fast else 4
    return ColPlan("fast" if fast else "generic", nblk, rows_per, lanes, cdiv(rows_per, lanes) + lanes, nblk)


def bwd_plan(rows, c, aligned=True):
    """col_sums: one col_direct launch (16 row lanes per 64 columns, no partials) when C % 4 == 0, rows <= 1024 and everything is aligned."""
    if c % 4 == 0 and rows <= 1024 and aligned:
        return ColPlan("direct", 1, rows, 16, cdiv(rows, 16) + 16, 0)
    return bn_plan(rows, c, aligned)


def apply_route(c, aligned=True):
    """launch_bn_apply / the backward's apply: float4 when C % 4 == 0 and every operand is 16-byte aligned."""
    return "float4" if c % 4 == 0 and aligned else "scalar"


BnCase = namedtuple("BnCase", "rows c aligned fwd bwd apply why")
# (rows, C, aligned) with the forward reduction route, the backward reduction route and the apply form each takes.  Every route of the issue's C
# list and every loop tail of its rows list appears once; (3712, 34) is the long generic chain of the one-step-mean defect.
BN_CASES = [
    BnCase(1, 34, True, "generic", "generic", "scalar", "rows = 1: variance 0, biased running variance; C % 4 = 2"),
    BnCase(2, 60, True, "generic", "direct", "float4", "two rows; generic partials with the float4 apply"),
    BnCase(29, 120, True, "generic", "direct", "float4", "r + 28 < r1 is never true: the tail loop alone"),
    BnCase(33, 34, True, "generic", "generic", "scalar", "r + 28 < r1 holds once for every wave, then the tail"),
    BnCase(127, 130, True, "generic", "generic", "scalar", "one generic row block; three 64-column blocks, the last with 2 live columns"),
    BnCase(129, 34, True, "generic", "generic", "scalar", "two generic row blocks (65 + 64 rows)"),
    BnCase(3712, 34, True, "generic", "generic", "scalar", "29 generic row blocks: the chain length of the one-step-mean defect"),
    BnCase(520, 64, True, "fast", "direct", "float4", "three fast blocks of 174 rows, the last partial (172)"),
    BnCase(1024, 4, True, "fast", "direct", "float4", "fast path, C = 4 (256 row lanes); the col_direct limit of the backward"),
    BnCase(1025, 4, True, "fast", "fast", "float4", "one row past the col_direct limit: the backward takes the fast partials"),
    BnCase(1024, 60, True, "generic", "direct", "float4", "generic forward, col_direct backward at its limit"),
    BnCase(1025, 60, True, "generic", "generic", "float4", "one row past the limit: generic partials in the backward"),
    BnCase(129, 32, True, "fast", "direct", "float4", "fast path, C = 32"),
    BnCase(33, 256, True, "fast", "direct", "float4", "fast path, C = 256 (4 row lanes)"),
    BnCase(29, 1024, True, "fast", "direct", "float4", "fast path, nq = 256: one contributor per quad"),
    BnCase(130, 64, False, "generic", "generic", "scalar", "every operand offset by one float: misalignment forces generic + scalar"),
]


def bn_inputs(rows, c, cls):
    """-> x, gamma, beta, dy, running_mean, running_var (fp32).  uniform: centred (-1, 1); offset: 100 + (-1.7, 1.7) (unit spread, post-ReLU-like);
    decades: the columns scaled over logspace(-2, 1); const_zero: channel c // 2 constant 100.3 and the last channel all zero in a random map."""
    key = f"bn{rows}x{c}{cls}"
    x = T(key + "x", (rows, c))
    if cls == "offset":
        x = (100.0 + 1.7 * x.double()).float()
    elif cls == "decades":
        x = (x.double() * torch.logspace(-2, 1, c, dtype=torch.float64)).float()
    elif cls == "const_zero":
        x[:, c // 2] = 100.3
        x[:, c - 1] = 0.0
    elif cls != "uniform":
        raise ValueError(cls)
    g = T(key + "g", (c,), 0.5, 1.5) * torch.where(torch.arange(c) % 3 == 1, -1.0, 1.0)
    return x, g, T(key + "b", (c,), -0.5, 0.5), T(key + "dy", (rows, c)), T(key + "rm", (c,), -0.5, 0.5), T(key + "rv", (c,), 0.5, 1.5)


def bn_forward_f64(x, g, b, rm, rv, mom, eps=BN_EPS):
    X, rows = x.double(), x.shape[0]
    mean = X.mean(0)
    var = (X - mean).pow(2).mean(0)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    unb = var * rows / (rows - 1) if rows > 1 else var
    m = f32(mom)
    return {"y": (X - mean) * rstd * g.double() + b.double(), "mean": mean, "rstd": rstd, "var": var,
            "running_mean": (1.0 - m) * rm.double() + m * mean, "running_var": (1.0 - m) * rv.double() + m * unb}


def _rstd_err(var, e_var, eps):
    """|d rstd| <= 0.5 rstd^3 e_var (1 + 2 t) for t = e_var / (var + eps) <= 0.1 ((1 - t)^-1/2 - 1 <= 0.5 t (1 + 2 t) there), linear in e_var so that half
    the variance bound is half of this one; past t = 0.1 (a channel whose mean^2 / var exhausts fp32 in the _sq routes) rstd is a saturating
    function of the error and is held in the variance domain instead (sq_var_of): the bound here is inf."""
    r = 1.0 / torch.sqrt(var + eps)
    t = e_var / (var + eps)
    return torch.where(t <= 0.1, 0.5 * r ** 3 * e_var * (1 + 2 * t), torch.full_like(r, float("inf"))) + 2 * U * r


def _derived_bounds(x, g, b, rm, rv, mom, eps, ref, e_mean, e_var):
    """rstd, running statistics, y and the folded affine from the bounds of mean and variance."""
    X, rows = x.double(), x.shape[0]
    m = f32(mom)
    e_rstd = _rstd_err(ref["var"], e_var, f32(eps))
    unb_f = rows / (rows - 1) if rows > 1 else 1.0
    dev = (X - ref["mean"]).abs()
    ga = g.double().abs()
    dev_e = torch.where(torch.isinf(e_rstd), e_rstd, dev * torch.nan_to_num(e_rstd, posinf=0.0))
    scale = g.double() * ref["rstd"]
    e_scale = ga * e_rstd + 2 * U * scale.abs()
    return {
        "mean": e_mean, "rstd": e_rstd, "var": e_var + 4 * U * (ref["var"] + f32(eps)),
        "running_mean": m * e_mean + 4 * U * (((1 - m) * rm.double()).abs() + (m * ref["mean"]).abs()) + U * ref["running_mean"].abs(),
        "running_var": m * (e_var * unb_f + U * ref["var"] * unb_f) + 4 * U * (((1 - m) * rv.double()).abs() + m * ref["var"] * unb_f) + U * ref["running_var"].abs(),
        "y": ga * (ref["rstd"] * e_mean + dev_e) + 5 * U * ga * ref["rstd"] * dev + 2 * U * ref["y"].abs() + U * b.double().abs(),
        "aff_scale": e_scale,
        "aff_shift": ref["mean"].abs() * e_scale + scale.abs() * e_mean + 2 * U * (b.double().abs() + (ref["mean"] * scale).abs()),
    }


def bn_forward_bounds(x, g, b, rm, rv, mom, plan, eps=BN_EPS):
    """The two-pass and the _gap entry points (module docstring: mean, var and what derives from them)."""
    X, rows = x.double(), x.shape[0]
    ref = bn_forward_f64(x, g, b, rm, rv, mom, eps)
    K = plan.L + plan.Z + 8
    e_mean = 2 * U * ref["mean"].abs() + K * U * (X - ref["mean"]).abs().sum(0) / rows
    e0 = K * U * X.abs().sum(0) / rows
    e_var = (K + 8) * U * (ref["var"] + e0 * e0) + U * ref["var"]
    return ref, _derived_bounds(x, g, b, rm, rv, mom, eps, ref, e_mean, e_var)


def bn_backward_f64(x, dy, g, mean32, rstd32):
    """The backward's contract on the fp32 save_mean / save_rstd it is GIVEN."""
    X, D, rows = x.double(), dy.double(), x.shape[0]
    m, r = mean32.double(), rstd32.double()
    sdy, sdyx = D.sum(0), (D * (X - m)).sum(0)
    xh = (X - m) * r
    return {"dx": g.double() * r * (D - sdy / rows - xh * (r * sdyx) / rows), "dbeta": sdy, "dgamma": r * sdyx}


def bn_backward_bounds(x, dy, g, mean32, rstd32, plan):
    X, D = x.double(), dy.double()
    m, r = mean32.double(), rstd32.double()
    ref = bn_backward_f64(x, dy, g, mean32, rstd32)
    K = plan.L + plan.Z + 8
    return ref, {"dbeta": K * U * D.abs().sum(0) + U * ref["dbeta"].abs(),
                 "dgamma": r * K * U * (D * (X - m)).abs().sum(0) + 2 * U * ref["dgamma"].abs()}


def bn_dx_unit(dy, g, rstd32):
    """The per-element unit of a dx error: |gamma_c| rstd_c rms_rows(dy[:, c]) (at least 2^-126)."""
    rms = dy.double().pow(2).mean(0).sqrt()
    return torch.clamp(g.double().abs() * rstd32.double() * rms, min=FLT_MIN).expand(dy.shape)


# Worst |torch float32 CPU batch-norm backward - bn_backward_f64| / bn_dx_unit per input class over BN_CASES (test_train_tail_f64.py re-measures
# them: native_batch_norm_backward on the [rows, C] map with the same fp32 save_mean / save_rstd).  Worst case (rows x C) in brackets:
#   uniform 3.15e-7 (29 x 1024)    offset 3.50e-7 (127 x 130)    decades 3.30e-7 (33 x 256)    const_zero 3.81e-7 (129 x 32)
BN_DX_CPU_F32 = {"uniform": 3.15e-7, "offset": 3.50e-7, "decades": 3.30e-7, "const_zero": 3.81e-7}
BN_DX_FACTOR = 4.0


def bn_dx_tol(cls):
    return BN_DX_FACTOR * BN_DX_CPU_F32[cls]


def bn_dx_cpu_float32(x, dy, g, mean32, rstd32):
    gi = torch.ops.aten.native_batch_norm_backward(dy, x, g, None, None, mean32, rstd32, True, BN_EPS, [True, True, True])
    return gi[0]


# ---- emulation of the two-level column reduction -------------------------------------------------------------------------------------------
def _chains(t, plan, order, drop_last=False):
    """sum over the rows of fp32 terms t [rows, C] as the plan orders it: per block, `lanes` fp32 chains over rows j, j + lanes, ..., the lanes
    combined one after the other in fp32, the block partials folded in float64.  order "forward" | "reversed" (chains and lane combine run
    backwards)."""
    t = np.ascontiguousarray(t, dtype=np.float32)
    rows, c = t.shape
    nblk, rp, nl = plan.nblk, plan.rows_per, plan.lanes
    kmax = cdiv(rp, nl)
    buf = np.zeros((nblk, kmax * nl, c), np.float32)
    for i in range(nblk):
        seg = t[i * rp:min(rows, (i + 1) * rp)]
        buf[i, :len(seg)] = seg
    buf = buf.reshape(nblk, kmax, nl, c)
    acc = np.zeros((nblk, nl, c), np.float32)
    for k in (range(kmax) if order == "forward" else reversed(range(kmax))):
        acc = acc + buf[:, k]
    part = np.zeros((nblk, c), np.float32)
    for j in (range(nl) if order == "forward" else reversed(range(nl))):
        part = part + acc[:, j]
    if drop_last and nblk > 1:
        part = part[:-1]
    return part.astype(np.float64).sum(0)


def emulate_bn_forward(x, g, b, rm, rv, mom, plan, order="forward", fault=None, eps=BN_EPS, m0=None):
    """The forward's fp32 data flow.  m0: a first-pass mean given from outside (the _gap entry point).  faults: "one_step_mean" (the arithmetic
    before the two-step mean), "drop_last_chunk", "col64_from_col0" (channel 64 normalised with channel 0's statistics), "biased_running_var"."""
    X = x.numpy().astype(np.float32)
    rows, c = X.shape
    drop = fault == "drop_last_chunk"
    if m0 is None:
        m0 = (_chains(X, plan, order, drop) / rows).astype(np.float32)
    d = X - m0[None, :]
    q, s = _chains(d * d, plan, order, drop), _chains(d, plan, order, drop)
    if fault == "one_step_mean":
        mean, var = m0, q / rows
    else:
        dm = s / rows
        mean = (m0.astype(np.float64) + dm).astype(np.float32)
        var = np.maximum(q / rows - dm * dm, 0.0)
    rstd = (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)
    unb = var if (rows == 1 or fault == "biased_running_var") else var * rows / (rows - 1)
    mo = np.float32(mom)
    one = np.float32(1.0)
    ms, rs = mean.copy(), rstd.copy()
    if fault == "col64_from_col0" and c > 64:
        ms[64], rs[64] = ms[0], rs[0]
    y = (X - ms[None, :]) * rs[None, :] * g.numpy()[None, :] + b.numpy()[None, :]
    out = {"y": y, "mean": mean, "rstd": rstd, "running_mean": (one - mo) * rm.numpy() + mo * mean,
           "running_var": (one - mo) * rv.numpy() + mo * unb.astype(np.float32)}
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in out.items()}


def emulate_bn_backward(x, dy, g, mean32, rstd32, plan, order="forward", fault=None):
    X, D = x.numpy(), dy.numpy()
    rows = X.shape[0]
    m, r, ga = mean32.numpy(), rstd32.numpy(), g.numpy()
    drop = fault == "drop_last_chunk"
    sdy = _chains(D, plan, order, drop).astype(np.float32)
    sdyx = _chains(D * (X - m[None, :]), plan, order, drop).astype(np.float32)
    inv = np.float32(1.0) / np.float32(rows)
    xh = (X - m[None, :]) * r[None, :]
    dx = ga[None, :] * r[None, :] * (D - (sdy * inv)[None, :] - xh * (r * sdyx)[None, :] * inv)
    return {"dx": torch.from_numpy(dx.astype(np.float32)), "dbeta": torch.from_numpy(sdy), "dgamma": torch.from_numpy(r * sdyx)}


# ---- partial-fed entry points ---------------------------------------------------------------------------------------------------------------
GAP_C = (4, 32, 256)
GAP_BATCH = (1, 3, 65)
GAP_PIXELS = 5                      # pixels per tile of the test maps (the tower's tiles hold <= 256)


def gap_tiles(c):
    return (1, 3, 256 // c + 1)     # one tile; fewer than / one more than the 256 / C tile groups of clip_sum_from_gap


def gap_cases():
    """(batch, tiles, C): every C with every tile count at batch 3, every batch at tiles 3."""
    return sorted({(3, t, c) for c in GAP_C for t in gap_tiles(c)} | {(bt, 3, c) for c in GAP_C for bt in GAP_BATCH})


def gap_inputs(batch, tiles, c, cls):
    """-> the BatchNorm inputs of a [batch * tiles * GAP_PIXELS, C] map plus gap, gap_sq [batch, tiles, C]: the per-tile sums and sums of squares in
    float64, each rounded once to fp32."""
    rows = batch * tiles * GAP_PIXELS
    x, g, b, dy, rm, rv = bn_inputs(rows, c, cls)
    xt = x.double().view(batch, tiles, GAP_PIXELS, c)
    return x, g, b, rm, rv, xt.sum(2).float(), xt.pow(2).sum(2).float()


def clip_sum_bound(gap):
    tiles = gap.shape[1]
    return (tiles + 8) * U * gap.double().abs().sum(1) + U * gap.double().sum(1).abs()


def bn_sq_bounds(x, g, b, rm, rv, mom, gap, gap_sq, eps=BN_EPS):
    rows = x.shape[0]
    ref = bn_forward_f64(x, g, b, rm, rv, mom, eps)
    sg, sq = gap.double().abs().sum((0, 1)), gap_sq.double().abs().sum((0, 1))
    e_mean = 2 * U * sg / rows + U * ref["mean"].abs()
    e_var = 2 * U * (sq + 2 * ref["mean"].abs() * sg) / rows + U * ref["var"]
    return ref, _derived_bounds(x, g, b, rm, rv, mom, eps, ref, e_mean, e_var)


def sq_var_of(rstd32, eps=BN_EPS):
    """rstd in the variance domain: 1 / rstd^2 - eps, held to e_var + 4 u (var + eps) (the rounding of rstd doubled, twice)."""
    return 1.0 / rstd32.double() ** 2 - f32(eps)


def emulate_bn_sq(x, g, b, rm, rv, mom, gap, gap_sq, eps=BN_EPS):
    """bn_finalize_sq_kernel: double sums of the fp32 partials, E[x^2] - mean^2 in double, rounded to fp32 once."""
    rows = x.shape[0]
    m = gap.double().sum((0, 1)) / rows
    var = torch.clamp(gap_sq.double().sum((0, 1)) / rows - m * m, min=0.0)
    mean, rstd = m.float(), (1.0 / torch.sqrt(var + f32(eps))).float()
    unb = var * rows / (rows - 1) if rows > 1 else var
    mo = torch.tensor(mom, dtype=torch.float32)
    scale = rstd * g
    return {"mean": mean, "rstd": rstd, "running_mean": (1 - mo) * rm + mo * mean, "running_var": (1 - mo) * rv + mo * unb.float(),
            "y": (x - mean) * rstd * g + b, "aff_scale": scale, "aff_shift": b - mean * scale}


# =========================================================================================================================================
# 2. smooth-L1
# =========================================================================================================================================
SL1_N = (1, 255, 257, 262147)       # 262147 = 1024 * 256 + 3: every one of the 1024 blocks strides twice at least once
SL1_BETA = (1.0, 0.25)


def sl1_blocks(n):
    return min(cdiv(n, 256), 1024)


def sl1_inputs(n):
    """pred, target on the grid 1/64 in [-2, 2]; the first elements are d = +-beta for both betas, d = 0 and d = -0."""
    p = torch.round(T(f"sl1p{n}", (n,), -2, 2) * 64) / 64
    t = torch.round(T(f"sl1t{n}", (n,), -2, 2) * 64) / 64
    fixed = [(1.5, 0.5), (0.5, 1.5), (0.75, 0.5), (0.5, 0.75), (0.5, 0.5), (-0.0, 0.0), (0.0, -0.0)]
    for i, (a, c) in enumerate(fixed[:n] if n > 1 else fixed[:1]):
        p[i], t[i] = a, c
    return p, t


def sl1_eval(pred, target, beta, scale, dt=torch.float64, flip=False, fault=None):
    p, t, n = pred.to(dt), target.to(dt), pred.numel()
    be = torch.tensor(f32(beta), dtype=dt)
    d = p - t
    ad = d.abs()
    lin = ad >= be
    if fault == "branch_le":
        lin = ad > be
    if fault == "beta_ignored":
        lin = ad >= 1.0
    terms = torch.where(lin, ad - 0.5 * be, 0.5 * d * d / be)
    k = torch.tensor(f32(scale), dtype=dt) / torch.tensor(float(n), dtype=dt)
    dp = k * torch.where(lin, torch.where(d > 0, 1.0, -1.0).to(dt), d / be)
    s = (terms.flip(0) if flip else terms).sum()
    return s.double() * (f32(scale) / n), dp


def sl1_bounds(pred, target, beta, scale):
    n = pred.numel()
    loss, dp = sl1_eval(pred, target, beta, scale)
    d = pred.double() - target.double()
    be = f32(beta)
    terms = torch.where(d.abs() >= be, d.abs() - 0.5 * be, 0.5 * d * d / be)
    L = cdiv(n, sl1_blocks(n) * 256) + 8
    return (L + 12) * U * terms.abs().sum() * abs(f32(scale)) / n + 2 * U * loss.abs(), 4 * U * dp.abs()


# =========================================================================================================================================
# 3. cross entropy / focal
# =========================================================================================================================================
CE_B = (1, 6, 70)
CE_C = (1, 6, 64, 65, 130)
CE_GAMMA = (-1.0, 0.0, 1.0, 2.0)
CE_CLASSES = ("uniform", "label_above", "label_below", "tie", "shifted")


def ce_inputs(B, C, cls):
    key = f"ce{B}x{C}{cls}"
    z = T(key + "z", (B, C), -4, 4)
    y = (torch.arange(B) * 7 + 3) % C
    if cls == "label_above":
        z[torch.arange(B), y] += 30.0
    elif cls == "label_below":
        z[torch.arange(B), y] -= 30.0
    elif cls == "tie":
        z[:, 0] = 4.0
        z[:, C - 1] = 4.0
    elif cls == "shifted":
        z = z + 1e4
    return z, y.long(), T(key + "a", (B,), 0.25, 1.0)


def ce_eval(z, y, alpha, gamma, scale, dt=torch.float64, flip=False, fault=None):
    """-> rowloss [B], loss (float64 scalar), dlogits [B, C].  gamma < 0: plain CE (alpha unused)."""
    z = z.to(dt)
    B, C = z.shape
    m = torch.zeros(B, 1, dtype=dt) if fault == "no_max" else z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    se = (e.flip(1) if flip else e).sum(1, keepdim=True)
    logp = z.gather(1, y[:, None]) - m - torch.log(se)
    ce, pt = -logp, torch.exp(logp)
    if gamma >= 0:
        a = alpha.to(dt)[:, None] if alpha is not None else torch.ones(B, 1, dtype=dt)
        om = 1.0 - pt
        w = om ** int(gamma)
        loss = a * w * ce
        dce = a * (w + (gamma * om ** int(gamma - 1) * pt * ce if gamma > 0 else 0.0))
    else:
        loss, dce = ce, torch.ones(B, 1, dtype=dt)
    onehot = torch.zeros(B, C, dtype=dt).scatter_(1, y[:, None], 1.0)
    dl = torch.tensor(f32(scale), dtype=dt) * dce * (e / se - onehot) / B
    return loss[:, 0], loss.double().sum() * (f32(scale) / B), dl


def ce_bounds(z, y, alpha, gamma, scale):
    z = z.double()
    B, C = z.shape
    zm = z - z.max(1, keepdim=True).values
    e = torch.exp(zm)
    se = e.sum(1, keepdim=True)
    rho_i = FN + U * zm.abs()
    rho_se = rho_i.max(1, keepdim=True).values + (cdiv(C, 64) + 8) * U
    lse = torch.log(se)
    zy = zm.gather(1, y[:, None])
    logp = zy - lse
    e_logp = 2 * U * zy.abs() + rho_se + FN * lse.abs() + 2 * U * logp.abs()
    ce, pt = -logp, torch.exp(logp)
    if gamma < 0:
        loss, e_loss, dce, e_dce = ce, e_logp + U * ce.abs(), torch.ones_like(ce), torch.zeros_like(ce)
    else:
        gi = int(gamma)
        a = alpha.double().abs()[:, None] if alpha is not None else torch.ones_like(ce)
        e_pt = pt * (e_logp + FN)
        om = 1.0 - pt
        e_om = 2 * U + e_pt
        w = om ** gi
        e_w = (gi * om ** (gi - 1) * e_om if gi > 0 else 0.0) + (e_om ** 2 if gi == 2 else 0.0) + FN * w
        loss = a * w * ce
        e_loss = a * (e_w * ce + w * e_logp) + 4 * U * loss.abs()
        if gi > 0:
            h = om ** (gi - 1)
            e_h = (e_om if gi == 2 else 0.0) + FN * h
            t = gi * h * pt * ce
            e_t = gi * (e_h * pt * ce + h * e_pt * ce + h * pt * e_logp) + FN * t
            dce, e_dce = a * (w + t), a * (e_w + e_t) + 2 * U * a * (w + t)
        else:
            dce, e_dce = a * w, U * a * w
    sm = e / se
    e_sm = sm * (rho_i + rho_se + 2 * U) + FLT_MIN
    diff = (sm - torch.zeros(B, C, dtype=torch.float64).scatter_(1, y[:, None], 1.0)).abs()
    s = abs(f32(scale))
    dl = s * dce * diff / B
    e_dl = s / B * (e_dce * diff + dce.abs() * (e_sm + U * diff)) + 4 * U * dl
    total = (loss.sum() * s / B).abs()
    return e_loss[:, 0], s / B * e_loss.sum() + 2 * U * total, e_dl


# =========================================================================================================================================
# 4. KLD, reparameterisation
# =========================================================================================================================================
KLD_SHAPES = ((1, 1), (5, 32), (3, 85), (1, 257), (7, 1000))
KLD_LOGVAR = ((-2.0, 1.0), (-10.0, 10.0))


def kld_inputs(n, d, lv):
    key = f"kld{n}x{d}{lv[1]}"
    return T(key + "m", (n, d), -2, 2), T(key + "l", (n, d), lv[0], lv[1]), T(key + "e", (n, d), -2, 2)


def kld_eval(mu, lv, scale, dt=torch.float64, flip=False):
    m, l, n = mu.to(dt), lv.to(dt), mu.shape[0]
    k = torch.tensor(f32(scale), dtype=dt) / torch.tensor(float(n), dtype=dt)
    e = torch.exp(l)
    terms = (1.0 + l - m * m - e).reshape(-1)
    s = (terms.flip(0) if flip else terms).sum()
    return -0.5 * k * s, k * m, k * 0.5 * (e - 1.0)


def kld_bounds(mu, lv, scale):
    m, l, (n, d) = mu.double(), lv.double(), mu.shape
    k = abs(f32(scale)) / n
    loss, dmu, dlv = kld_eval(mu, lv, scale)
    A = 1.0 + l.abs() + m * m + torch.exp(l)
    L = cdiv(n * d, 256) + 8
    return 0.5 * k * (L + 16) * U * A.sum() + 3 * U * loss.abs(), 4 * U * dmu.abs(), 0.5 * k * (5 * U * torch.exp(l) + U) + 4 * U * dlv.abs()


def reparam_eval(mu, lv, eps, dt=torch.float64):
    return eps.to(dt) * torch.exp(0.5 * lv.to(dt)) + mu.to(dt)


def reparam_bound(mu, lv, eps):
    z = reparam_eval(mu, lv, eps)
    return 7 * U * eps.double().abs() * torch.exp(0.5 * lv.double()) + 2 * U * z.abs() + U * mu.double().abs()


# =========================================================================================================================================
# 5. memory gates
# =========================================================================================================================================
GATE_SHAPES = ((1, 1, 1, 1), (2, 5, 126, 3), (3, 8, 64, 8), (2, 4, 65, 0), (2, 34, 282, 17))       # (B, P, D, chunk)
TM_SHAPES = tuple(s for s in GATE_SHAPES if s[3] >= 1) + ((2, 64, 4, 64),)
GATE_AXES = ("clip", "frame", "dim")


def gate_inputs(B, P, D, chunk, saturate=False):
    """-> mem [B, D], pred [B, P, D], dout [B, P, D], score [B, chunk].  saturate: |<m, p>| > 100 on the gated frames, both signs."""
    key = f"gate{B}x{P}x{D}x{chunk}{int(saturate)}"
    m, p, g = T(key + "m", (B, D)), T(key + "p", (B, P, D)), T(key + "g", (B, P, D))
    if saturate:
        sign = torch.where(torch.arange(P) % 2 == 0, 1.0, -1.0).view(1, P, 1)
        p = (sign * m.sign().view(B, 1, D) * (p.abs() + 0.5) * (600.0 / D + 1.0)).float()
        m = (m.sign() * (m.abs() + 0.5)).float()
    return m, p, g, T(key + "s", (B, max(chunk, 1)), -50, 50)[:, :chunk].contiguous()


def sp_eval(m, p, chunk, dt=torch.float64, flip=False):
    m, p = m.to(dt), p.to(dt)
    pr = (m[:, None, :] * p[:, :chunk]) if chunk else torch.zeros(p.shape[0], 0, p.shape[2], dtype=dt)
    s = torch.sigmoid((pr.flip(2) if flip else pr).sum(2))
    out = p.clone()
    out[:, :chunk] = s[..., None] * p[:, :chunk] + (1.0 - s[..., None]) * m[:, None, :]
    return out, s


def sp_bounds(m, p, chunk):
    D = m.shape[1]
    md, pd = m.double(), p.double()
    out, s = sp_eval(m, p, chunk)
    e_dot = (cdiv(D, 64) + 14) * U * (md[:, None, :] * pd[:, :chunk]).abs().sum(2)
    e_s = s * (1 - s) * (e_dot + FN) + 3 * U * s + FLT_MIN
    e_out = torch.zeros_like(out)
    sc = s[..., None]
    e_out[:, :chunk] = e_s[..., None] * (pd[:, :chunk] - md[:, None, :]).abs() + 4 * U * ((sc * pd[:, :chunk]).abs() + ((1 - sc) * md[:, None, :]).abs()) \
        + U * out[:, :chunk].abs()
    return e_out, e_s


def sp_bwd_eval(m, p, gate, g, chunk, dt=torch.float64, flip=False, fault=None):
    m, p, g, s = m.to(dt), p.to(dt), g.to(dt), gate.to(dt)[..., None]
    pc, gc, mm = p[:, :chunk], g[:, :chunk], m[:, None, :]
    t = gc * (pc - mm)
    ds = (t.flip(2) if flip else t).sum(2, keepdim=True)
    dscore = ds * s * (1.0 - s)
    dp = g.clone()
    dp[:, :chunk] = gc * s + dscore * mm
    terms = gc * (1.0 - s) + dscore * pc
    if fault == "dm_last_frame" and chunk:
        terms = terms[:, :chunk - 1]
    return dp, (terms.flip(1) if flip else terms).sum(1)


def sp_bwd_bounds(m, p, gate, g, chunk):
    D = m.shape[1]
    md, pd, gd, s = m.double(), p.double(), g.double(), gate.double()[..., None]
    pc, gc, mm = pd[:, :chunk], gd[:, :chunk], md[:, None, :]
    ds = (gc * (pc - mm)).sum(2, keepdim=True)
    e_ds = (cdiv(D, 64) + 14) * U * (gc * (pc - mm)).abs().sum(2, keepdim=True)
    dscore = ds * s * (1 - s)
    e_dsc = s * (1 - s) * e_ds + 4 * U * dscore.abs()
    e_dp = torch.zeros_like(pd)
    e_dp[:, :chunk] = mm.abs() * e_dsc + 6 * U * ((gc * s).abs() + (dscore * mm).abs())
    mag = (gc * (1 - s)).abs() + (dscore * pc).abs()
    e_dm = (pc.abs() * e_dsc).sum(1) + (chunk + 6) * U * mag.sum(1)
    return e_dp, e_dm


def tm_eval(score, p, chunk, dt=torch.float64, flip=False, fault=None):
    s, p = score.to(dt), p.to(dt)
    mx = torch.zeros(s.shape[0], 1, dtype=dt) if fault == "no_max" else s.max(1, keepdim=True).values
    e = torch.exp(s - mx)
    w = e / (e.flip(1) if flip else e).sum(1, keepdim=True)
    out = p.clone()
    out[:, :chunk] = p[:, :chunk] * (1.0 + w[..., None])
    return out, w


def tm_bounds(score, p, chunk):
    s = score.double()
    out, w = tm_eval(score, p, chunk)
    rho_i = FN + U * (s - s.max(1, keepdim=True).values).abs()
    e_w = w * (rho_i + rho_i.max(1, keepdim=True).values + (chunk + 4) * U) + FLT_MIN
    e_out = torch.zeros_like(out)
    e_out[:, :chunk] = p.double()[:, :chunk].abs() * e_w[..., None] + 4 * U * out[:, :chunk].abs()          # 1 + w and the product: two roundings
    return e_out, e_w


def tm_bwd_eval(w, p, g, chunk, dt=torch.float64, flip=False):
    w, p, g = w.to(dt), p.to(dt), g.to(dt)
    dp = g.clone()
    dp[:, :chunk] = g[:, :chunk] * (1.0 + w[..., None])
    t = g[:, :chunk] * p[:, :chunk]
    dw = (t.flip(2) if flip else t).sum(2)
    wd = w * dw
    return dp, w * (dw - (wd.flip(1) if flip else wd).sum(1, keepdim=True))


def tm_bwd_bounds(w, p, g, chunk):
    D = p.shape[2]
    wd, pd, gd = w.double(), p.double(), g.double()
    dp, dscore = tm_bwd_eval(w, p, g, chunk)
    t = gd[:, :chunk] * pd[:, :chunk]
    dw = t.sum(2)
    e_dw = (cdiv(D, 64) + 14) * U * t.abs().sum(2)
    dot = (wd * dw).sum(1, keepdim=True)
    e_dot = (wd * e_dw).sum(1, keepdim=True) + (chunk + 2) * U * (wd * dw).abs().sum(1, keepdim=True)
    return 4 * U * dp.abs(), wd * (e_dw + e_dot + 2 * U * (dw.abs() + dot.abs())) + 2 * U * dscore.abs() + FLT_MIN * (1 + dw.abs() + dot.abs())     # + a weight below 2^-126, flushed or denormal


# =========================================================================================================================================
# 6. Adam
# =========================================================================================================================================
ADAM_T = (1, 2, 1000, 100000)
ADAM_WD = (0.0, 1e-5)
ADAM_N = (1, 7, 8, 9, 1027, 4103)
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_CLASSES = ("decades", "zero", "tiny_v")
AdamPlan = namedtuple("AdamPlan", "route head n4 tail workgroups")


def adam_plan(n, phase=0, grad_phase=None):
    """launch_adam: phase = the offset of the p / m / v slices from a 16-byte boundary in floats, grad_phase that of the gradient (default: the same)."""
    if (grad_phase is not None and grad_phase != phase) or n < 8:
        return AdamPlan("scalar", 0, 0, 0, min(cdiv(n, 256), 16384))
    head = (4 - phase) % 4
    n4 = (n - head) // 4
    return AdamPlan("float4", head, n4, n - head - 4 * n4, cdiv(n4, 1024))


def adam_inputs(n, cls):
    key = f"adam{n}{cls}"
    p = T(key + "p", (n,))
    if cls == "zero":
        z = torch.zeros(n)
        return p, z, z.clone(), z.clone()
    g = (T(key + "g", (n,)).double() * 10.0 ** (-6.0 * T(key + "d", (n,), 0, 1).double())).float()          # six decades
    m = (0.5 * g.double() * T(key + "m", (n,), 0.5, 1.5).double()).float()
    v = (g.double() ** 2 * T(key + "v", (n,), 0.5, 1.5).double()).float()
    if cls == "tiny_v":                      # sqrt(v) << eps: the step is lr m / eps scaled
        g, m, v = (g * 1e-12).float(), (m * 1e-12).float(), (v.double() * 1e-24).float()
    return p, g, m, v


def adam_eval(p, g, m, v, t, wd, dt=torch.float64, fault=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    c = lambda val: torch.tensor(f32(val), dtype=dt)
    bc1, bc2s = 1.0 - f32(b1) ** t, np.sqrt(1.0 - f32(b2) ** t)
    if dt == torch.float32:
        bc1, bc2s = f32(bc1), f32(bc2s)
    if fault == "no_bc2":
        bc2s = 1.0
    bc1, bc2s = torch.tensor(bc1, dtype=dt), torch.tensor(bc2s, dtype=dt)
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    one = torch.tensor(1.0, dtype=dt)
    gi = g + c(wd) * p
    mi = c(b1) * m + (one - c(b1)) * gi
    vi = c(b2) * v + (one - c(b2)) * gi * gi
    pn = p - (c(lr) / bc1) * mi / (torch.sqrt(vi) / bc2s + c(eps))
    return pn, mi, vi


def adam_bounds(p, g, m, v, t, wd, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    pn, mi, vi = adam_eval(p, g, m, v, t, wd, lr=lr, b1=b1, b2=b2, eps=eps)
    P, G, M, V = p.double(), g.double(), m.double(), v.double()
    b1, b2, lr, eps, wd = f32(b1), f32(b2), f32(lr), f32(eps), f32(wd)
    gi = G + wd * P
    e_g = 2 * U * (G.abs() + (wd * P).abs())
    e_m = (1 - b1) * e_g + 4 * U * ((b1 * M).abs() + ((1 - b1) * gi).abs()) + 4 * FLT_MIN         # + underflow of the products (flushed or denormal)
    e_v = 2 * (1 - b2) * gi.abs() * e_g + (1 - b2) * e_g ** 2 + 5 * U * (b2 * V + (1 - b2) * gi * gi) + 4 * FLT_MIN
    A = lr / (1.0 - b1 ** t)
    bc2s = np.sqrt(1.0 - b2 ** t)
    rt = torch.sqrt(vi)
    e_rt = torch.where(vi > e_v, e_v / torch.clamp(rt, min=FLT_MIN), torch.sqrt(e_v))         # |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|)
    den = rt / bc2s + eps
    e_den = (e_rt + 3 * U * rt) / bc2s + U * den
    upd = A * mi / den
    e_upd = A * (e_m / den + mi.abs() * e_den / den ** 2) + 4 * U * upd.abs()
    return e_upd + 2 * U * pn.abs(), e_m + 2 * U * mi.abs(), e_v + 2 * U * vi.abs()


# =========================================================================================================================================
# 7. bf16 payload
# =========================================================================================================================================
BF16_N = (1, 255, 257)
BF16_NAN_BITS = (0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001, 0xFF800001, 0x7FC00000, 0x7F80FFFF, 0x7FFF8000)


def bf16_finite_bits():
    """fp32 bit patterns: ties to even in both directions, the largest finite value (-> inf), denormals, +-0, +-inf, and hashed values."""
    fixed = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,
             0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x80000001, 0x80008000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
             0x3F800000, 0x00800000, 0x00807FFF, 0x0080FFFF]
    rnd = (T("bf16bits", (300,), 0, 1).double() * 2.0 ** 32).long().clamp(0, 2 ** 32 - 1).tolist()
    rnd = [b for b in rnd if (b & 0x7FFFFFFF) <= 0x7F800000]
    return fixed + rnd


def bits_to_f32(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def bf16_rne_bits(bits, nan_case=True):
    """f32_to_bf16_rne of csrc/common.h on uint32 bit patterns -> uint16 patterns (nan_case = False: the function before its NaN case)."""
    u = np.asarray(bits, dtype=np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    if nan_case:
        r = np.where((u & 0x7FFFFFFF) > 0x7F800000, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def is_bf16_nan(h):
    h = np.asarray(h).astype(np.uint16)
    return (h & 0x7FFF) > 0x7F80


# =========================================================================================================================================
# 8. segment operators
# =========================================================================================================================================
SEG_AXES = ("clip", "channel")
SegCase = namedtuple("SegCase", "batch hw c ws route why")
SEG_CASES = [
    SegCase(1, 1, 8, False, "one_kernel", "a single pixel"),
    SegCase(3, 5, 34, False, "one_kernel", "workspace NULL, generic C"),
    SegCase(3, 130, 130, False, "one_kernel", "workspace NULL: 33 rows per wave, three column blocks, the last with 2 columns"),
    SegCase(3, 130, 64, True, "fast", "segmented fast path, nseg = 3"),
    SegCase(3, 5, 8, True, "fast", "segmented fast path, C = 8: 128 row lanes for 5 rows"),
    SegCase(1, 130, 8, True, "fast", "one segment"),
    SegCase(3, 130, 34, True, "generic", "one generic launch per segment, two row blocks each"),
    SegCase(3, 1, 130, True, "generic", "HW = 1 through the generic partials"),
    SegCase(513, 1, 8, True, "one_kernel", "batch > 512 falls back to the one-kernel form although a workspace is given"),
]


def seg_plan(case):
    if not case.ws or case.batch > 512:
        return ColPlan("one_kernel", 1, case.hw, 4, cdiv(case.hw, 4) + 4, 0)
    return bn_plan(case.hw, case.c, True, case.batch)


def seg_inputs(case):
    key = f"seg{case.batch}x{case.hw}x{case.c}"
    shape = (case.batch, case.hw, case.c)
    return T(key + "x", shape), T(key + "dy", shape), T(key + "g", (case.batch, case.c), 0, 1), T(key + "a", (case.batch, case.c))


def seg_eval(x, dy, gate, add, scale, dt=torch.float64, flip=False):
    """-> seg_mean, seg_dot, se_scale without add, se_scale with add."""
    x, dy, gate, add = x.to(dt), dy.to(dt), gate.to(dt), add.to(dt)
    f = (lambda t: t.flip(1)) if flip else (lambda t: t)
    return f(x).sum(1) * torch.tensor(f32(scale), dtype=dt), f(dy * x).sum(1), dy * gate[:, None, :], dy * gate[:, None, :] + add[:, None, :]


def seg_bounds(x, dy, gate, add, scale, plan):
    K = plan.L + plan.Z + 8
    mean, dot, y0, y1 = seg_eval(x, dy, gate, add, scale)
    ag = (dy.double() * gate.double()[:, None, :]).abs()
    return (K * U * x.double().abs().sum(1) * abs(f32(scale)) + 2 * U * mean.abs(), K * U * (dy.double() * x.double()).abs().sum(1) + 2 * U * dot.abs(),
            2 * U * ag + 2 * U * y0.abs(), 2 * U * ag + 2 * U * y1.abs())
