"""Test-side float64 restatements of the kernels of csrc/misc.hip that no other test compares on their own -- the front half of the prior encoder
(prior_pred_kernel, tm_gram_kernel, tm_apply_kernel through eg_prior_encoder), the five contrastive-loss kernels, small_linear_kernel,
convt1d_kernel and the two embedding kernels -- with the bound every ELEMENT of their results is held to, the case lists of the GPU tests (a reason
per case and the route it takes), and CPU emulations of the kernels' fp32 arithmetic in two summation orders (tests/test_misc_f64.py).  A helper
module (not collected: no test_ prefix); CPU only.  T, U, compare_sliced are those of tests/small_ops_f64.py; FN (one expf / logf: 4 u), FLT_MIN
and the sigmoid / softmax rules are those of tests/train_tail_f64.py section 5.  The reference is always float64 of the same fp32 inputs.
u = 2^-24.  A single rounding can reach u |ref| on its own and correct arithmetic is asked to stay at HALF of every bound, so a rounding that is
counted on its own enters as 2 u.  K(n) = ceil(n / 64) + 8 is the chain of a block_dot: a lane's n / 64 terms, the 6-level butterfly, the bias.

1. Prior encoder (P prior frames = conv channels, PL = F - P predicted frames, the pose axis D = conv length)
    conv1       s1 = b1 + sum w1 x over 3 P terms, one chain:  e_s1 = (3 P + 3) u (|b1| + sum |w1 x|).
    ReLU, BN    h1 = relu(s1) sc1 + sh1.  ReLU is 1-Lipschitz (no flip handling):  e_h1 = |sc1| e_s1 + 2 u |relu(s1) sc1| + 2 u |h1|.
    conv2       e_s2 = sum |w2| e_h1 (the zero padding of the hidden map is exact) + (3 PL + 3) u (|b2| + sum |w2 h1|);  pred like h1.
    spatial     cat = [prior (bit for bit) | pred], columns D .. Dpad-1 are +0.
    memory      flat = prior[:, P - chunk:] (exact).  Every Linear y = W x + b with an input error e_x:
                e_y = sum |W| e_x + K(n) u sum |W x| + 2 u |y|  (M1 of the TM encoder is one thread's chain: chunk + 3 for K).
                m = sp1(sp0(flat)), tm_mem = tc1(tc0(flat));  dot_c = <m, pred_c>: e_dot = sum (|m| e_pred + |pred| e_m + e_m e_pred) + K(D) u sum |m pred|;
                s = sigmoid(dot): e_s = s (1 - s) (e_dot + FN) + 3 u s + 2^-126;  g = s pred + (1 - s) m:
                e_g = e_s |pred - m| + s e_pred + (1 - s) e_m + e_s (e_pred + e_m) + 4 u (|s pred| + |(1 - s) m|) + u |g|;
                tm_pe = tm1(tm0(flat(g[:chunk])));  tm_gram = tm_mem^T tm_pe over the batch: e_G = sum_b (|mem| e_pe + |pe| e_mem + e_mem e_pe) + (B + 3) u sum_b |mem pe|;
                score = tm_mem G (block_dot over D);  w = softmax(score): a score error is a relative error of its exponential, so with
                rel_c = expm1(FN + u |score_c - max| + e_score_c):  e_w = w (rel_c + max_j rel_j + (chunk + 4) u) + 2^-126;
                out_c = g_c + g_c w_c:  e_out = (1 + w) e_g + |g| e_w + e_g e_w + 4 u |out|.   Frames c >= chunk keep e_pred.
    The clips of one call are coupled through tm_gram (the reference's torch.mm over the batch): clip b of a batch differs from clip b alone.
    inputs      biases and BN shifts of order 1 (a hidden halo position computed from the bias, where zero padding belongs, is far outside the bound);
                sp1 and tm1 are scaled (prior_inputs) so that every SP sigmoid lies in [0.05, 0.95] and every TM softmax row has two weights
                >= 0.05: a one-hot softmax cannot see a fault of the TM step.  tests/test_misc_f64.py checks both on the reference alone.
2. Contrastive loss (face, audio [n, d])
    norms       inv = 1 / max(sqrt(sum x^2), 1e-12); the terms are positive, so the relative error is r(L) = (0.5 (L + 1) + 3) u for a chain of
                L additions.  The forward takes the face norm by a 256-slot tree (L = ceil(d / 256) + 8) and the audio norm by one serial loop
                (L = d); the backward takes both by the tree.  The bounds use the longer chain of the two routes for each.
    distance    t_k = fh_k - ah_k: e_t = |fh_k| (r_f + 2 u) + |ah_k| (r_a + 2 u) + 2 u |t_k|;  dist = sum t^2 serial:
                e_dist = sum (2 |t| e_t + e_t^2) + (d + 2) u dist;  E_D = min(e_dist / D, sqrt(e_dist)) + 2 u D.
    cross       c = max(1 / (D + 1e-8), 1e-8).  With x = D + 1e-8 and delta = E_D + 2 u x:  e_c = c delta / (x - delta) + 2 u c  (exact, not
                linearised: c^2 E_D to first order) while delta < x / 2.  Past that the bound is VACUOUS (inf): a face row bit-identical to its
                audio row has D = 0 and c = 1e8 in float64, while in fp32 the two norm routes of the forward may differ in the last bit.  Such an
                element is held to the one-sided statement  cross >= (1 - 4 u) / (D + E_D + 1e-8);  a row whose only vacuous element is its
                diagonal must be a hit with a row loss of at most 8 u (the diagonal is the maximum, every other exponential underflows); a row with
                any other vacuous element (d = 1: every normalised value is +-1 and D is 0 or 2) is held to finiteness only, and so is the mean.
    row loss    lse - c_ii:  e_row = sum_j p_j e_c_j + e_c_ii + rho_se + FN |log se| + 2 u (|m| + |log se| + |lse| + |c_ii|),
                rho_se = max_j (FN + u |c_j - m|) + (ceil(n / 256) + 9) u.   loss = mean: mean(e_row) + (ceil(n / 256) + 10) u mean |row| + 2 u |loss|.
    acc         a row is DECIDED when the float64 margin between its two largest values exceeds the sum of their bounds, or when those two come
                from bit-identical audio rows (the kernel computes them bit-equal; the lower index wins, as torch.argmax).  The hit of a decided
                row must be exact; acc must equal float32(hits) / float32(n) when every row is decided.
    gradients   suffer the cancellation of the normalisation's projection g - xh <xh, g>.  Tolerance per element (con_grad_tols):
                CON_GRAD_FACTOR = 4 x the error of torch's own float32 CPU autograd against float64 on the same inputs, per input class, in units of
                the row's gradient rms (con_grad_units; floored at u x the rms of the row's terms in magnitude), CON_GRAD_CPU_F32 below --
                tests/test_misc_f64.py re-measures it and fails when stale by > 2 x; it is measured against the reference, never against the kernel
                -- plus 4 u x the element's own terms in magnitude, A_ik = sum_j |W_ij| |fh_ik - ah_jk| / |f_i| carried through the projection.  The
                second part is what fused multiply-adds need where two terms cancel exactly (two tied columns pull a face row in opposite
                directions: the float64 gradient is 0): torch rounds both products and their sum is 0, a fused chain keeps the second product exact
                and is left with the rounding of the first, and the projection spreads that over the row.
                Cases (CON_GRAD_CASES): d = 1 is left out (the projection annihilates the gradient), and so are 255 x 3 and 257 x 3 (hundreds of
                directions cannot be kept apart in three dimensions: chance pairs at D ~ 1e-3 make a row's softmax ill-conditioned and torch's own
                float32 gradient is off by more than the row's rms).  The near class has every softmax row one-hot to e^-99: its float64 gradients
                are below 1e-36, the kernel's must be finite and below 1e-30.  In the identical-row case W_ii (read from the workspace) must be
                exactly 0: dD/dx = 0 at D = 0, as torch.norm has it.
                Defect these tests found (fixed in csrc/misc.hip): the backward kernels summed fh_i sum_j W_ij - sum_j W_ij ah_j, whose terms are
                of size |W| where those of sum_j W_ij (fh_i - ah_j) are of size |W| D, in one chain of n fused multiply-adds, and the distance in one
                chain of d.  Next to an audio row (the tie rows, D = 0.03) the face gradient was ~20 units off (fault "factored_sum"); correct
                arithmetic of single chains reached 0.7 to 0.95 of the tolerance at 300 x 257.  The kernels now sum term by term in four
                interleaved chains, the distance too; test_gpu_contrastive_f64.py::test_contrastive_backward_matches_float64_per_element fails
                on the ties class when that is reverted.
3. eg_small_linear      K(In) u sum |w x| + 2 u |y|.
4. eg_conv_transpose1d  (3 cin + 4) u (|bias| + sum |w x|) max(1, |scale|) + u |y|  (conv1d_bound's form; an even output has cin terms, an odd one 2 cin).
5. eg_embedding         bit for bit; nothing to bound.

Worst element of correct arithmetic (the emulations, both orders) as a fraction of its bound: WORST_OF_CORRECT_ARITHMETIC below -- prior encoder cat
0.040, tm_mem 0.008, tm_pe and tm_gram < 0.001 (the bounds carry every stage's worst case through sums of up to 2820 terms; the faults of
PRIOR_FAULTS still exceed them, tests/test_misc_f64.py); contrastive cross 0.113, row loss 0.047, loss 0.013, gface 0.31, gaudio 0.30;
small_linear 0.209; transposed convolution 0.138.

Worst element seen on the MI355X as a fraction of its bound or tolerance (the GPU tests print theirs as FRACTION lines; also GPU_WORST_FRACTIONS):
    eg_prior_encoder       cat 0.030   tm_mem 0.007   tm_pe < 0.001   tm_gram 0.001
    eg_contrastive_loss    cross 0.103   row loss 0.079   loss 0.014          eg_contrastive_loss_backward   gface 0.280   gaudio 0.369
    eg_small_linear 0.209                eg_conv_transpose1d 0.151           eg_embedding: bit for bit
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as TF

from small_ops_f64 import T, U, compare_sliced, images_of, sliced_errors  # noqa: F401  (re-exported for the tests)
from train_tail_f64 import FLT_MIN, FN, cdiv, worst  # noqa: F401

F64 = torch.float64
LDS_LIMIT = 160 * 1024

# Worst element of correct arithmetic as a fraction of its bound over every case (tests/test_misc_f64.py measures, prints and holds each to <= 0.5
# and to these figures, which are its own rounded up):
WORST_OF_CORRECT_ARITHMETIC = {
    "prior cat": 0.05, "prior tm_mem": 0.01, "prior tm_pe": 0.01, "prior tm_gram": 0.01,
    "con cross": 0.12, "con rowloss": 0.05, "con loss": 0.02, "con gface": 0.35, "con gaudio": 0.47,
    "small_linear": 0.21, "convt": 0.14,
}
# Worst element on the MI355X as a fraction of its bound / tolerance (the FRACTION lines of the GPU modules):
GPU_WORST_FRACTIONS = {
    "prior cat": 0.030, "prior tm_mem": 0.007, "prior tm_pe": 0.001, "prior tm_gram": 0.001,
    "contrastive cross": 0.103, "contrastive rowloss": 0.079, "contrastive loss": 0.014, "contrastive gface": 0.280, "contrastive gaudio": 0.369,
    "small_linear": 0.209, "conv_transpose1d": 0.151,
}


def K(n):
    return cdiv(n, 64) + 8


# =========================================================================================================================================
# 1. prior encoder
# =========================================================================================================================================
PriorCase = namedtuple("PriorCase", "B P PL D Dpad chunk variant staged refused why")
# LDS of one workgroup (egi_prior_encoder): dc = min(D, 64) pose columns per slice (variant 1: dc = D), base = 4 (P (dc + 4) + PL (dc + 2) + PL dc
# [+ chunk D + 2 D]) bytes, conv weights 4 (3 PL P + 3 PL PL) bytes; the weights are staged when base + weights <= 160 KiB = 163840.
PRIOR_SPATIAL = [
    PriorCase(2, 4, 30, 126, 128, 0, 0, True, False, "two slices, the last one partial (62 columns), two pad columns"),
    PriorCase(2, 4, 30, 63, 64, 0, 0, True, False, "below one slice"),
    PriorCase(2, 4, 30, 64, 64, 0, 0, True, False, "exactly one slice, no pad column"),
    PriorCase(2, 4, 30, 65, 128, 0, 0, True, False, "a second slice of one column whose whole input comes from the halo"),
    PriorCase(2, 4, 30, 128, 128, 0, 0, True, False, "a boundary between two full slices"),
    PriorCase(2, 4, 30, 1, 64, 0, 0, True, False, "D = 1: every conv term but the centre tap is padding"),
    PriorCase(3, 10, 50, 282, 320, 0, 0, True, False, "five slices, 38 pad columns (the BEAT shape): base 28720 + weights 36000 B"),
    PriorCase(1, 10, 118, 130, 192, 0, 0, False, False, "base 64080 + weights 181248 B > 163840: the conv weights are read through L1 (stage_w = 0)"),
]
PRIOR_MEMORY = [
    PriorCase(4, 4, 30, 126, 128, 4, 1, True, False, "the TED shape: base 35584 + weights 12240 B"),
    PriorCase(1, 4, 30, 126, 128, 4, 1, True, False, "B = 1: the gram is the clip's own outer product"),
    PriorCase(2, 4, 30, 126, 128, 3, 1, True, False, "chunk 3: three of the four waves work in the chunk loops"),
    PriorCase(2, 6, 30, 126, 128, 5, 1, True, False, "chunk 5: wave 0 takes two turns, the others one"),
    PriorCase(2, 6, 30, 126, 128, 4, 1, True, False, "P 6 with chunk 4: the memory reads the LAST four prior frames, not the first"),
    PriorCase(2, 4, 30, 65, 128, 4, 1, True, False, "D = 65: a block_dot lane with two terms, the others one"),
    PriorCase(2, 4, 30, 63, 64, 4, 1, True, False, "D = 63: a block_dot with an idle lane"),
    PriorCase(3, 10, 50, 282, 320, 10, 1, False, False, "the BEAT shape: base 138176 + weights 36000 B > 163840, unstaged"),
    PriorCase(1, 10, 110, 282, 320, 10, 1, False, True, "base 274016 B > 163840: refused (EG_ERR_UNSUPPORTED), every output untouched"),
]
PRIOR_CASES = PRIOR_SPATIAL + PRIOR_MEMORY
PRIOR_AXES = ("clip", "frame", "dim")
PriorPlan = namedtuple("PriorPlan", "dc slices staged smem refused")


def prior_plan(c):
    """egi_prior_encoder's launch arithmetic restated."""
    dc = c.D if c.variant == 1 else min(c.D, 64)
    base = 4 * (c.P * (dc + 4) + c.PL * (dc + 2) + c.PL * dc + (c.chunk * c.D + 2 * c.D if c.variant == 1 else 0))
    wb = 4 * (3 * c.PL * c.P + 3 * c.PL * c.PL)
    staged = base + wb <= LDS_LIMIT
    smem = base + (wb if staged else 0)
    return PriorPlan(dc, cdiv(c.D, dc), staged, smem, smem > LDS_LIMIT)


def _signed(key, shape, lo, hi):
    """Magnitudes in (lo, hi), every third value negative."""
    n = int(np.prod(shape))
    return T(key, shape, lo, hi) * torch.where(torch.arange(n) % 3 == 1, -1.0, 1.0).view(shape)


def prior_inputs(c):
    """-> dict of fp32 tensors: prior, conv (the eight conv / BN vectors, in the ABI's order), mem (the twelve memory-net tensors, or None).
    Biases and BN shifts are of order 1.  For the memory variant sp1 (weight and bias) is scaled so that the largest |<m, pred_c>| is 2.5 and tm1
    so that the widest score row spans 2: the scale comes from the float64 reference of the unscaled weights."""
    key = f"prior{c.B}x{c.P}x{c.PL}x{c.D}x{c.chunk}v{c.variant}"
    P, PL, D = c.P, c.PL, c.D
    a1, a2 = 1.0 / np.sqrt(3 * P), 1.0 / np.sqrt(3 * PL)
    conv = [T(key + "w1", (PL, P, 3), -a1, a1), T(key + "b1", (PL,), -1.5, 1.5), _signed(key + "s1", (PL,), 0.5, 1.5), T(key + "t1", (PL,), -1.5, 1.5),
            T(key + "w2", (PL, PL, 3), -a2, a2), T(key + "b2", (PL,), -1.5, 1.5), _signed(key + "s2", (PL,), 0.5, 1.5), T(key + "t2", (PL,), -1.5, 1.5)]
    inp = {"prior": T(key + "x", (c.B, P, D)), "conv": conv, "mem": None}
    if c.variant == 1:
        CD, ch = c.chunk * D, c.chunk
        a0, ad, ac = 1.0 / np.sqrt(CD), 1.0 / np.sqrt(D), 1.0 / np.sqrt(ch)
        mem = []
        for net, n_out in (("sp", D), ("tc", D), ("tm", ch)):
            n_mid = D if net != "tm" else ch
            a_mid = ad if net != "tm" else ac
            mem += [T(key + net + "w0", (n_mid, CD), -a0, a0), T(key + net + "b0", (n_mid,), -0.5, 0.5),
                    T(key + net + "w1", (n_out, n_mid), -a_mid, a_mid), T(key + net + "b1", (n_out,), -0.5, 0.5)]
        inp["mem"] = mem
        r = prior_f64(inp, c)
        k = 2.5 / float(r["dot"].abs().max())
        mem[2], mem[3] = (mem[2].double() * k).float(), (mem[3].double() * k).float()
        r = prior_f64(inp, c)
        sc = r["score"]
        k = 2.0 / float((sc.max(1).values - sc.min(1).values).max())
        mem[10], mem[11] = (mem[10].double() * k).float(), (mem[11].double() * k).float()
    return inp


def _lin(w, b, x):
    return x @ w.t() + b


def _affine(s, sc, sh):
    return torch.relu(s) * sc.view(1, -1, 1) + sh.view(1, -1, 1)


def prior_f64(inp, c):
    """The operator in float64, plainly: two padded convolutions, the two memory nets, the concatenation.  -> dict with cat [B, F, Dpad], tm_mem,
    tm_pe, tm_gram and the intermediates the bounds and the conditions need (pred, m, dot, s, g, score, w)."""
    x = inp["prior"].double()
    w1, b1, s1, t1, w2, b2, s2, t2 = (v.double() for v in inp["conv"])
    h1 = _affine(TF.conv1d(x, w1, b1, padding=1), s1, t1)
    pred = _affine(TF.conv1d(h1, w2, b2, padding=1), s2, t2)
    out = {"h1": h1, "pred": pred}
    final = pred
    if c.variant == 1:
        sp_w0, sp_b0, sp_w1, sp_b1, tc_w0, tc_b0, tc_w1, tc_b1, tm_w0, tm_b0, tm_w1, tm_b1 = (v.double() for v in inp["mem"])
        ch = c.chunk
        flat = x[:, c.P - ch:, :].reshape(c.B, -1)
        m = _lin(sp_w1, sp_b1, _lin(sp_w0, sp_b0, flat))
        mem = _lin(tc_w1, tc_b1, _lin(tc_w0, tc_b0, flat))
        dot = (pred[:, :ch] * m[:, None, :]).sum(2)
        s = torch.sigmoid(dot)
        g = pred.clone()
        g[:, :ch] = s[..., None] * pred[:, :ch] + (1.0 - s[..., None]) * m[:, None, :]
        pe = _lin(tm_w1, tm_b1, _lin(tm_w0, tm_b0, g[:, :ch].reshape(c.B, -1)))
        gram = mem.t() @ pe
        score = mem @ gram
        w = torch.softmax(score, 1)
        final = g.clone()
        final[:, :ch] = g[:, :ch] + g[:, :ch] * w[..., None]
        out.update(m=m, tm_mem=mem, dot=dot, s=s, g=g, tm_pe=pe, tm_gram=gram, score=score, w=w)
    cat = torch.zeros(c.B, c.P + c.PL, c.Dpad, dtype=F64)
    cat[:, :c.P, :c.D], cat[:, c.P:, :c.D] = x, final
    out["cat"] = cat
    return out


def _lin_err(w, x, y, e_x, k):
    return e_x @ w.abs().t() + k * U * (x.abs() @ w.abs().t()) + 2 * U * y.abs()


def prior_bounds(inp, c):
    """-> (reference dict, bounds dict for cat, tm_mem, tm_pe, tm_gram) by the module docstring, stage by stage."""
    r = prior_f64(inp, c)
    x = inp["prior"].double()
    w1, b1, s1, t1, w2, b2, s2, t2 = (v.double() for v in inp["conv"])
    P, PL, D, B = c.P, c.PL, c.D, c.B

    def aff_err(s, e_s, sc, y):
        return sc.abs().view(1, -1, 1) * e_s + 2 * U * (torch.relu(s) * sc.view(1, -1, 1)).abs() + 2 * U * y.abs()

    sa = TF.conv1d(x, w1, b1, padding=1)
    e_h1 = aff_err(sa, (3 * P + 3) * U * TF.conv1d(x.abs(), w1.abs(), b1.abs(), padding=1), s1, r["h1"])
    sb = TF.conv1d(r["h1"], w2, b2, padding=1)
    e_s2 = TF.conv1d(e_h1, w2.abs(), None, padding=1) + (3 * PL + 3) * U * TF.conv1d(r["h1"].abs(), w2.abs(), b2.abs(), padding=1)
    e_pred = aff_err(sb, e_s2, s2, r["pred"])
    e_cat = torch.zeros_like(r["cat"])
    bounds = {}
    if c.variant != 1:
        e_cat[:, P:, :D] = e_pred
        return r, {"cat": e_cat}
    sp_w0, sp_b0, sp_w1, sp_b1, tc_w0, tc_b0, tc_w1, tc_b1, tm_w0, tm_b0, tm_w1, tm_b1 = (v.double() for v in inp["mem"])
    ch, CD = c.chunk, c.chunk * D
    flat = x[:, P - ch:, :].reshape(B, -1)
    zero = torch.zeros_like(flat)
    v = _lin(sp_w0, sp_b0, flat)
    e_m = _lin_err(sp_w1, v, r["m"], _lin_err(sp_w0, flat, v, zero, K(CD)), K(D))
    v = _lin(tc_w0, tc_b0, flat)
    e_mem = _lin_err(tc_w1, v, r["tm_mem"], _lin_err(tc_w0, flat, v, zero, K(CD)), K(D))
    m, pred, ep = r["m"][:, None, :], r["pred"][:, :ch], e_pred[:, :ch]
    em = e_m[:, None, :]
    e_dot = (m.abs() * ep + pred.abs() * em + em * ep).sum(2) + K(D) * U * (m * pred).abs().sum(2)
    s = r["s"]
    e_s = (s * (1 - s) * (e_dot + FN) + 3 * U * s + FLT_MIN)[..., None]
    sc = s[..., None]
    e_g = e_pred.clone()
    e_g[:, :ch] = e_s * (pred - m).abs() + sc * ep + (1 - sc) * em + e_s * (ep + em) + 4 * U * ((sc * pred).abs() + ((1 - sc) * m).abs()) + U * r["g"][:, :ch].abs()
    gf = r["g"][:, :ch].reshape(B, -1)
    v = _lin(tm_w0, tm_b0, gf)
    e_pe = _lin_err(tm_w1, v, r["tm_pe"], _lin_err(tm_w0, gf, v, e_g[:, :ch].reshape(B, -1), K(CD)), ch + 3)
    mem, pe = r["tm_mem"], r["tm_pe"]
    e_G = mem.abs().t() @ e_pe + e_mem.t() @ pe.abs() + e_mem.t() @ e_pe + (B + 3) * U * (mem.abs().t() @ pe.abs())
    G = r["tm_gram"]
    e_score = mem.abs() @ e_G + e_mem @ G.abs() + e_mem @ e_G + K(D) * U * (mem.abs() @ G.abs())
    score, w = r["score"], r["w"]
    rel = torch.expm1(FN + U * (score - score.max(1, keepdim=True).values).abs() + e_score)
    e_w = (w * (rel + rel.max(1, keepdim=True).values + (ch + 4) * U) + FLT_MIN)[..., None]
    e_out = e_g.clone()
    g = r["g"][:, :ch]
    e_out[:, :ch] = (1 + w[..., None]) * e_g[:, :ch] + g.abs() * e_w + e_g[:, :ch] * e_w + 4 * U * r["cat"][:, P:P + ch, :D].abs()
    e_cat[:, P:, :D] = e_out
    bounds.update(cat=e_cat, tm_mem=e_mem, tm_pe=e_pe, tm_gram=e_G)
    return r, bounds


PRIOR_FAULTS = ("halo_wrong_side", "hidden_halo_from_bias", "affine_before_relu", "mem_first_chunk", "pe_ungated", "gram_own_clip", "row_times_w",
                "pad_unwritten")


def _conv_valid(x, w, b, flip):
    """An unpadded k = 3 convolution in x's precision as the kernel sums it: the bias first, then one multiply-add per (channel, tap), channels
    outer; flip: the same chain backwards."""
    cout, cin, k = w.shape
    width = x.shape[2] - k + 1
    s = b.view(1, -1, 1).expand(x.shape[0], cout, width).clone()
    terms = [(ci, t) for ci in range(cin) for t in range(k)]
    for ci, t in (reversed(terms) if flip else terms):
        s = s + w[:, ci, t].view(1, -1, 1) * x[:, ci:ci + 1, t:t + width]
    return s


def _dot_rows(w, x, flip):
    """x [B, n] @ w [O, n]^T as block_dot sums it: lane l adds its terms l, l + 64, ... one after the other, then the 64 partials meet in a
    six-level butterfly; flip: chains and butterfly levels in the opposite order."""
    n = x.shape[1]
    nl = cdiv(n, 64)
    p = torch.zeros(x.shape[0], w.shape[0], nl * 64, dtype=x.dtype)
    p[:, :, :n] = x[:, None, :] * w[None, :, :]
    p = p.view(x.shape[0], w.shape[0], nl, 64)
    acc = torch.zeros(x.shape[0], w.shape[0], 64, dtype=x.dtype)
    for i in (reversed(range(nl)) if flip else range(nl)):
        acc = acc + p[:, :, i]
    for h in ((1, 2, 4, 8, 16, 32) if flip else (32, 16, 8, 4, 2, 1)):
        acc = acc + acc[:, :, torch.arange(64) ^ h]
    return acc[:, :, 0]


def emulate_prior(inp, c, dt=torch.float32, flip=False, fault=None):
    """The kernels' data flow in precision dt: per slice of dc pose columns the input with a halo of 2 (zero outside [0, D)), the hidden map with a
    halo of 1 (zero outside [0, D), never computed), the two convolutions, then the memory nets on the whole axis, the gram over the batch and the
    softmax scaling.  Unwritten elements of cat are NaN.  fault: one of PRIOR_FAULTS."""
    plan = prior_plan(c)
    x = inp["prior"].to(dt)
    w1, b1, s1, t1, w2, b2, s2, t2 = (v.to(dt) for v in inp["conv"])
    B, P, PL, D = c.B, c.P, c.PL, c.D

    def aff(s, sc, sh):
        if fault == "affine_before_relu":
            return torch.relu(s * sc.view(1, -1, 1) + sh.view(1, -1, 1))
        return torch.relu(s) * sc.view(1, -1, 1) + sh.view(1, -1, 1)

    pred = torch.empty(B, PL, D, dtype=dt)
    for sl in range(plan.slices):
        d0 = sl * plan.dc
        dc = min(plan.dc, D - d0)
        pos = torch.arange(d0 - 2, d0 + dc + 2)
        ok = (pos >= 0) & (pos < D)
        xs = torch.zeros(B, P, dc + 4, dtype=dt)
        xs[:, :, ok] = x[:, :, pos[ok]]
        if fault == "halo_wrong_side" and sl > 0:            # the two left halo columns of a later slice hold the right halo's values
            xs[:, :, :2] = xs[:, :, dc + 2:].clone()
        h1 = aff(_conv_valid(xs, w1, b1, flip), s1, t1)      # positions d0 - 1 .. d0 + dc
        hp = pos[1:-1]
        if fault != "hidden_halo_from_bias":
            h1[:, :, (hp < 0) | (hp >= D)] = 0
        pred[:, :, d0:d0 + dc] = aff(_conv_valid(h1, w2, b2, flip), s2, t2)
    out = {}
    final = pred
    if c.variant == 1:
        sp_w0, sp_b0, sp_w1, sp_b1, tc_w0, tc_b0, tc_w1, tc_b1, tm_w0, tm_b0, tm_w1, tm_b1 = (v.to(dt) for v in inp["mem"])
        ch = c.chunk
        first = 0 if fault == "mem_first_chunk" else P - ch
        flat = x[:, first:first + ch, :].reshape(B, -1)
        m = _dot_rows(sp_w1, _dot_rows(sp_w0, flat, flip) + sp_b0, flip) + sp_b1
        mem = _dot_rows(tc_w1, _dot_rows(tc_w0, flat, flip) + tc_b0, flip) + tc_b1
        pr = pred[:, :ch] * m[:, None, :]
        dot = (pr.flip(2) if flip else pr).sum(2)
        s = (1.0 / (1.0 + torch.exp(-dot)))[..., None]
        g = pred.clone()
        g[:, :ch] = s * pred[:, :ch] + (1.0 - s) * m[:, None, :]
        src = pred if fault == "pe_ungated" else g
        pe = _dot_rows(tm_w1, _dot_rows(tm_w0, src[:, :ch].reshape(B, -1), flip) + tm_b0, flip) + tm_b1
        if fault == "gram_own_clip":
            score = torch.stack([mem[b] @ (mem[b][:, None] * pe[b][None, :]) for b in range(B)])
            gram = mem.t() @ pe
        else:
            gram = (mem.flip(0).t() @ pe.flip(0)) if flip else mem.t() @ pe
            score = _dot_rows(gram.t().contiguous(), mem, flip)
        e = torch.exp(score - score.max(1, keepdim=True).values)
        w = (e / (e.flip(1) if flip else e).sum(1, keepdim=True))[..., None]
        final = g.clone()
        final[:, :ch] = g[:, :ch] * w if fault == "row_times_w" else g[:, :ch] + g[:, :ch] * w
        out.update(tm_mem=mem, tm_pe=pe, tm_gram=gram)
    cat = torch.full((B, P + PL, c.Dpad), float("nan"), dtype=dt)
    if fault != "pad_unwritten":
        cat[:, :, D:] = 0
    cat[:, :P, :D], cat[:, P:, :D] = x, final
    out["cat"] = cat
    return out


# =========================================================================================================================================
# 2. contrastive loss
# =========================================================================================================================================
ConCase = namedtuple("ConCase", "n d why")
CON_CASES = [
    ConCase(1, 1, "a single element: loss 0, acc 1"),
    ConCase(12, 1, "d = 1: every normalised value is +-1, D is 0 or 2 -- held one-sidedly and to finiteness"),
    ConCase(2, 3, "the smallest off-diagonal"),
    ConCase(12, 64, "the golden shape's neighbourhood: one column per thread, most threads idle"),
    ConCase(255, 3, "one column short of every thread owning one"),
    ConCase(256, 64, "every thread owns exactly one column"),
    ConCase(257, 3, "row 256: its diagonal is thread 0's SECOND column (i % 256)"),
    ConCase(300, 257, "a d-loop longer than 256 (the staging and the norm tree take two turns) and 44 diagonals owned as second columns"),
    ConCase(2, 257, "the long d-loop with one idle row of threads"),
    ConCase(12, 300, "d = 300"),
]
CON_CLASSES = ("generic", "near", "ties", "zero_row", "identical")
CON_GRAD_FACTOR = 4.0
# Worst |torch float32 CPU autograd - con_grads_f64| per input class in units of con_grad_unit over CON_GRAD_MEASURE (tests/test_misc_f64.py
# re-measures them):
CON_GRAD_CPU_F32 = {"generic": 1.67e-6, "ties": 1.81e-5, "zero_row": 2.38e-5, "identical": 6.20e-6}
CON_GRAD_NEAR_ABS = 1e-30       # the near class: every softmax row is one-hot to e^-99, the float64 gradients are below 1e-36 -- nothing but denormals
# The gradient cases: d = 1 is left out (the projection annihilates the gradient), and so are the d = 3 cases with hundreds of rows: that many
# directions cannot be kept apart in three dimensions, chance pairs at D ~ 1e-3 make a row's softmax ill-conditioned (c^2 E_D ~ 1), and torch's own
# float32 gradient is off by more than the row's rms there (measured: 1.4 to 1.7 units at 255 x 3 and 257 x 3).
CON_GRAD_CASES = [c for c in CON_CASES if c.d >= 64 or c.n == 2]
CON_GRAD_MEASURE = CON_GRAD_CASES


def con_classes_for(case):
    """d = 1 and n = 1 run the generic class alone (nothing else can be built there)."""
    return ("generic",) if case.d == 1 or case.n == 1 else CON_CLASSES


def con_tie_rows(n):
    """-> [(face row r, audio rows (j, j2))]: audio row j2 is a bit copy of row j and face row r lies next to both, so both hold r's maximum.
    r = j: the lower index is the diagonal (a hit that a last-index argmax loses); r = j2: the lower index is not (a miss that it would win).
    n >= 260: j2 = j + 256 (the same thread's two columns) as well as neighbours (different threads)."""
    if n < 2:
        return []
    if n < 8:
        return [(1, (0, 1))]
    t = [(3, (3, 4)), (6, (5, 6))]
    if n >= 264:
        t += [(1, (1, 257)), (263, (7, 263))]
    return t


def con_inputs(n, d, cls):
    """-> face, audio (fp32).  generic: correlated rows, distances near sqrt 2 off the diagonal; near: every pair (i, i) at distance ~1e-2; ties:
    con_tie_rows on top of generic; zero_row: face row n // 2 all zero; identical: face row n - 1 a bit copy of audio row n - 1."""
    key = f"con{n}x{d}{cls}"
    base = T(key + "b", (n, d))
    face = (base + 0.5 * T(key + "f", (n, d))).float()
    audio = (base + 0.5 * T(key + "a", (n, d))).float()
    if cls == "near":
        fd = face.double()
        nz = T(key + "n", (n, d)).double()
        nz = nz - fd * (nz * fd).sum(1, keepdim=True) / fd.pow(2).sum(1, keepdim=True)          # across the row: the normalisation removes what lies along it
        audio = (fd + 1e-2 * fd.norm(dim=1, keepdim=True) * nz / nz.norm(dim=1, keepdim=True).clamp(min=1e-30)).float()
    elif cls == "ties":
        for r, (j, j2) in con_tie_rows(n):
            audio[j2] = audio[j]
            ad = audio[j].double()
            nz = T(key + f"t{r}", (d,)).double()
            nz = nz - ad * (nz * ad).sum() / ad.pow(2).sum()
            face[r] = (ad + 3e-2 * ad.norm() * nz / nz.norm().clamp(min=1e-30)).float()
    elif cls == "zero_row":
        face[n // 2] = 0.0
    elif cls == "identical":
        face[n - 1] = audio[n - 1]
    elif cls != "generic":
        raise ValueError(cls)
    return face, audio


def _chain(t, axis, flip=False):
    """The sum of t along axis as ONE chain of additions in t's precision; flip: backwards.  (numpy's accumulate adds one element after the other
    in the array's type; torch.cumsum on the CPU accumulates float32 in double.)"""
    if t.shape[axis] == 0 or t.dtype == F64:         # float64 is the reference: a plain sum
        return t.sum(axis)
    a = (t.flip(axis) if flip else t).contiguous().numpy()
    return torch.from_numpy(np.ascontiguousarray(np.take(np.add.accumulate(a, axis=axis, dtype=a.dtype), -1, axis=axis)))


def _chain4(t, axis, flip=False):
    """Four interleaved chains (index % 4) combined pairwise: the gradient sums of the backward kernels."""
    n = t.shape[axis]
    p = [_chain(t.index_select(axis, torch.arange(r, max(n, r), 4)), axis, flip) for r in range(4)]
    return (p[0] + p[1]) + (p[2] + p[3])


def _dist_rows(fh, ah, flip=False, block=32, four=False):
    """|fh_i - ah_j| for every pair by explicit differences (no Gram-matrix cancellation), the squares added in one chain over k (the forward
    kernel's serial loop; four: in four interleaved chains, the backward's), a block of rows at a time."""
    out = []
    for i0 in range(0, fh.shape[0], block):
        t = fh[i0:i0 + block, None, :] - ah[None, :, :]
        out.append(torch.sqrt((_chain4 if four else _chain)(t * t, 2, flip)))
    return torch.cat(out)


def _tree(t, flip=False):
    """A 256-slot workgroup reduction of the last axis: slot s adds its terms s, s + 256, ... in a chain, the slots meet in a halving tree."""
    if t.dtype == F64:
        return t.sum(-1)
    n = t.shape[-1]
    nl = cdiv(n, 256)
    p = torch.zeros(t.shape[:-1] + (nl * 256,), dtype=t.dtype)
    p[..., :n] = t
    acc = _chain(p.view(t.shape[:-1] + (nl, 256)), -2, flip)
    h = 128
    while h:
        acc = (acc[..., h:2 * h] + acc[..., :h]) if flip else (acc[..., :h] + acc[..., h:2 * h])
        h //= 2
    return acc[..., 0]


def con_forward(face, audio, dt=F64, flip=False, fault=None, backward=False):
    """-> dict: cross [n, n], rowloss [n], hit [n] (first-index argmax == i), loss, acc, and fh, ah, D, finv, ainv.  The sums run as the kernels
    order them: the face norm by the 256-slot tree, the audio norm by one chain, the distance by one chain over k (backward: the audio norm by the
    tree and the distance in four interleaved chains, as the backward kernels have them), the row's exponentials and the mean over the rows by the tree.  faults: "argmax_last", "diag_minus_256", "no_max"."""
    f, a = face.to(dt), audio.to(dt)
    n = f.shape[0]
    finv = 1.0 / torch.clamp(torch.sqrt(_tree(f * f, flip)), min=1e-12)[:, None]
    ainv = 1.0 / torch.clamp(torch.sqrt(_tree(a * a, flip) if backward else _chain(a * a, 1, flip)), min=1e-12)[:, None]
    fh, ah = f * finv, a * ainv
    D = _dist_rows(fh, ah, flip, four=backward)
    c = torch.clamp(1.0 / (D + 1e-8), min=1e-8)
    m = c.max(1, keepdim=True).values
    if fault == "argmax_last":
        am = n - 1 - c.flip(1).argmax(1)
    else:
        am = c.argmax(1)
    e = torch.exp(c) if fault == "no_max" else torch.exp(c - m)
    se = _tree(e, flip)
    idx = torch.arange(n)
    di = torch.where(idx >= 256, idx - 256, idx) if fault == "diag_minus_256" else idx
    row = (torch.log(se) if fault == "no_max" else m[:, 0] + torch.log(se)) - c[idx, di]
    hit = (am == idx)
    loss = _tree(row, flip) / n
    return {"cross": c, "rowloss": row, "hit": hit, "loss": loss, "acc": hit.to(dt).sum() / n, "fh": fh, "ah": ah, "D": D, "finv": finv, "ainv": ainv, "m": m[:, 0],
            "se": se}


def _pair_sums(W, x, y, flip, fma):
    """out[i, k] = sum_j W[i, j] (x[i, k] - y[j, k]) in four interleaved chains over j (j % 4) combined pairwise, as the backward kernels sum it.
    fma: every multiply-add is fused (the product exact, one rounding), which is what the compiler makes of acc += w * t."""
    n = y.shape[0]
    if x.dtype == F64:
        return torch.stack([(W * (x[:, k:k + 1] - y[None, :, k])).sum(1) for k in range(x.shape[1])], 1)
    acc = [torch.zeros_like(x) for _ in range(4)]
    for j in (reversed(range(n)) if flip else range(n)):
        w, t = W[:, j:j + 1], x - y[j][None, :]
        acc[j % 4] = (w.double() * t.double() + acc[j % 4].double()).to(x.dtype) if fma else acc[j % 4] + w * t
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def con_grads(face, audio, dt=F64, flip=False, fault=None, fma=False):
    """d loss / d face, d loss / d audio by the closed form (csrc/misc.hip, above contrastive_norms_kernel) and W [n, n]: both norms by the tree,
    g_fh_i = sum_j W_ij (fh_i - ah_j) and g_ah_j = -sum_i W_ij (fh_i - ah_j) term by term in four interleaved chains each (fma: fused multiply-adds), the
    projection's inner product by the tree.  faults: "no_projection", "through_zero" (dD/dx = (x - y) / D at D = 0), "factored_sum" (fh_i sum_j W_ij - sum_j W_ij ah_j with
    fused multiply-adds: the kernels' form before these tests.  Its terms are of size |W| where those of the sum above are of size |W| D, so
    next to an audio row -- two tied columns at D = 0.03 -- the rounding it is left with is 1 / D times larger)."""
    r = con_forward(face, audio, dt, flip, backward=True)
    n = face.shape[0]
    c, D, fh, ah = r["cross"], r["D"], r["fh"], r["ah"]
    e = torch.exp(c - r["m"][:, None])
    G = (e / r["se"][:, None] - torch.eye(n, dtype=dt)) / n
    live = (1.0 / (D + 1e-8)) > 1e-8
    if fault != "through_zero":
        live = live & (D > 0)
    W = torch.where(live, -G * c * c / D, torch.zeros_like(D))
    if fault == "factored_sum":
        def fused(Wm, y):           # sum_j Wm[i, j] y[j, k] as one chain of fused multiply-adds
            acc = torch.zeros(Wm.shape[0], y.shape[1], dtype=dt)
            for j in range(y.shape[0]):
                acc = (Wm[:, j:j + 1].double() * y[j][None, :].double() + acc.double()).to(dt)
            return acc
        g_fh = fh * _tree(W, flip)[:, None] - fused(W, ah)
        g_ah = ah * _tree(W.t().contiguous(), flip)[:, None] - fused(W.t(), fh)
    else:
        g_fh, g_ah = _pair_sums(W, fh, ah, flip, fma), _pair_sums(W.t(), ah, fh, flip, fma)
    if fault == "no_projection":
        gf, ga = g_fh * r["finv"], g_ah * r["ainv"]
    else:
        gf = (g_fh - fh * _tree(fh * g_fh, flip)[:, None]) * r["finv"]
        ga = (g_ah - ah * _tree(ah * g_ah, flip)[:, None]) * r["ainv"]
    return {"gface": gf, "gaudio": ga, "W": W, "D": D, "fh": fh, "ah": ah, "finv": r["finv"], "ainv": r["ainv"]}


def con_torch(face, audio, dt):
    """The loss as the reference module states it, in torch ops of precision dt, and its autograd gradients -> (loss, gface, gaudio)."""
    f, a = face.to(dt).clone().requires_grad_(True), audio.to(dt).clone().requires_grad_(True)
    fh, ah = TF.normalize(f, p=2, dim=1), TF.normalize(a, p=2, dim=1)
    dist = torch.norm(fh[:, None, :] - ah[None, :, :], p=2, dim=2)
    c = torch.clamp(1.0 / (dist + 1e-8), min=1e-8)
    loss = TF.cross_entropy(c, torch.arange(f.shape[0]))
    loss.backward()
    return loss.detach(), f.grad, a.grad


def con_grad_terms(g):
    """-> (A_face [n, d], A_audio [n, d]): the terms of each gradient element taken in magnitude, A_ik = sum_j |W_ij| |fh_ik - ah_jk| / |f_i| (and the
    same down the columns for the audio rows), carried through the projection (A_ik + |xh_ik| sum_k' |xh_ik'| A_ik'), from a float64 con_grads result and its inputs' normalised rows."""
    W, fh, ah = g["W"].abs(), g["fh"], g["ah"]
    af = torch.stack([(W * (fh[:, k:k + 1] - ah[None, :, k]).abs()).sum(1) for k in range(fh.shape[1])], 1) * g["finv"]
    aa = torch.stack([(W * (fh[:, k:k + 1] - ah[None, :, k]).abs()).sum(0) for k in range(fh.shape[1])], 1) * g["ainv"]
    through = lambda t, xh: t + xh.abs() * (xh.abs() * t).sum(1, keepdim=True)         # g - xh <xh, g> carries every element's error into every other
    return through(af, fh), through(aa, ah)


def con_grad_units(g):
    """-> (unit of gface, unit of gaudio), per element: the rms of the element's row of the float64 gradient, floored at u x the rms of the row's
    terms in magnitude (con_grad_terms) and at 2^-126.  The floor is the rounding of the terms themselves: where they cancel (two tied columns
    pull a face row in opposite directions with equal weight: the float64 gradient is 0) nothing finer can be asked."""
    out = []
    for grad, terms in zip((g["gface"], g["gaudio"]), con_grad_terms(g)):
        rms = lambda t: t.double().pow(2).mean(1, keepdim=True).sqrt()
        out.append(torch.maximum(torch.maximum(rms(grad), U * rms(terms)), torch.tensor(FLT_MIN, dtype=F64)).expand(grad.shape))
    return out


def con_grad_tols(g, cls):
    """-> (tolerance of gface, of gaudio), per element: CON_GRAD_FACTOR x the float32 CPU error of the class in the units above, plus 4 u x the
    element's own terms in magnitude.  The second part is what an implementation with fused multiply-adds needs where two terms cancel exactly:
    torch rounds both products and their sum is 0; a fused chain keeps the second product exact and is left with the rounding of the first."""
    return [con_grad_tol(cls) * unit + 4 * U * terms for unit, terms in zip(con_grad_units(g), con_grad_terms(g))]


def con_grad_tol(cls):
    return CON_GRAD_FACTOR * CON_GRAD_CPU_F32[cls]


def con_bounds(face, audio):
    """-> (reference dict of con_forward, bounds dict: cross [n, n] (inf where vacuous), cross_floor [n, n] (the one-sided statement), rowloss [n]
    (inf where the row is only held to finiteness), loss (a number, inf likewise), decided [n] bool, row_kind [n]: 0 bounded, 1 only the diagonal
    vacuous, 2 finiteness only)."""
    r = con_forward(face, audio)
    n, d = face.shape
    fh, ah, D, c = r["fh"], r["ah"], r["D"], r["cross"]
    rel = lambda L: (0.5 * (L + 1) + 3) * U
    r_f, r_a = rel(cdiv(d, 256) + 8), rel(max(d, cdiv(d, 256) + 8))
    e_dist = torch.empty_like(D)
    for i0 in range(0, n, 32):
        t = (fh[i0:i0 + 32, None, :] - ah[None, :, :]).abs()
        e_t = fh[i0:i0 + 32, None, :].abs() * (r_f + 2 * U) + ah[None, :, :].abs() * (r_a + 2 * U) + 2 * U * t
        e_dist[i0:i0 + 32] = (2 * t * e_t + e_t * e_t).sum(2)
    e_dist = e_dist + (d + 2) * U * D * D
    E_D = torch.minimum(e_dist / torch.clamp(D, min=1e-300), torch.sqrt(e_dist)) + 2 * U * D
    x = D + 1e-8
    delta = E_D + 2 * U * x
    vac = delta >= 0.5 * x
    e_c = torch.where(vac, torch.full_like(c, float("inf")), c * delta / torch.clamp(x - delta, min=1e-300) + 2 * U * c)
    e_c = torch.where(c <= 1e-8, torch.full_like(c, U * 1e-8), e_c)
    floor = (1 - 4 * U) / (D + E_D + 1e-8)
    idx = torch.arange(n)
    off = vac.clone()
    off[idx, idx] = False
    kind = torch.where(off.any(1), 2, torch.where(vac[idx, idx], 1, 0))
    m, se = r["m"], r["se"]
    lse = m + torch.log(se)
    p = torch.exp(c - m[:, None]) / se[:, None]
    ecz = torch.nan_to_num(e_c, posinf=0.0)
    rho_se = (FN + U * (c - m[:, None]).abs()).max(1).values + (cdiv(n, 256) + 9) * U
    e_row = (p * ecz).sum(1) + ecz[idx, idx] + rho_se + FN * torch.log(se).abs() + 2 * U * (m.abs() + torch.log(se).abs() + lse.abs() + c[idx, idx].abs())
    e_row = torch.where(kind == 2, torch.full_like(e_row, float("inf")), torch.where(kind == 1, torch.full_like(e_row, 8 * U), e_row))
    row = r["rowloss"]
    if bool((kind == 2).any()):
        e_loss = float("inf")
    else:
        e_loss = float(e_row.mean() + (cdiv(n, 256) + 10) * U * row.abs().mean() + 2 * U * r["loss"].abs())
    # decided rows: the margin of the two largest values against their bounds, or bit-identical audio rows behind them
    top = torch.topk(c, min(2, n), dim=1)
    if n == 1:
        decided = torch.ones(1, dtype=torch.bool)
    else:
        i1, i2 = top.indices[:, 0], top.indices[:, 1]
        margin = top.values[:, 0] - top.values[:, 1]
        same = (audio[i1].view(torch.int32) == audio[i2].view(torch.int32)).all(1)
        decided = same | (margin > ecz[idx, i1] + e_c[idx, i2]) | ((kind == 1) & (i1 == idx))
        decided = decided & ((kind != 2) | same)
    return r, {"cross": e_c, "cross_floor": floor, "vacuous": vac, "rowloss": e_row, "loss": e_loss, "decided": decided, "row_kind": kind}


# =========================================================================================================================================
# 3. small linear   (n, In, Out, ldx, ldy, column offset of y in its row)
# =========================================================================================================================================
CVAE_Q = (16, 48, 128)          # d_model / 4 of the three generator widths the CVAE is built for
SL_CASES = [(2, 8, 16, 8, 16, 0), (2, 16, 32, 16, 64, 32), (2, 64, 128, 64, 128, 0)] + \
           [(2, 128, 4 * q, 128, 4 * q, 0) for q in CVAE_Q] + [(2, 4 * q, 128, 4 * q, 128, 0) for q in CVAE_Q] + \
           [(3, 70, 5, 77, 9, 2), (1, 1, 1, 1, 1, 0), (2, 65, 4, 65, 4, 0)]          # In % 64 != 0 with ldx > In, ldy > Out; one term; one lane with two terms


def sl_inputs(case):
    n, In, Out, ldx, ldy, col = case
    key = "sl" + "_".join(map(str, case))
    a = 1.0 / np.sqrt(In)
    return T(key + "x", (n, In)), T(key + "w", (Out, In), -a, a), T(key + "b", (Out,), -1, 1)


def sl_eval(x, w, b, dt=F64, flip=False, fault=None):
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    return _dot_rows(w, x, flip) + (64.0 * b if fault == "bias_per_lane" else b)


def sl_bound(x, w, b):
    return K(x.shape[1]) * U * (x.double().abs() @ w.double().abs().t()) + 2 * U * sl_eval(x, w, b).abs()


# =========================================================================================================================================
# 4. transposed convolution   (n, cin, cout, lin)
# =========================================================================================================================================
CT_LIN = (1, 16, 63, 64, 65, 128)       # 2 lin outputs in workgroups of 128: 64 | 65 is the workgroup boundary, 63 one short of it
CT_CASES = [(2, 4, 8, l) for l in CT_LIN] + [(2, 8, 16, l) for l in CT_LIN] + [(2, 4, 8, q) for q in (48,)] + [(2, 8, 16, 2 * q) for q in (48, 128)]
CT_AXES = ("sample", "channel", "position")


def ct_inputs(case):
    n, cin, cout, lin = case
    key = "ct" + "_".join(map(str, case))
    a = 1.0 / np.sqrt(2 * cin)
    return (T(key + "x", (n, cin, lin)), T(key + "w", (cin, cout, 3), -a, a), T(key + "b", (cout,), -0.5, 0.5),
            _signed(key + "s", (cout,), 0.5, 1.5), T(key + "t", (cout,), -0.5, 0.5))


def ct_f64(x, w, b, sc, sh):
    y = TF.conv_transpose1d(x.double(), w.double(), b.double(), stride=2, padding=1, output_padding=1)
    return TF.leaky_relu(y, 0.2) * sc.double().view(1, -1, 1) + sh.double().view(1, -1, 1)


def ct_bound(x, w, b, sc, sh):
    cin = x.shape[1]
    mag = TF.conv_transpose1d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=1, output_padding=1)
    return (3 * cin + 4) * U * mag * torch.clamp(sc.double().abs(), min=1.0).view(1, -1, 1) + U * ct_f64(x, w, b, sc, sh).abs()


def emulate_ct(x, w, b, sc, sh, dt=torch.float32, flip=False, fault=None):
    """convt1d_kernel's sum stated per output parity: output 2 j takes tap 1 of x[j]; output 2 j + 1 takes tap 0 of x[j + 1] (dropped at
    j + 1 == lin) and tap 2 of x[j].  faults: "parity" (the taps of even and odd outputs exchanged), "keep_lin" (the dropped term is kept and reads
    the element behind the row in memory; behind the last row: 1)."""
    x, w, b, sc, sh = (v.to(dt) for v in (x, w, b, sc, sh))
    n, cin, lin = x.shape
    if flip:
        x, w = x.flip(1), w.flip(0)
    nxt = torch.zeros_like(x)
    nxt[:, :, :-1] = x[:, :, 1:]
    if fault == "keep_lin":
        flat = torch.cat([x.reshape(-1), torch.ones(1, dtype=dt)])
        nxt[:, :, -1] = flat[(torch.arange(n * cin) + 1) * lin].view(n, cin)
    mm = lambda xx, k: torch.einsum("ncl,co->nol", xx, w[:, :, k])
    even, odd = mm(x, 1), mm(nxt, 0) + mm(x, 2)
    if fault == "parity":
        even, odd = odd, even
    y = torch.stack([even, odd], 3).reshape(n, w.shape[1], 2 * lin) + b.view(1, -1, 1)
    return TF.leaky_relu(y, 0.2) * sc.view(1, -1, 1) + sh.view(1, -1, 1)


# =========================================================================================================================================
# 5. embedding   (rows, dim, ld)
# =========================================================================================================================================
EMB_CASES = [(180, 300, 320), (1, 4, 64), (64, 64, 64), (65, 64, 128)]
EMB_WORDS = 11


def emb_inputs(case):
    """-> idx int64 [rows] (with -1, 0, n_words - 1, n_words and 2^40 among them), table [n_words, dim] whose rows no clamped index reads are NaN."""
    rows, dim, ld = case
    edge = [-1, 0, EMB_WORDS - 1, EMB_WORDS, 2 ** 40]
    idx = torch.tensor([edge[r] if r < len(edge) else 2 + (r * 5) % 4 for r in range(rows)], dtype=torch.int64) if rows > 1 else torch.tensor([2 ** 40])
    table = T(f"emb{rows}x{dim}", (EMB_WORDS, dim))
    used = torch.zeros(EMB_WORDS, dtype=torch.bool)
    used[idx.clamp(0, EMB_WORDS - 1)] = True
    table[~used] = float("nan")
    return idx, table


def emb_rows(idx, table):
    return table[idx.clamp(0, table.shape[0] - 1)]
