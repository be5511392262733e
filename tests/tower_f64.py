"""Test-side float64 restatement of the audio tower's training sites (Full_model/ResNetSE34V2.py:62-74, ResNetBlocks.py:21-37, the final
final_conv1 -> bn1 of Models_spatial_memory.py:121-123) and a comparison that localises an error.  A helper module of the tower tests (not
collected: no test_ prefix).

  stem   conv1(+bias) -> ReLU -> bn1
  block  conv1 (stride s) -> ReLU -> bn1 -> conv2 -> bn2 -> SE gate -> * gate + shortcut -> ReLU; the shortcut is the block input or, with a
         downsample branch, bn(conv1x1 stride s)
  final  final_conv1(+bias) -> bn1

BatchNorm in train mode (batch statistics; running buffers updated with momentum 0.1 and the unbiased variance, as nn.BatchNorm2d does).
Everything runs in torch float64 on the CPU, NCHW, with the reference's parameter names relative to the site.  `run_site` returns full tensors:
the output, the input gradient, every parameter gradient, the updated running statistics, the ReLU masks (conv1's "r1" and the block's last
"out") and the pre-activations behind them.

`masks` (optional) replaces the ReLU decisions: the comparison with a GPU forward runs the reference on the GPU's own masks, so that an
element both sides place within rounding of zero (a "flip") does not move everything upstream of it; `check_flips` then holds those elements
to a count and to a rounding-sized pre-activation.

`compare(got, ref, bounds, what)` checks three things: relative L2 over the whole tensor; relative L2 per slice -- per output channel and per
3x3 tap of a weight gradient, per channel x {first row, last row, first column, last column, each 32-column tile (the convolutions' tile
width)} of a map; and max |got - ref| / rms(ref).
"""
import numpy as np
import torch
import torch.nn.functional as TF

MOMENTUM, EPS = 0.1, 1e-5
TILE_W = 32

# Bounds of `compare` per precision.  whole: the site test's relative-L2 tolerances.  slice / elem: >= 3x the worst values measured on the
# MI355X over the 15 sites of tests/golden/tower_grads.npz and the 12 cases of test_tower_shapes_backward_matches_float64 (both tests print them):
#   f32     slice 8.3e-6 (layer1.2 B=25 dconv1.weight), element 1.6e-4 (layer1.1 B=16 dbn1.bias), whole 6.3e-5 (layer1.1 B=16 dbn1.bias)
#   bf16x3  slice 3.2e-5 (layer3.3 golden crop dconv1.weight), element 9.1e-4 (same tensor), whole 9.9e-5 (layer1.2 B=25 dbn1.bias)
# The worst whole and element values sit on bn1's bias gradient: a sum over the map of conv2's input gradient, which bn2's mean subtraction makes
# nearly cancel (border terms remain), so its relative error is large in any fp32 arithmetic -- torch's fp32 CPU path is at 5.7e-4 on that tensor.
BOUNDS = {"f32": dict(whole=1e-4, slice=3e-5, elem=5e-4), "bf16x3": dict(whole=3e-4, slice=1e-4, elem=3e-3)}

# A flipped ReLU element is a pre-activation the two forwards place on different sides of zero; it must be rounding-sized: |pre| below this
# fraction of the rms of its map (the f32 convolutions differ from float64 by ~1e-6 of it).
FLIP_PRE_REL = 1e-4


# ---- parameters ----------------------------------------------------------------------------------------------------------------
def site_prefix(site):
    if site == "final":
        return "audio_encoder."
    if site == "stem":
        return "audio_encoder.feat_extractor."
    return f"audio_encoder.feat_extractor.{site}."


def site_state(sd, site):
    """sd: a generator state_dict (CPU) -> (params {name: float64 leaf}, running {bn name: (mean, var) float64}), names relative to the site."""
    p = site_prefix(site)
    if site == "stem":
        names = ["conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias"]
        bns = ["bn1"]
    elif site == "final":
        names = ["final_conv1.weight", "final_conv1.bias", "bn1.weight", "bn1.bias"]
        bns = ["bn1"]
    else:
        names = ["conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "se.fc.0.weight", "se.fc.0.bias", "se.fc.2.weight",
                 "se.fc.2.bias"]
        bns = ["bn1", "bn2"]
        if p + "downsample.0.weight" in sd:
            names += ["downsample.0.weight", "downsample.1.weight", "downsample.1.bias"]
            bns += ["downsample.1"]
    params = {k: sd[p + k].detach().double().clone().requires_grad_(True) for k in names}
    running = {b: (sd[p + b + ".running_mean"].detach().double().clone(), sd[p + b + ".running_var"].detach().double().clone()) for b in bns}
    return params, running


# ---- the sites -----------------------------------------------------------------------------------------------------------------
def run_site(site, params, running, x, g, stride=1, masks=None):
    """x, g: NCHW (any float dtype; promoted to float64).  -> dict(out, dx, grads, running, masks, pre), all float64 NCHW / the parameters' shapes."""
    P = params
    for t in P.values():
        t.grad = None
    run = {k: (m.clone(), v.clone()) for k, (m, v) in running.items()}
    pre, used = {}, {}

    def relu(t, key):
        pre[key] = t.detach()
        m = (t.detach() > 0) if masks is None or key not in masks else masks[key].to(torch.bool)
        used[key] = m
        return t * m.to(t.dtype)

    def bn(t, name):
        rm, rv = run[name]
        return TF.batch_norm(t, rm, rv, P[name + ".weight"], P[name + ".bias"], True, MOMENTUM, EPS)

    xi = x.detach().double().clone().requires_grad_(True)
    if site == "stem":
        out = bn(relu(TF.conv2d(xi, P["conv1.weight"], P["conv1.bias"], padding=1), "r1"), "bn1")
    elif site == "final":
        out = bn(TF.conv2d(xi, P["final_conv1.weight"], P["final_conv1.bias"], padding=1), "bn1")
    else:
        b1 = bn(relu(TF.conv2d(xi, P["conv1.weight"], None, stride=stride, padding=1), "r1"), "bn1")
        b2 = bn(TF.conv2d(b1, P["conv2.weight"], None, padding=1), "bn2")
        h = TF.relu(TF.linear(b2.mean(dim=(2, 3)), P["se.fc.0.weight"], P["se.fc.0.bias"]))
        gate = torch.sigmoid(TF.linear(h, P["se.fc.2.weight"], P["se.fc.2.bias"]))
        res = xi if "downsample.0.weight" not in P else bn(TF.conv2d(xi, P["downsample.0.weight"], None, stride=stride), "downsample.1")
        out = relu(b2 * gate[:, :, None, None] + res, "out")
    out.backward(g.detach().double())
    return dict(out=out.detach(), dx=xi.grad, grads={k: t.grad for k, t in P.items()}, running=run, masks=used, pre=pre)


def check_flips(pre, gpu_mask, max_frac, what):
    """gpu_mask: the GPU forward's ReLU decisions (bool, NCHW); pre: the float64 pre-activation behind them.  -> number of elements decided
    differently.  Their count is bounded relative to the map, and each must be rounding-sized."""
    fl = gpu_mask.to(torch.bool) != (pre > 0)
    n = int(fl.sum())
    assert n <= max(3, int(max_frac * pre.numel())), f"{what}: {n} of {pre.numel()} ReLU mask elements differ from the float64 forward"
    if n:
        rms = float(pre.norm()) / np.sqrt(pre.numel())
        worst = float(pre[fl].abs().max())
        assert worst <= FLIP_PRE_REL * rms, f"{what}: a flipped ReLU element has pre-activation {worst:.2e} (rms {rms:.2e}): not rounding-sized"
    return n


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _slice_errors(d, r):
    """-> [(slice family, index, ||d_s||, ||r_s||, numel of the slice)] for a map [B, C, H, W] or a weight [Co, Ci, kh, kw]."""
    out = []

    def fam(name, dd, rr, dims, idx_fmt):
        dn = dd.pow(2).sum(dim=dims).sqrt().reshape(-1)
        rn = rr.pow(2).sum(dim=dims).sqrt().reshape(-1)
        n = rr.numel() // max(1, dn.numel())
        for i in range(dn.numel()):
            out.append((name, idx_fmt(i), float(dn[i]), float(rn[i]), n))

    if d.dim() == 4 and d.shape[2:] in ((3, 3), (1, 1)):           # weight gradient [Co, Ci, kh, kw]
        fam("out channel", d, r, (1, 2, 3), lambda i: f"co {i}")
        if d.shape[2:] == (3, 3):
            fam("tap", d, r, (0, 1), lambda i: f"(kh, kw) = {divmod(i, 3)}")
    elif d.dim() == 4:                                               # map [B, C, H, W]
        Wd = d.shape[3]
        for name, sl in (("first row", (slice(None), slice(None), slice(0, 1))), ("last row", (slice(None), slice(None), slice(-1, None))),
                         ("first column", (slice(None), slice(None), slice(None), slice(0, 1))),
                         ("last column", (slice(None), slice(None), slice(None), slice(-1, None)))):
            fam(name, d[sl], r[sl], (0, 2, 3), lambda i, n=name: f"channel {i}")
        for t0 in range(0, Wd, TILE_W):
            sl = (slice(None), slice(None), slice(None), slice(t0, t0 + TILE_W))
            fam(f"columns {t0}..{min(Wd, t0 + TILE_W) - 1}", d[sl], r[sl], (0, 2, 3), lambda i: f"channel {i}")
    return out


def errors(got, ref):
    """-> (whole relative L2, (worst slice relative L2, its description), max |d| / rms(ref)).  A slice is measured against at least 1 % of
    its fair share of the norm (a slice with a near-zero reference is not divided by zero)."""
    r = ref.detach().double().cpu()
    d = got.detach().double().cpu().reshape(r.shape) - r
    rn = float(r.norm())
    whole = float(d.norm()) / max(rn, 1e-300)
    rms = rn / np.sqrt(max(1, r.numel()))
    elem = float(d.abs().max()) / max(rms, 1e-300) if r.numel() else 0.0
    worst = (0.0, "")
    for fam, idx, dn, sn, n in _slice_errors(d, r):
        e = dn / max(sn, 1e-2 * rn * np.sqrt(n / r.numel()), 1e-300)
        if e > worst[0]:
            worst = (e, f"{fam}, {idx}")
    return whole, worst, elem


def compare(got, ref, bounds, what):
    """Assert the three checks; -> (whole, slice, element) errors for reporting."""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got.detach().cpu()).all()), f"{what}: non-finite values"
    whole, (sl, where), elem = errors(got, ref)
    assert whole <= bounds["whole"], f"{what}: relative L2 {whole:.2e} > {bounds['whole']:.0e}"
    assert sl <= bounds["slice"], f"{what}: slice relative L2 {sl:.2e} > {bounds['slice']:.0e} at {where}"
    assert elem <= bounds["elem"], f"{what}: max |d| / rms {elem:.2e} > {bounds['elem']:.0e}"
    return whole, sl, elem


def fp_check(z, key, got, tol, what):
    """The golden fingerprint check: got in the reference's layout; sample and norm as written by make_golden_tower_grad.fp()."""
    v = got.detach().reshape(-1).double().cpu().numpy()
    stride = max(1, v.size // 64)
    ref_s, ref_n = z[key + "/sample"], float(z[key + "/norm"])
    e_s = np.linalg.norm(v[::stride][:64] - ref_s) / max(np.linalg.norm(ref_s), 1e-30)
    e_n = abs(np.linalg.norm(v) - ref_n) / max(ref_n, 1e-30)
    assert e_s < tol and e_n < tol, f"{what}: sample rel err {e_s:.2e}, norm rel err {e_n:.2e} (tol {tol:.0e})"
    return max(e_s, e_n)
