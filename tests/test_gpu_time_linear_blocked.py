"""time_linear_kernel (csrc/misc.hip, TextEncoderTCN.fc1: y[b,t',c] = bias[t'] + sum_t W[t',t] x[b,t,c]) through eg_time_linear: the
register-blocked kernel must return the bits of the reference kernel it replaces (EG_TIME_LINEAR=ref: same summation per output element, bias
first, then t ascending, one multiply-add per term) and agree with a float64 einsum.

Shapes: the headline's (L 60, C 320) at one and three clips; a partial channel block with ld > C (the padding columns of y stay untouched, those
of x are NaN and must not be read into a result); L = 34 (8 or 9 rows per wave: one chunk of five and a remainder of 3 or 4; not a multiple of 4);
L = 1 (three of the four waves own no row).  Biases reach 1e3 against products of order 1, so a sum that does not start from the bias, or starts
from another row's, is off by orders of magnitude more than the tolerance.

Tolerance against float64: 2e-6 of the largest |reference| of the case (max-normalised: an element is bias + 60 terms of order 1, and the
rounding of each of its L additions is relative to the running sum, which the bias dominates)."""
import numpy as np
import pytest
import torch

from emotiongestures_amd.synth import hash_uniform

pytestmark = pytest.mark.gpu

CASES = [(1, 60, 320, 320), (3, 60, 320, 320), (2, 60, 70, 128), (2, 34, 64, 64), (1, 1, 64, 64)]       # (B, L, C, ld)
SENTINEL = -6.0e30
REL_TOL = 2e-6


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(B, L, C, ld):
    x = np.full((B, L, ld), np.nan, np.float32)
    x[:, :, :C] = hash_uniform("tl.x", (B, L, C), -1.0, 1.0, L + C)
    w = hash_uniform("tl.w", (L, L), -1.0, 1.0, L)
    bias = hash_uniform("tl.b", (L,), -1e3, 1e3, L)
    return x, w, bias


def _run(x, w, bias, B, L, C, ld):
    from emotiongestures_amd import _lib as Lb
    from emotiongestures_amd.engine import _ptr, _stream
    lib = Lb.load()
    y = torch.full((B, L, ld), SENTINEL, device=dev())
    Lb.check(lib.eg_time_linear(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, L, C, ld, _stream(dev())), "eg_time_linear")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_blocked_kernel_is_bit_equal_to_the_reference_kernel_and_close_to_float64(case, monkeypatch):
    B, L, C, ld = case
    x, w, bias = _inputs(B, L, C, ld)
    xd, wd, bd = (torch.from_numpy(a).to(dev()) for a in (x, w, bias))
    monkeypatch.delenv("EG_TIME_LINEAR", raising=False)
    new = _run(xd, wd, bd, B, L, C, ld)
    monkeypatch.setenv("EG_TIME_LINEAR", "ref")
    ref_kernel = _run(xd, wd, bd, B, L, C, ld)
    monkeypatch.delenv("EG_TIME_LINEAR")
    assert torch.equal(new, ref_kernel), f"{case}: {int((new != ref_kernel).sum())} elements differ from the reference kernel"
    got = new.cpu().numpy()
    assert np.all(got[:, :, C:] == np.float32(SENTINEL)), f"{case}: a padding column of y was written"
    ref = bias.astype(np.float64)[None, :, None] + np.einsum("pt,btc->bpc", w.astype(np.float64), x[:, :, :C].astype(np.float64))
    err = float(np.abs(got[:, :, :C] - ref).max() / np.abs(ref).max())
    print(f"time_linear {case}: max |d| / max |ref| = {err:.3e}")
    assert np.isfinite(got[:, :, :C]).all()
    assert err <= REL_TOL, f"{case}: {err:.3e} of the largest reference value"


def test_unknown_switch_value_is_refused(monkeypatch):
    from emotiongestures_amd import _lib as Lb
    from emotiongestures_amd.engine import _ptr, _stream
    lib = Lb.load()
    B, L, C, ld = CASES[-1]
    x, w, bias = (torch.from_numpy(a).to(dev()) for a in _inputs(B, L, C, ld))
    y = torch.full((B, L, ld), SENTINEL, device=dev())
    monkeypatch.setenv("EG_TIME_LINEAR", "fast")
    rc = lib.eg_time_linear(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, L, C, ld, _stream(dev()))
    monkeypatch.delenv("EG_TIME_LINEAR")
    torch.cuda.synchronize()
    assert rc == -1 and b"EG_TIME_LINEAR" in lib.eg_last_error()
    assert bool((y == SENTINEL).all())
