"""The front half of Prior_MemoryEncoder on the GPU -- prior_pred_kernel, tm_gram_kernel, tm_apply_kernel of csrc/misc.hip through eg_prior_encoder
-- every ELEMENT against float64 (tests/misc_f64.py section 1: reference, bounds, cases, input conditions).  Outputs sit in canary-guarded
buffers, inputs in NaN-filled ones (the prior beyond [B, P, D] and everything around the weights is NaN), the spatial variant passes its optional
outputs as NULL."""
import pytest
import torch

import misc_f64 as M
import misc_gpu as G
import train_tail_gpu as D

pytestmark = pytest.mark.gpu
_ID = lambda c: f"v{c.variant}-{c.B}x{c.P}x{c.PL}x{c.D}-c{c.chunk}"


def _run(c, inp, what):
    L, lib, ptr, st = D.api()
    prior = G.up_nan(inp["prior"])
    conv = [G.up_nan(t) for t in inp["conv"]]
    mem = [G.up_nan(t) for t in inp["mem"]] if c.variant == 1 else None
    F = c.P + c.PL
    cat = D.Guarded((c.B, F, c.Dpad))
    extra = {k: D.Guarded(s) for k, s in (("tm_mem", (c.B, c.D)), ("tm_pe", (c.B, c.chunk)), ("tm_gram", (c.D, c.chunk)))} if c.variant == 1 else {}
    e = lambda k: ptr(extra[k].t) if k in extra else None
    rc = lib.eg_prior_encoder(ptr(prior), G.pointer_array(conv, 8), G.pointer_array(mem, 12) if mem else None, ptr(cat.t), e("tm_mem"), e("tm_pe"),
                              e("tm_gram"), c.B, c.P, F, c.D, c.Dpad, c.chunk, c.variant, st)
    return L, rc, cat, extra


@pytest.mark.parametrize("c", M.PRIOR_CASES, ids=_ID)
def test_prior_encoder_matches_float64_per_element(c):
    inp = M.prior_inputs(c)
    what = f"prior encoder {_ID(c)}"
    L, rc, cat, extra = _run(c, inp, what)
    if c.refused:
        assert rc == D.UNSUPPORTED and b"LDS need" in L.load().eg_last_error(), what
        for g in (cat, *extra.values()):
            g.untouched(what)
        return
    L.check(rc, what)
    ref, bound = M.prior_bounds(inp, c)
    got = cat.intact(what + " cat")
    D.frac("prior cat", got, ref["cat"], bound["cat"], what + " cat", M.PRIOR_AXES)
    assert torch.equal(G.bits(got[:, :c.P, :c.D]), G.bits(inp["prior"])), what + ": the prior rows of cat are not bitwise copies"
    assert bool((G.bits(got[:, :, c.D:]) == 0).all()), what + ": the pad columns are not +0"
    for k, g in extra.items():
        D.frac("prior " + k, g.intact(what + " " + k), ref[k], bound[k], what + " " + k)
    if c.variant == 1 and c.B > 1:
        # the clips of one call are coupled through tm_gram, as in the reference: clip 0 alone is another result, and the right one for a batch of 1
        c1 = c._replace(B=1)
        inp1 = dict(inp, prior=inp["prior"][:1].contiguous())
        L, rc, cat1, extra1 = _run(c1, inp1, what + " clip 0 alone")
        L.check(rc, what)
        ref1, bound1 = M.prior_bounds(inp1, c1)
        alone = cat1.intact(what + " clip 0 alone")
        D.frac("prior cat", alone, ref1["cat"], bound1["cat"], what + " clip 0 alone", M.PRIOR_AXES)
        assert M.worst(alone, got[:1], bound["cat"][:1]) > 1.0, what + ": clip 0 of the batch equals clip 0 alone -- the gram did not run over the batch"
    D.report("prior cat", *("prior " + k for k in extra))


def test_prior_encoder_refusals_write_nothing():
    """The refusals of include/emogest.h on real buffers: dpad < d, chunk past min(P, F - P, 64) (65 is never launched), memory pointers partly set."""
    c = M.PRIOR_MEMORY[0]
    inp = M.prior_inputs(c)
    L, lib, ptr, st = D.api()
    prior, conv, mem = G.up_nan(inp["prior"]), [G.up_nan(t) for t in inp["conv"]], [G.up_nan(t) for t in inp["mem"]]
    F = c.P + c.PL
    outs = [D.Guarded((c.B, F, c.Dpad)), D.Guarded((c.B, c.D)), D.Guarded((c.B, 65)), D.Guarded((c.D, 65))]
    call = lambda mm, P, Fr, dpad, chunk: lib.eg_prior_encoder(ptr(prior), G.pointer_array(conv, 8), mm, *(ptr(o.t) for o in outs), c.B, P, Fr, c.D, dpad,
                                                               chunk, 1, st)
    full = G.pointer_array(mem, 12)
    assert call(full, c.P, F, c.D - 1, c.chunk) == D.BAD_ARG and b"dpad" in lib.eg_last_error()
    assert call(full, 100, 128, c.Dpad, 65) == D.BAD_ARG and b"chunk=65" in lib.eg_last_error()
    assert call(full, c.P, F, c.Dpad, c.P + 1) == D.BAD_ARG and call(full, c.P, F, c.Dpad, 0) == D.BAD_ARG
    assert call(G.pointer_array(mem[:11] + [None], 12), c.P, F, c.Dpad, c.chunk) == D.BAD_ARG and b"partly set" in lib.eg_last_error()
    for o in outs:
        o.untouched("refused eg_prior_encoder")
