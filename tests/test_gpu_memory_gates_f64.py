"""The two memory nets of the prior encoder on the GPU -- eg_sp_gate_forward / _backward and eg_tm_scale_forward / _backward of csrc/train.hip --
through the C ABI, every ELEMENT against float64 (tests/train_tail_f64.py section 5).  The backward entry points take the forward's gate / weights
as an argument; they are given the fp32 rounding of the float64 ones and the reference uses those, so each kernel is held on its own.  Outputs sit
in canary-guarded buffers."""
import pytest
import torch

import train_tail_f64 as S
import train_tail_gpu as D

pytestmark = pytest.mark.gpu
_ID = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("saturate", [False, True], ids=["plain", "saturated"])
@pytest.mark.parametrize("shape", S.GATE_SHAPES, ids=_ID)
def test_spatial_gate_matches_float64_per_element(shape, saturate):
    """sp_gate_fwd_kernel / sp_gate_bwd_kernel: out, gate, dpred, dmem.  Pass-through frames (c >= chunk) are bitwise copies; with |<m, p>| > 100
    the gate is exactly 0 or 1 and nothing is NaN; chunk = 0 writes no gate and a zero dmem."""
    L, lib, ptr, st = D.api()
    B, P, Dm, chunk = shape
    m, p, g, _ = S.gate_inputs(B, P, Dm, chunk, saturate)
    md, pd, gd = D.up(m), D.up(p), D.up(g)
    what = f"sp_gate {shape} saturated {saturate}"
    out, gate = D.Guarded((B, P, Dm)), D.Guarded((B, max(chunk, 1)))          # (chunk = 0: the entry point still wants a pointer; nothing is written)
    L.check(lib.eg_sp_gate_forward(ptr(md), ptr(pd), ptr(out.t), ptr(gate.t), B, P, Dm, chunk, st), what)
    o, s = out.intact(what + " out"), gate.intact(what + " gate")[:, :chunk]
    if chunk == 0:
        gate.untouched(what + " gate")
    (ro, rs), (bo, bs) = S.sp_eval(m, p, chunk), S.sp_bounds(m, p, chunk)
    D.frac("sp_gate out", o, ro, bo, what + " out", S.GATE_AXES)
    D.frac("sp_gate gate", s, rs, bs, what + " gate", ("clip", "frame"))
    assert torch.equal(o[:, chunk:].view(torch.int32), p[:, chunk:].view(torch.int32)), what + ": pass-through frames are not bitwise copies"
    if saturate and chunk:
        assert set(s.unique().tolist()) <= {0.0, 1.0} and len(s.unique()) == min(2, chunk), what + ": the gate did not saturate to exactly 0 and 1"
    gate32 = rs.float()
    gated = D.up(gate32) if chunk else gate.t
    dp, dm = D.Guarded((B, P, Dm)), D.Guarded((B, Dm))
    L.check(lib.eg_sp_gate_backward(ptr(md), ptr(pd), ptr(gated), ptr(gd), ptr(dp.t), ptr(dm.t), B, P, Dm, chunk, st), what)
    gdp, gdm = dp.intact(what + " dpred"), dm.intact(what + " dmem")
    (rdp, rdm), (bdp, bdm) = S.sp_bwd_eval(m, p, gate32, g, chunk), S.sp_bwd_bounds(m, p, gate32, g, chunk)
    D.frac("sp_gate dpred", gdp, rdp, bdp, what + " dpred", S.GATE_AXES)
    D.frac("sp_gate dmem", gdm, rdm, bdm, what + " dmem", ("clip", "dim"))
    assert torch.equal(gdp[:, chunk:].view(torch.int32), g[:, chunk:].view(torch.int32)), what + ": pass-through gradients are not bitwise copies"
    if chunk == 0:
        assert bool((gdm == 0).all())
    D.report("sp_gate out", "sp_gate gate", "sp_gate dpred", "sp_gate dmem")


@pytest.mark.parametrize("shape", S.TM_SHAPES, ids=_ID)
def test_temporal_scale_matches_float64_per_element(shape):
    """tm_scale_fwd_kernel / tm_scale_bwd_kernel with scores in +-50: out, w, dpred, dscore; sum_c dscore = 0 within the sum of its bounds."""
    L, lib, ptr, st = D.api()
    B, P, Dm, chunk = shape
    m, p, g, score = S.gate_inputs(B, P, Dm, chunk)
    pd, gd, sd = D.up(p), D.up(g), D.up(score)
    what = f"tm_scale {shape}"
    out, w = D.Guarded((B, P, Dm)), D.Guarded((B, chunk))
    L.check(lib.eg_tm_scale_forward(ptr(sd), ptr(pd), ptr(out.t), ptr(w.t), B, P, Dm, chunk, st), what)
    o, gw = out.intact(what + " out"), w.intact(what + " w")
    (ro, rw), (bo, bw) = S.tm_eval(score, p, chunk), S.tm_bounds(score, p, chunk)
    D.frac("tm_scale out", o, ro, bo, what + " out", S.GATE_AXES)
    D.frac("tm_scale w", gw, rw, bw, what + " w", ("clip", "frame"))
    assert torch.equal(o[:, chunk:].view(torch.int32), p[:, chunk:].view(torch.int32)), what + ": pass-through frames are not bitwise copies"
    w32 = rw.float()
    wd = D.up(w32)
    dp, ds = D.Guarded((B, P, Dm)), D.Guarded((B, chunk))
    L.check(lib.eg_tm_scale_backward(ptr(wd), ptr(pd), ptr(gd), ptr(dp.t), ptr(ds.t), B, P, Dm, chunk, st), what)
    gdp, gds = dp.intact(what + " dpred"), ds.intact(what + " dscore")
    (rdp, rds), (bdp, bds) = S.tm_bwd_eval(w32, p, g, chunk), S.tm_bwd_bounds(w32, p, g, chunk)
    D.frac("tm_scale dpred", gdp, rdp, bdp, what + " dpred", S.GATE_AXES)
    D.frac("tm_scale dscore", gds, rds, bds, what + " dscore", ("clip", "frame"))
    assert bool((gds.double().sum(1).abs() <= bds.sum(1) + rds.sum(1).abs()).all()), what + ": sum_c dscore is not 0 within its bound"
    D.report("tm_scale out", "tm_scale w", "tm_scale dpred", "tm_scale dscore")


def test_temporal_scale_refuses_chunk_65():
    L, lib, ptr, st = D.api()
    B, P, Dm = 1, 70, 4
    p, s = D.up(torch.ones(B, P, Dm)), D.up(torch.zeros(B, 65))
    out, w, ds = D.Guarded((B, P, Dm)), D.Guarded((B, 65)), D.Guarded((B, 65))
    assert lib.eg_tm_scale_forward(ptr(s), ptr(p), ptr(out.t), ptr(w.t), B, P, Dm, 65, st) == D.BAD_ARG
    assert lib.eg_tm_scale_backward(ptr(s), ptr(p), ptr(p), ptr(out.t), ptr(ds.t), B, P, Dm, 65, st) == D.BAD_ARG
    for o in (out, w, ds):
        o.untouched("tm_scale chunk 65")
    assert lib.eg_tm_scale_forward(ptr(s), ptr(p), ptr(out.t), ptr(w.t), B, P, Dm, 64, st) == 0
