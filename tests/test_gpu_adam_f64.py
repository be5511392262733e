"""eg_adam_step and eg_adam_step_dev on the GPU through the C ABI: one step from given (p, g, m, v) against float64 with the fp32 hyper-parameters
the ABI receives, p, m and v per ELEMENT (tests/train_tail_f64.py section 6).  The slices sit in canary-guarded buffers at every 16-byte phase:
the float4 kernel updates the head / tail elements inside its one launch, a gradient on another phase forces the scalar kernel (adam_plan restates
the choice).  The bitwise float4-vs-scalar comparison stays in tests/test_gpu_training.py."""
import pytest
import torch

import train_tail_f64 as S
import train_tail_gpu as D

pytestmark = pytest.mark.gpu
H = S.ADAM_HYPER


def _step(p, g, m, v, t, wd, phase, grad_phase, dev_count, what):
    L, lib, ptr, st = D.api()
    n = p.numel()
    gp, gm, gv = D.Guarded((n,), phase, p), D.Guarded((n,), phase, m), D.Guarded((n,), phase, v)
    gd = D.up(g, grad_phase)
    if dev_count:
        step = torch.tensor([t], dtype=torch.int32, device=D.dev())
        rc = lib.eg_adam_step_dev(ptr(gp.t), ptr(gd), ptr(gm.t), ptr(gv.t), n, H["lr"], H["b1"], H["b2"], H["eps"], wd, ptr(step), st)
    else:
        rc = lib.eg_adam_step(ptr(gp.t), ptr(gd), ptr(gm.t), ptr(gv.t), n, H["lr"], H["b1"], H["b2"], H["eps"], wd, t, st)
    L.check(rc, what)
    return gp.intact(what + " p"), gm.intact(what + " m"), gv.intact(what + " v")


def _hold(out, p, g, m, v, t, wd, what):
    ref, bound = S.adam_eval(p, g, m, v, t, wd), S.adam_bounds(p, g, m, v, t, wd)
    for k, o, r, bd in zip("pmv", out, ref, bound):
        D.frac("adam " + k, o, r, bd, f"{what} {k}", ("element",))


@pytest.mark.parametrize("dev_count", [False, True], ids=["host_step", "device_step"])
@pytest.mark.parametrize("n", S.ADAM_N)
def test_adam_step_matches_float64_per_element(n, dev_count):
    """t = 1, 2, 1000, 100000; weight decay 0 and 1e-5; gradients over six decades, g = m = v = 0 with wd = 0 (p bitwise unchanged) and
    sqrt(v) << eps; n on both sides of the float4 threshold (8), with a tail (1027) and two workgroups (4103)."""
    assert S.adam_plan(n).route == ("scalar" if n < 8 else "float4")
    for cls in S.ADAM_CLASSES:
        p, g, m, v = S.adam_inputs(n, cls)
        for t in S.ADAM_T:
            for wd in ((0.0,) if cls == "zero" else S.ADAM_WD):
                what = f"adam n {n} {cls} t {t} wd {wd} dev {dev_count}"
                out = _step(p, g, m, v, t, wd, 0, 0, dev_count, what)
                _hold(out, p, g, m, v, t, wd, what)
                if cls == "zero":
                    assert torch.equal(out[0].view(torch.int32), p.view(torch.int32)), what + ": p changed although g = m = v = 0"
    D.report("adam p", "adam m", "adam v")


@pytest.mark.parametrize("dev_count", [False, True], ids=["host_step", "device_step"])
@pytest.mark.parametrize("n", [9, 1027, 4103])
def test_adam_every_slice_phase_matches_float64_per_element(n, dev_count):
    """Slice offsets 0..3 floats (float4 kernel: head = (4 - phase) % 4 elements in front of the first 16-byte boundary, the rest behind the
    last float4) and the gradient on another phase (scalar kernel): the elements at both ends of the slice are held like every other, and the
    canaries on both sides stay."""
    p, g, m, v = S.adam_inputs(n, "decades")
    for phase in range(4):
        for grad_phase in (phase, (phase + 2) % 4):
            plan = S.adam_plan(n, phase, grad_phase)
            assert plan.route == ("float4" if grad_phase == phase else "scalar")
            what = f"adam n {n} phase {phase} grad phase {grad_phase} ({plan.route}: head {plan.head}, tail {plan.tail}) dev {dev_count}"
            _hold(_step(p, g, m, v, 2, 1e-5, phase, grad_phase, dev_count, what), p, g, m, v, 2, 1e-5, what)
    D.report("adam p", "adam m", "adam v")
