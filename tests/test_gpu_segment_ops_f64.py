"""eg_seg_mean / eg_seg_dot / eg_se_scale and the gradient-bucket payload conversion eg_f32_to_bf16 / eg_bf16_to_f32 on the GPU through the C ABI
(tests/train_tail_f64.py sections 7 and 8).  The segment reductions are held per ELEMENT on their three routes: one kernel (workspace NULL, or
batch > 512), the segmented fast path (C | 1024, more than one segment) and one generic launch per segment.  The conversion is BITWISE torch's cast on
every finite value and +-inf; a NaN must come back a NaN -- f32_to_bf16_rne once had no NaN case (0x7FFFFFFF -> -0, 0xFFFFFFFF -> +0,
0x7F800001 -> +inf), so a NaN gradient could leave the bf16 bucket payload of train/optim.py as a zero."""
import numpy as np
import pytest
import torch

import train_tail_f64 as S
import train_tail_gpu as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", S.SEG_CASES, ids=lambda k: f"{k.batch}x{k.hw}x{k.c}-{k.route}")
def test_segment_ops_match_float64_per_element(case):
    L, lib, ptr, st = D.api()
    B, HW, C = case.batch, case.hw, case.c
    plan = S.seg_plan(case)
    assert plan.route == case.route
    x, dy, gate, add = S.seg_inputs(case)
    xd, dyd, gd, ad = D.up(x), D.up(dy), D.up(gate), D.up(add)
    scale = 1.0 / HW
    ref, bound = S.seg_eval(x, dy, gate, add, scale), S.seg_bounds(x, dy, gate, add, scale, plan)
    what = f"segment ops {B}x{HW}x{C} ({case.route})"
    ws = D.workspace(int(lib.eg_colreduce_workspace_floats(C))) if case.ws else None
    mean, dot = D.Guarded((B, C)), D.Guarded((B, C))
    L.check(lib.eg_seg_mean(ptr(xd), ptr(mean.t), B, HW, C, scale, ptr(ws.t) if ws else None, st), what + " seg_mean")
    L.check(lib.eg_seg_dot(ptr(dyd), ptr(xd), ptr(dot.t), B, HW, C, ptr(ws.t) if ws else None, st), what + " seg_dot")
    if ws:
        ws.intact(what + " workspace")
    D.frac("seg_mean", mean.intact(what + " seg_mean"), ref[0], bound[0], what + " seg_mean", S.SEG_AXES)
    D.frac("seg_dot", dot.intact(what + " seg_dot"), ref[1], bound[1], what + " seg_dot", S.SEG_AXES)
    for i, a in ((2, None), (3, ad)):
        y = D.Guarded((B, HW, C))
        L.check(lib.eg_se_scale(ptr(dyd), ptr(gd), ptr(a), ptr(y.t), B, HW, C, st), what + " se_scale")
        D.frac("se_scale", y.intact(what + " se_scale"), ref[i], bound[i], what + f" se_scale add {a is not None}", ("clip", "pixel", "channel"))
    D.report("seg_mean", "seg_dot", "se_scale")


def _to_bf16(x32):
    L, lib, ptr, st = D.api()
    n = x32.numel()
    out, xd = D.Guarded((cdiv2(n),)), D.up(x32)     # n uint16 slots in ceil(n / 2) 4-byte slots
    L.check(lib.eg_f32_to_bf16(ptr(xd), ptr(out.t), n, st), "eg_f32_to_bf16")
    got = out.intact("eg_f32_to_bf16").view(torch.int16)
    if n % 2:           # the upper half of the last 4-byte slot still holds the canary (little endian)
        assert int(got[n]) & 0xFFFF == D.SENTINEL >> 16, "eg_f32_to_bf16: a store behind the last element"
    return got[:n].numpy().view(np.uint16)


def cdiv2(n):
    return (n + 1) // 2


def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


@pytest.mark.parametrize("n", S.BF16_N)
def test_f32_to_bf16_is_torchs_cast_bitwise(n):
    """Every finite pattern of bf16_finite_bits (ties to even in both directions, the largest finite float -> inf, denormals, +-0) and +-inf, cycled
    through n = 1, 255, 257 elements at every starting point of the list."""
    bits = S.bf16_finite_bits()
    for start in range(0, len(bits), n):
        chunk = _cycle(bits[start:] + bits[:start], n)
        x = S.bits_to_f32(chunk)
        want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        got = _to_bf16(x)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"n {n}: 0x{chunk[bad[0]]:08X} -> 0x{got[bad[0]]:04X}, torch 0x{want[bad[0]]:04X} ({bad.size} elements)"


@pytest.mark.parametrize("n", S.BF16_N)
def test_f32_to_bf16_keeps_nan(n):
    """NaN must come back as NaN (any payload or sign).  Without the NaN case of f32_to_bf16_rne, 0x7FFFFFFF becomes -0, 0xFFFFFFFF +0 and
    0x7F800001 +inf."""
    chunk = _cycle(list(S.BF16_NAN_BITS), n)
    got = _to_bf16(S.bits_to_f32(chunk))
    bad = np.nonzero(~S.is_bf16_nan(got))[0]
    assert bad.size == 0, f"n {n}: NaN 0x{chunk[bad[0]]:08X} -> 0x{got[bad[0]]:04X}"
    assert np.array_equal(got, S.bf16_rne_bits(chunk))


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", S.BF16_N)
def test_bf16_to_f32_is_torchs_cast_bitwise(n, scale):
    """bf16 -> fp32 x scale, bitwise torch's (cast, then one fp32 product): every pattern above after its rounding to bf16, and NaN stays NaN."""
    L, lib, ptr, st = D.api()
    h = S.bf16_rne_bits(S.bf16_finite_bits() + list(S.BF16_NAN_BITS)).astype(np.int16)
    for start in range(0, len(h), n):
        chunk = torch.from_numpy(np.resize(np.roll(h, -start), n).copy())
        want = chunk.view(torch.bfloat16).float() * scale
        out, hd = D.Guarded((n,)), D.up(chunk)
        L.check(lib.eg_bf16_to_f32(ptr(hd), ptr(out.t), n, scale, st), "eg_bf16_to_f32")
        got = out.intact("eg_bf16_to_f32")
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), f"n {n} scale {scale}: NaN positions differ"
        bad = (got.view(torch.int32) != want.view(torch.int32)) & ~nan
        assert not bool(bad.any()), f"n {n} scale {scale}: 0x{int(chunk[bad.nonzero()[0, 0]]) & 0xFFFF:04X} differs ({int(bad.sum())} elements)"
