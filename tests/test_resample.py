"""Polyphase resampler, CPU side: the plan table and the fp32 filter from the library's host entries, the float64 restatement against
scipy.signal.resample_poly, the chunked form against the delayed offline one, and the refusals by name.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import resample_np as R
from conftest import build_mirror
from emotiongestures_amd import _lib as L
from emotiongestures_amd import resample as RS

NEW_SYMBOLS = ("eg_resample_plan", "eg_resample_out_length", "eg_resample_filter", "eg_resample", "eg_resample_stream_state_bytes",
               "eg_resample_stream_reset", "eg_resample_stream_push")


@pytest.mark.parametrize("rate", R.RATES)
def test_plan_table_value_for_value(rate):
    p = RS.plan(rate)
    assert (p["L"], p["M"], p["half"], p["K"], p["D"], p["Hs"]) == R.PLAN_TABLE[rate]
    assert {k: p[k] for k in ("L", "M", "half", "K", "D", "Hs")} == R.plan_np(rate)
    assert p["pitch"] % 2 == 1 and p["pitch"] >= p["K"] and p["bank_floats"] == p["L"] * p["pitch"]
    assert RS.ratio(rate) == (p["L"], p["M"]) and RS.stream_delay(rate) == p["D"]
    for n in (0, 1, 2, 777, 1001):
        assert RS.out_length(n, rate) == R.out_length_np(n, rate) == L.load().eg_resample_out_length(n, rate, 16000)


def test_every_rate_the_header_lists_is_supported():
    for rate in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        Lf, M = RS.ratio(rate)
        assert max(Lf, M) <= RS.MAX_FACTOR == 640 and Lf * rate == M * 16000


@pytest.mark.parametrize("rate", R.RATES)
def test_fp32_filter_is_firwin_times_L_within_one_rounding(rate):
    from scipy.signal import firwin
    p = RS.plan(rate)
    ref = firwin(2 * p["half"] + 1, 1.0 / max(p["L"], p["M"]), window=("kaiser", 5.0)) * p["L"]
    h = RS.filter_taps(rate)
    assert h.dtype == np.float32 and h.shape == ref.shape
    assert np.abs(h.astype(np.float64) - ref).max() <= 6e-8
    assert np.abs(R.filter_np(rate) - ref).max() <= 1e-14
    # every tap, the near-zero ones at the sinc's zero crossings included, is one fp32 rounding of the definition's own float64 value
    # (np.sinc / np.kaiser): the element-wise bound of the GPU tests is relative to sum |x||h|, which one such tap alone can make up
    ref64 = R.filter_np(rate)
    assert (np.abs(h.astype(np.float64) - ref64) <= 2.0 ** -24 * np.abs(ref64)).all()
    # the bank holds the same taps: bank[phase][j] = h[phase + j*L], zero elsewhere
    bank = np.full(p["bank_floats"], np.nan, np.float32)
    L.check(L.load().eg_resample_filter(rate, 16000, None, C.c_void_p(bank.ctypes.data)), "eg_resample_filter")
    bank = bank.reshape(p["L"], p["pitch"])
    want = np.zeros_like(bank)
    for ph in range(p["L"]):
        taps = h[ph::p["L"]]
        want[ph, :len(taps)] = taps
    assert np.array_equal(bank, want)


@pytest.mark.parametrize("rate", R.RATES)
def test_restatement_equals_scipy_resample_poly(rate):
    from scipy.signal import resample_poly
    rng = np.random.default_rng(rate)
    p = R.plan_np(rate)
    for n in (1, 2, 777, 1000, 1001, 1999):
        x = rng.standard_normal(n)
        y, S = R.resample_np(x, rate)
        ref = resample_poly(x, p["L"], p["M"])
        assert y.shape == ref.shape == (R.out_length_np(n, rate),)
        assert np.abs(y - ref).max() <= 1e-12, (rate, n, np.abs(y - ref).max())
        assert (S >= np.abs(y) - 1e-12).all()


@pytest.mark.parametrize("rate", [48000, 44100, 24000, 22050, 8000])
def test_chunked_equals_delayed_offline(rate):
    p = R.plan_np(rate)
    hop = 640
    st = R.StreamNp(rate, hop)
    rng = np.random.default_rng(rate + 1)
    n_in = 3 * st.hop_in + st.hop_in // 3 + 1                   # ends inside the fourth push
    x = rng.standard_normal(n_in)
    ref, _S = R.resample_np(x, rate, delay=p["D"])
    got = []
    for c in range(4):
        chunk = np.full(st.hop_in, np.nan)
        seg = x[c * st.hop_in:(c + 1) * st.hop_in]
        chunk[:len(seg)] = seg
        got.append(st.push(chunk, end=-1 if c < 3 else len(seg)))
    got = np.concatenate(got)
    assert np.abs(got[:len(ref)] - ref).max() <= 1e-12
    assert not got[len(ref):].any() and len(ref) == R.out_length_np(n_in, rate)


def test_rates_refused_by_name():
    for bad in (0, -16000):
        with pytest.raises(L.EgError, match=re.escape(f"rate_in={bad}")):
            RS.plan(bad)
    with pytest.raises(L.EgError, match=re.escape("rate_out=0")):
        RS.ratio(48000, 0)
    with pytest.raises(L.EgError, match=r"L=16000 / M=44101.*max\(L, M\) <= 640"):
        RS.plan(44101)
    lib = L.load()
    p = L.EgResamplePlan()
    assert lib.eg_resample_plan(0, 16000, C.byref(p)) != 0 and "rate_in=0" in lib.eg_last_error().decode()
    assert lib.eg_resample_plan(48000, 16000, None) != 0 and "null plan" in lib.eg_last_error().decode()
    assert lib.eg_resample_out_length(5, 44101, 16000) == -1 and lib.eg_resample_out_length(-1, 48000, 16000) == -1
    assert lib.eg_resample_stream_state_bytes(0, 48000, 16000) == 0 and lib.eg_resample_stream_state_bytes(2, 44101, 16000) == 0
    assert lib.eg_resample_stream_state_bytes(3, 48000, 16000) >= 3 * 60 * 4
    assert lib.eg_resample_filter(48000, 16000, None, None) != 0 and "null h_taps and null h_bank" in lib.eg_last_error().decode()


def test_python_surface_refusals():
    with pytest.raises(L.EgError, match="audio must be a CUDA tensor"):
        RS.resample_audio(torch.zeros(2, 480), 48000)
    with pytest.raises(L.EgError, match="L=16000"):
        RS.resample_audio(torch.zeros(2, 480), 44101)
    with pytest.raises(L.EgError, match=re.escape("hop_in=30 < Hs=60")):
        RS.StreamResampler(2, 48000, 10)
    with pytest.raises(L.EgError, match="must be a multiple of 160"):
        RS.StreamResampler(2, 44100, 59733)
    with pytest.raises(L.EgError, match="CUDA device"):
        RS.StreamResampler(2, 48000, 640, device="cpu")


def test_gesture_stream_refuses_a_fractional_input_hop_by_name():
    from emotiongestures_amd.streaming import AUTO_MEL, GestureStream
    gen = build_mirror("spatial", 34, 126, 4, 4, seed=3).eval()
    seed = torch.zeros(2, 4, 126)
    with pytest.raises(L.EgError, match=r"hop_samples=59733 at audio_rate=44100.*multiple of 160 \(nearest: 59680 or 59840\)"):
        GestureStream((gen, None, AUTO_MEL), 2, seed, hop_samples=59733, n_samples=64000, audio_rate=44100)
    with pytest.raises(L.EgError, match="audio_rate.*no mel front-end"):
        GestureStream((gen, None, None), 2, seed, audio_rate=48000)


def _offline(lib, **over):
    """eg_resample with dummy non-null pointers: every refusal comes before the launch, so nothing is dereferenced."""
    lens = over.pop("lengths", [480, 100])
    keep = None if lens is None else np.ascontiguousarray(lens, np.int64)
    dummy = C.c_void_p(256)
    a = dict(x=dummy, U=2, in_stride=480, lengths=None if keep is None else C.c_void_p(keep.ctypes.data), d_lengths=dummy, rate_in=48000,
             rate_out=16000, d_bank=dummy, delay=0, y=dummy, out_stride=160, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    rc = lib.eg_resample(*a.values())
    return rc, lib.eg_last_error().decode()


def _push(lib, **over):
    dummy = C.c_void_p(256)
    a = dict(state=dummy, rows=2, rate_in=48000, rate_out=16000, d_bank=dummy, chunk=dummy, hop_in=1920, ends=dummy, out=dummy, hop_out=640,
             stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    rc = lib.eg_resample_stream_push(*a.values())
    return rc, lib.eg_last_error().decode()


OFFLINE_REFUSALS = [
    (dict(x=None), "null x"), (dict(lengths=None), "null lengths"), (dict(d_lengths=None), "null d_lengths"), (dict(d_bank=None), "null d_bank"),
    (dict(y=None), "null y"), (dict(y=C.c_void_p(260)), "not 16-byte aligned"),
    (dict(rate_in=0), "rate_in=0"), (dict(rate_in=44101), "L=16000 / M=44101"),
    (dict(U=0), "U=0"), (dict(U=65536), "U=65536"),
    (dict(lengths=[480, 0]), "lengths[1]=0"), (dict(lengths=[481, 5]), "lengths[0]=481 (1..in_stride=480)"),
    (dict(out_stride=159), "out_stride=159 < 160"), (dict(delay=-1), "delay=-1"),
]
PUSH_REFUSALS = [
    (dict(state=None), "null state"), (dict(d_bank=None), "null d_bank"), (dict(chunk=None), "null chunk_in"), (dict(out=None), "null out"),
    (dict(rows=0), "rows=0"), (dict(rate_in=-5), "rate_in=-5"), (dict(rate_in=44101), "L=16000"),
    (dict(hop_in=1919), "hop_in=1919 is not hop_out * M / L"), (dict(hop_in=30, hop_out=10), "hop_in=30 < Hs=60"),
    (dict(hop_in=0, hop_out=0), "hop_in=0"),
]


@pytest.mark.parametrize("over,needle", OFFLINE_REFUSALS, ids=[f"{list(o)[0]}-{n}" for o, n in OFFLINE_REFUSALS])
def test_offline_entry_refuses_by_name_before_any_device_use(over, needle):
    lib = L.load()
    before = lib.eg_launch_count()
    rc, msg = _offline(lib, **over)
    assert rc != 0 and "eg_resample" in msg and needle in msg, (rc, msg)
    assert lib.eg_launch_count() == before


@pytest.mark.parametrize("over,needle", PUSH_REFUSALS, ids=[f"{list(o)[0]}-{n}" for o, n in PUSH_REFUSALS])
def test_push_entry_refuses_by_name_before_any_device_use(over, needle):
    lib = L.load()
    before = lib.eg_launch_count()
    rc, msg = _push(lib, **over)
    assert rc != 0 and "eg_resample_stream_push" in msg and needle in msg, (rc, msg)
    assert lib.eg_launch_count() == before


def test_reset_entry_refusals_and_symbols():
    import os
    from conftest import ROOT
    lib = L.load()
    assert lib.eg_resample_stream_reset(None, 2, 48000, 16000, None, None) != 0 and "null state" in lib.eg_last_error().decode()
    assert lib.eg_resample_stream_reset(C.c_void_p(256), 0, 48000, 16000, None, None) != 0 and "rows=0" in lib.eg_last_error().decode()
    header = open(os.path.join(ROOT, "include", "emogest.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"#define EG_RESAMPLE_TILE %d\b" % RS.TILE, header)
    assert re.search(r"#define EG_RESAMPLE_MAX_FACTOR %d\b" % RS.MAX_FACTOR, header)
