"""mel_power_kernel's register radix-4 transform (csrc/mel.hip) on the GPU.

1. The project's criterion (tests/small_ops_f64.py mel_criterion: at most one fp16 ulp, < 1 % of the bins differing, fp16-representable) against
   oracle.melspectrogram, every floor bin of the oracle exactly -80 dB, on the smallest inputs that reach every edge of the kernel: the lengths
   512 / 513 / 1023 / 1024 / 1535 (2 or 3 frames: 1024 and 1535 have an odd count, so the last pair's odd frame is empty), the two tones and
   the unit impulses of small_ops_f64 (impulses at 0 / 511 / 512 / 513 of a 2048-sample clip: five frames, the window zero and both frame seams),
   and silence, which is exactly 0 dB.  `oracle_reference` checks, on the CPU and before any launch, that the oracle alone is well-defined on
   each input: finite everywhere, and a non-empty set of floor bins for the tones.
2. Batch independence: three clips 40 dB apart in level; every row bit-equal to the clip alone.
3. The fp32 mel power of both transforms (default, and EG_MEL_FFT=2: the radix-2 kernel) against a float64 numpy evaluation built from the
   window and the filter table eg_mel_tables returns: the maximum relative error over the bins whose power is above 1e-6 of the clip maximum.
   The radix-4 figure must not exceed twice the radix-2 figure (a radix-4 transform has half the rounding stages; the factor is for a different
   rounding pattern, not for a less accurate transform).
4. An unknown EG_MEL_FFT value is refused with EG_ERR_BAD_ARG before any launch."""
import numpy as np
import pytest
import torch

import small_ops_f64 as S
from emotiongestures_amd.synth import synth_audio

pytestmark = pytest.mark.gpu

LENGTHS = tuple(n for n in S.MEL_LENGTHS if n <= 1535)          # 512, 513, 1023, 1024, 1535
IMPULSES = tuple(s for s in S.MEL_IMPULSES if s <= 513)         # 0, 511, 512, 513
TONE_SAMPLES = 2048
SENTINEL = -6.0e30


def _inputs():
    d = {f"len{n}": synth_audio(1, n, seed=n) for n in LENGTHS}
    t = np.arange(TONE_SAMPLES, dtype=np.float64) / 16000.0
    for hz in S.MEL_TONES_HZ:
        d[f"tone{hz:g}"] = (0.5 * np.sin(2.0 * np.pi * hz * t)).astype(np.float32)[None]
    imp = np.zeros((len(IMPULSES), 2048), np.float32)
    for i, s in enumerate(IMPULSES):
        imp[i, s] = 1.0
    d["impulses"] = imp
    d["silence"] = np.zeros((1, 1024), np.float32)
    return d


INPUTS = _inputs()
_ref = {}


def oracle_reference(name):
    """oracle.melspectrogram of the input, computed once; asserts that the oracle alone is well-defined on it."""
    if name not in _ref:
        from oracle import emogest_oracle as O
        ref = O.melspectrogram(INPUTS[name])
        assert np.isfinite(ref).all(), f"{name}: the oracle is not finite"
        if name.startswith("tone"):
            assert (ref == -80.0).any(), f"{name}: the oracle puts no bin at the floor"
        _ref[name] = ref
    return _ref[name]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_front = {}


def _mel():
    from emotiongestures_amd.engine import MelFrontEnd
    if "mel" not in _front:
        _front["mel"] = MelFrontEnd(dev())
    return _front["mel"]


def _call(audio):
    """eg_melspectrogram directly -> (status, spec [B, 128, frames], mel power workspace [B, 128, frames]); both pre-filled with a sentinel."""
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd.engine import _ptr, _stream
    lib, mel = L.load(), _mel()
    B, n = audio.shape
    frames = 1 + n // 512
    nbytes = int(lib.eg_mel_workspace_bytes(B, n))
    assert nbytes == B * 128 * frames * 4
    ws = torch.full((B, 128, frames), SENTINEL, device=dev())
    spec = torch.full((B, 128, frames), SENTINEL, device=dev())
    rc = lib.eg_melspectrogram(_ptr(audio), B, n, _ptr(mel.fb), _ptr(mel.win), _ptr(mel.tw), _ptr(mel.band), _ptr(spec), frames, _ptr(ws), nbytes,
                               _stream(dev()))
    torch.cuda.synchronize()
    return rc, spec, ws


def _spec(audio):
    from emotiongestures_amd import _lib as L
    rc, spec, _ = _call(audio)
    L.check(rc, "eg_melspectrogram")
    return spec


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_radix4_mel_meets_the_project_criterion(name, monkeypatch):
    monkeypatch.delenv("EG_MEL_FFT", raising=False)
    ref = oracle_reference(name)
    audio = INPUTS[name]
    got = _spec(torch.from_numpy(audio).to(dev())).cpu().numpy()
    diff = np.abs(got - ref)
    print(f"mel {name}: max |d| {diff.max():.4f} dB, {100 * float((diff > 0).mean()):.3f} % of bins differ, {100 * float((ref == -80).mean()):.1f} % at the floor")
    S.mel_criterion(got, ref, name)
    assert np.all(got[ref == -80.0] == -80.0), f"{name}: {int((got[ref == -80.0] != -80.0).sum())} floor bins are not at -80 dB"
    if name == "silence":
        assert np.all(got == 0.0)


def test_a_clip_is_bit_independent_of_its_batch(monkeypatch):
    monkeypatch.delenv("EG_MEL_FFT", raising=False)
    clip = S.hash_uniform("melfft.batch", (1, 2048), -1.0, 1.0, 0)
    audio = torch.from_numpy(np.concatenate([np.float32(s) * clip for s in (1.0, 1e-2, 1e-4)], 0)).to(dev())
    spec = _spec(audio)
    for i in range(3):
        assert torch.equal(_spec(audio[i:i + 1].contiguous())[0], spec[i]), f"clip {i} depends on the batch it travels in"


def _melpow_f64(audio):
    """The mel power [B, 128, frames] in float64 from the SAME fp32 window and filter table the kernels read."""
    mel = _mel()
    win = mel.win.cpu().numpy().astype(np.float64)
    fb_t = mel.fb.cpu().numpy().astype(np.float64).reshape(513, 128)
    B, n = audio.shape
    frames = 1 + n // 512
    padded = np.pad(audio.astype(np.float64), ((0, 0), (512, 512)))
    fr = np.stack([padded[:, 512 * f:512 * f + 1024] for f in range(frames)], 1) * win        # [B, frames, 1024]
    z = np.fft.rfft(fr, axis=-1)
    power = z.real ** 2 + z.imag ** 2
    return np.einsum("bfk,km->bmf", power, fb_t)


def _melpow_error(got, ref):
    worst = 0.0
    for b in range(ref.shape[0]):
        keep = ref[b] > 1e-6 * ref[b].max()
        worst = max(worst, float((np.abs(got[b] - ref[b])[keep] / ref[b][keep]).max()))
    return worst


def test_mel_power_is_no_less_accurate_than_the_radix2_kernel(monkeypatch):
    from emotiongestures_amd import _lib as L
    audio = synth_audio(2, 4096, seed=12)
    ref = _melpow_f64(audio)
    ad = torch.from_numpy(audio).to(dev())
    monkeypatch.delenv("EG_MEL_FFT", raising=False)
    rc4, spec4, pow4 = _call(ad)
    monkeypatch.setenv("EG_MEL_FFT", "2")
    rc2, spec2, pow2 = _call(ad)
    monkeypatch.setenv("EG_MEL_FFT", "4")
    rc4b, spec4b, pow4b = _call(ad)
    monkeypatch.delenv("EG_MEL_FFT")
    for rc in (rc4, rc2, rc4b):
        L.check(rc, "eg_melspectrogram")
    assert torch.equal(pow4, pow4b) and torch.equal(spec4, spec4b)          # "4" names the default
    e4, e2 = _melpow_error(pow4.cpu().numpy().astype(np.float64), ref), _melpow_error(pow2.cpu().numpy().astype(np.float64), ref)
    print(f"mel power, max relative error over bins above 1e-6 of the clip maximum: radix-4 {e4:.3e}, radix-2 {e2:.3e}")
    assert e4 <= 2.0 * e2, f"radix-4 {e4:.3e} against radix-2 {e2:.3e}"
    S.mel_criterion(spec4.cpu().numpy(), spec2.cpu().numpy(), "radix-4 against radix-2")


def test_unknown_switch_value_is_refused_before_any_launch(monkeypatch):
    from emotiongestures_amd import _lib as L
    lib = L.load()
    ad = torch.from_numpy(INPUTS["len1024"]).to(dev())
    _mel()
    before = lib.eg_launch_count()
    monkeypatch.setenv("EG_MEL_FFT", "7")
    rc, spec, ws = _call(ad)
    monkeypatch.delenv("EG_MEL_FFT")
    assert rc == -1 and b"EG_MEL_FFT" in lib.eg_last_error()
    assert lib.eg_launch_count() == before
    assert bool((spec == SENTINEL).all()) and bool((ws == SENTINEL).all())
