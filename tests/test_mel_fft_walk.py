"""The index arithmetic of mel_power_kernel's radix-4 transform, checked without a GPU: tools/mel_fft_walk.py restates which thread holds which
points in which pass, the exchange slots, the twiddle index per pass and the final order, in float64 numpy.  This checks the schedule as restated
there, not the kernel: what binds the kernel to it is tests/test_gpu_mel_fft.py (the oracle, and the float64 mel power)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mel_fft_walk", os.path.join(ROOT, "tools", "mel_fft_walk.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

TOL = 1e-12         # float64: five passes of O(1) roundings on a 1024-term sum, relative to the largest bin


@pytest.fixture(scope="module")
def walked():
    rng = np.random.default_rng(12)
    x = rng.standard_normal(W.N) + 1j * rng.standard_normal(W.N)
    got, slots = W.transform(x)
    return x, got, slots


def test_walk_equals_numpy_fft_in_natural_order(walked):
    x, got, _ = walked
    ref = np.fft.fft(x)
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= TOL * np.abs(ref).max()       # element for element: the final digit map is the identity


def test_two_real_frames_separate(walked):
    """Frame a as real and frame b as imaginary part: X_a[k] = (Z[k] + conj Z[N-k]) / 2, X_b[k] = (Z[k] - conj Z[N-k]) / 2i, through pair_bins()."""
    rng = np.random.default_rng(13)
    a, b = rng.standard_normal(W.N), rng.standard_normal(W.N)
    z, _ = W.transform(a + 1j * b)
    fa, fb = np.fft.rfft(a), np.fft.rfft(b)
    for _tid, k, nk in W.pair_bins():
        xa = 0.5 * (z[k] + np.conj(z[nk]))
        xb = -0.5j * (z[k] - np.conj(z[nk]))
        assert abs(xa - fa[k]) <= TOL * np.abs(fa).max() and abs(xb - fb[k]) <= TOL * np.abs(fb).max()


def test_every_pass_writes_a_permutation(walked):
    _, _, slots = walked
    assert len(slots) == W.PASSES
    for p, s in enumerate(slots):
        assert sorted(s) == list(range(W.N)), f"pass {p}: the exchange slots are not a permutation of 0..1023"


def test_every_pass_reads_a_permutation():
    elems = np.concatenate([W.read_elements(j) for j in range(W.THREADS)])
    assert sorted(elems.tolist()) == list(range(W.N))
    assert sorted(W.slot(elems).tolist()) == list(range(W.N))


def test_twiddle_indices_stay_inside_the_sign_extended_table():
    for p in range(W.PASSES):
        ns = 4 ** p
        ts = [W.twiddle_index(j, ns, r) for j in range(W.THREADS) for r in range(4)]
        assert min(ts) >= 0 and max(ts) < 1024 and (p > 0 or max(ts) == 0)
        assert max(W.twiddle_index(j, ns, r) for j in range(W.THREADS) for r in range(3)) < 512      # only r = 3 needs the sign


def test_pairing_reaches_every_bin_once():
    pairs = W.pair_bins()
    ks = [k for _t, k, _nk in pairs]
    assert sorted(ks) == list(range(513))
    assert all(nk == (W.N - k) % W.N for _t, k, nk in pairs)
    per_thread = {}
    for t, _k, _nk in pairs:
        per_thread[t] = per_thread.get(t, 0) + 1
    assert per_thread[0] == 3 and all(per_thread[t] == 2 for t in range(1, W.THREADS))


def test_exchange_is_bank_conflict_free_as_the_kernel_comment_states():
    assert [W.write_bank_conflicts(4 ** p) for p in range(W.PASSES)] == [1] * W.PASSES
    assert W.read_bank_conflicts() == 1


def test_twiddle_table_copy_reads_are_conflict_free_in_passes_4_and_16_and_at_most_four_way_after():
    slots = [W.tw_slot(t) for t in range(512)]
    assert len(set(slots)) == 512 and max(slots) < 1024          # injective, inside the 1024-slot buffer it borrows
    assert [W.twiddle_read_conflicts(4 ** p) for p in range(1, W.PASSES)] == [1, 1, 4, 3]      # unpadded: [4, 16, 8, 3]
