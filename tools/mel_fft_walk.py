"""The pass structure of mel_power_kernel's transform (csrc/mel.hip), restated in numpy without a GPU: which thread holds which points in
which pass, where each point goes in the LDS exchange, which table entry each twiddle is, and the order the spectrum comes out in.

1024-point complex radix-4 Stockham transform, 256 threads, four points per thread, five passes p = 0..4 with NS = 4**p:

    thread j reads elements  j + 256 r                      (r = 0..3; pass 0 reads them from the windowed frames themselves)
    k = j mod NS;  v[r] *= exp(-2 pi i r k (256 / NS) / 1024)  (table index t = r k 256 / NS; t >= 512 is -table[t - 512])
    y = DFT4(v)
    thread j writes elements 4 (j - k) + k + r NS            (into the other LDS buffer, slot(i) = i ^ (5 * ((i >> 4) & 3)))

The table entries come from the workgroup's LDS copy, entry t in slot t + (t >> 4).

After pass 4 the buffer holds the spectrum in natural order (digit map = identity).  The power step then pairs bin k with bin (1024 - k) mod
1024 for k = tid, tid + 256 (and 512 on thread 0) to separate the two real frames carried as real and imaginary part.

tests/test_mel_fft_walk.py checks this restatement against numpy.fft.fft; tests/test_gpu_mel_fft.py binds the kernel to the oracle."""
import numpy as np

N, THREADS, PASSES = 1024, 256, 5


def slot(i):
    """LDS float2 slot of complex element i (bits 4..5 XORed into bits 0..1 and 2..3)."""
    i = np.asarray(i)
    return i ^ (5 * ((i >> 4) & 3))


def read_elements(j):
    """Elements thread j holds at the start of every pass."""
    return np.array([j + 256 * r for r in range(4)])


def write_elements(j, ns):
    k = j % ns
    return np.array([4 * (j - k) + k + r * ns for r in range(4)])


def twiddle_index(j, ns, r):
    """Index t of exp(-2 pi i t / 1024) applied to point r of thread j in the pass with sub-transform length ns."""
    return r * (j % ns) * (256 // ns)


def table(dtype=np.complex128):
    """d_twiddle: exp(-2 pi i t / 1024), t = 0..511."""
    t = np.arange(N // 2)
    return np.exp(-2j * np.pi * t / N).astype(dtype)


def twiddle(tab, t):
    return tab[t] if t < 512 else -tab[t - 512]


def tw_slot(t):
    """LDS float2 slot of table entry t in the workgroup's copy of the twiddle table (one pad per 16 entries)."""
    return t + (t >> 4)


def twiddle_read_conflicts(ns):
    """Worst number of distinct slots of one 32-lane group of a twiddle read of the pass that fall on the same bank pair (8-byte reads, 64 banks)."""
    worst = 0
    for g in range(THREADS // 32):
        for r in range(1, 4):
            s = {tw_slot(twiddle_index(j, ns, r) & 511) for j in range(32 * g, 32 * g + 32)}       # identical addresses broadcast
            banks = [v % 32 for v in s]
            worst = max(worst, max(banks.count(v) for v in set(banks)))
    return worst


def dft4(v):
    a0, a1, a2 = v[0] + v[2], v[0] - v[2], v[1] + v[3]
    d = v[1] - v[3]
    a3 = complex(d.imag, -d.real)          # -i (v1 - v3)
    return np.array([a0 + a2, a1 + a3, a0 - a2, a1 - a3])


def transform(x):
    """x [1024] complex -> (spectrum as the final LDS buffer holds it, read back through slot(); the write-slot lists of every pass)."""
    tab = table()
    buf = np.asarray(x, np.complex128)      # pass 0 reads the inputs, unswizzled, from registers
    swizzled = False
    slots_per_pass = []
    for p in range(PASSES):
        ns = 4 ** p
        out = np.full(N, np.nan + 0j)
        slots = []
        for j in range(THREADS):
            src = read_elements(j)
            v = buf[slot(src)] if swizzled else buf[src]
            v = np.array([v[r] * twiddle(tab, twiddle_index(j, ns, r)) for r in range(4)])
            dst = slot(write_elements(j, ns))
            out[dst] = dft4(v)
            slots.extend(dst.tolist())
        slots_per_pass.append(slots)
        buf, swizzled = out, True
    return buf[slot(np.arange(N))], slots_per_pass


def pair_bins():
    """-> [(thread, k, nk)] of the power step."""
    pairs = []
    for tid in range(THREADS):
        for u in range(3):
            if u < 2 or tid == 0:
                k = tid + 256 * u if u < 2 else 512
                pairs.append((tid, k, (N - k) & (N - 1)))
    return pairs


def write_bank_conflicts(ns):
    """Worst number of distinct slots of one 16-lane write group that fall on the same pair of 4-byte banks (8-byte stores, 32 banks)."""
    worst = 0
    for g in range(THREADS // 16):
        for r in range(4):
            s = [int(slot(write_elements(j, ns)[r])) % 16 for j in range(16 * g, 16 * g + 16)]
            worst = max(worst, max(s.count(v) for v in set(s)))
    return worst


def read_bank_conflicts():
    """The same for the 32-lane groups of the 8-byte reads (64 banks)."""
    worst = 0
    for g in range(THREADS // 32):
        for r in range(4):
            s = [int(slot(read_elements(j)[r])) % 32 for j in range(32 * g, 32 * g + 32)]
            worst = max(worst, max(s.count(v) for v in set(s)))
    return worst


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    got, _ = transform(x)
    ref = np.fft.fft(x)
    print("max relative error vs numpy.fft.fft:", np.abs(got - ref).max() / np.abs(ref).max())
    print("twiddle read conflicts per pass:", [twiddle_read_conflicts(4 ** p) for p in range(1, PASSES)])
    print("write conflicts per pass:", [write_bank_conflicts(4 ** p) for p in range(PASSES)], " read conflicts:", read_bank_conflicts())
