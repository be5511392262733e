// Device code shared by the two beat-alignment paths: the clip call (mel.hip: eg_beat_align) and the whole-recording call
// (beat_tracks.hip: eg_beat_align_tracks).  Both must produce the same bits for a recording that fits the clip call, so the arithmetic that
// rounds -- the paired 2048-point FFT, the RMS tree, the banded mel sums, the fp64 GAHR walk -- exists once, here, and is inlined into both.
#pragma once
#include "common.h"
#include <math.h>

// Two onset frames (f0, f0 + 1) of one recording as one 2048-point complex radix-2 FFT in LDS (frame f0 the real part, f0 + 1 the imaginary
// part), then the 128 mel powers as power_to_db(ref=1.0) before the floor and the frame RMS.  One workgroup of 256 threads.
//   clip [n_samples]: the recording (centre padding is zero on both sides: nothing outside [0, n_samples) is read);
//   meldb [128][n_frames] and rms [n_frames]: this recording's slices.
// Returns the dB value this thread stored (band tid & 127 of frame f0 + (tid >> 7)), -inf when that frame does not exist.
__device__ __forceinline__ float beat_stft_frames(const float* __restrict__ clip, int n_samples, const float* __restrict__ melfb_t,
                                                  const float* __restrict__ window, const float* __restrict__ twiddle,
                                                  const int* __restrict__ band, float* __restrict__ meldb, float* __restrict__ rms,
                                                  int n_frames, int f0) {
    __shared__ float re[2048], im[2048], tws[2048];
    __shared__ float red[2][4];
    const int f1 = f0 + 1, tid = threadIdx.x;
    int live = 0;                          // bit 0 / 1: frame f0 / f1 has a non-zero windowed sample
    for (int i = tid; i < 2048; i += 256) {
        const int s0 = f0 * 512 - 1024 + i, s1 = s0 + 512;
        const float wv = window[i];
        const int r = (int)(__brev((unsigned)i) >> 21);       // 11-bit reversal
        const float a = (s0 >= 0 && s0 < n_samples) ? clip[s0] * wv : 0.f;
        const float c = (f1 < n_frames && s1 >= 0 && s1 < n_samples) ? clip[s1] * wv : 0.f;
        re[r] = a; im[r] = c;
        live |= (a != 0.f) | ((c != 0.f) << 1);
        tws[i] = twiddle[i];
    }
    // an all-zero frame keeps an exactly zero spectrum (librosa transforms each frame alone): without this the pairing's fp32 cross-talk
    // from a loud partner frame gives a silent frame a tiny RMS and moves onset_backtrack's minima on it
    const bool live0 = __syncthreads_or(live & 1), live1 = __syncthreads_or(live & 2);
#pragma unroll 1
    for (int s = 0; s < 11; ++s) {
        const int half = 1 << s;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = tid + u * 256;
            const int pos = j & (half - 1), i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half;
            const int tw = pos << (10 - s);
            const float c = tws[2 * tw], sn = tws[2 * tw + 1];             // exp(-2*pi*i*tw/2048) = c + i*sn
            const float xr = re[i1], xi = im[i1];
            const float tr = xr * c - xi * sn, ti = xr * sn + xi * c;
            const float ar = re[i0], ai = im[i0];
            re[i0] = ar + tr; im[i0] = ai + ti;
            re[i1] = ar - tr; im[i1] = ai - ti;
        }
        __syncthreads();
    }
    // power spectra of the two frames, bins 0..1024: thread tid takes k = tid + 256 u (and 1024 on thread 0)
    float pa[5], pb[5];
    float ra = 0.f, rb = 0.f;             // RMS partial sums, fixed order (k ascending per thread, then a fixed tree)
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const int k = u < 4 ? tid + u * 256 : 1024, nk = (2048 - k) & 2047;
        pa[u] = pb[u] = 0.f;
        if (u < 4 || tid == 0) {
            const float zr = re[k], zi = im[k], yr = re[nk], yi = im[nk];
            const float r0 = 0.5f * (zr + yr), i0 = 0.5f * (zi - yi);      // X0[k]
            const float r1 = 0.5f * (zi + yi), i1 = 0.5f * (yr - zr);      // X1[k]
            pa[u] = live0 ? r0 * r0 + i0 * i0 : 0.f;
            pb[u] = live1 ? r1 * r1 + i1 * i1 : 0.f;
            const float h = (k == 0 || k == 1024) ? 0.5f : 1.f;            // feature.rms(S=...): DC and Nyquist halved
            ra += h * pa[u];
            rb += h * pb[u];
        }
    }
    ra = wave_sum(ra);
    rb = wave_sum(rb);
    if ((tid & 63) == 0) { red[0][tid >> 6] = ra; red[1][tid >> 6] = rb; }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) { re[tid + u * 256] = pa[u]; im[tid + u * 256] = pb[u]; }
    if (tid == 0) { re[1024] = pa[4]; im[1024] = pb[4]; }
    if (tid < 2) {
        const int f = f0 + tid;
        const float s = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        if (f < n_frames) rms[f] = sqrtf(2.f * s / 4194304.f);      // 2 sum / n_fft^2
    }
    __syncthreads();
    // mel projection over the banded filters, thread (m = tid & 127, frame = tid >> 7); stored as power_to_db(ref=1.0) before the floor
    const int m = tid & 127, fr = tid >> 7, f = f0 + fr;
    const float* pw = fr ? im : re;
    const int b0 = band[2 * m], b1 = band[2 * m + 1];
    float s = 0.f;
    for (int k = b0; k < b1; ++k) s += melfb_t[k * 128 + m] * pw[k];
    if (f >= n_frames) return -INFINITY;
    const float db = 10.f * log10f(fmaxf(1e-10f, s));
    meldb[(size_t)m * n_frames + f] = db;
    return db;
}

// fp64 GAHR (Beat_score_v2.py:159-171) of one (audio set, pose set): mean over audio beats of exp(-d^2 / (2 sigma^2)), d = distance to the
// nearest pose beat (both lists ascending: the nearest is one of the two pose beats around the audio beat; |p - a| is monotone in p, so this
// is the same minimum upstream's double loop finds).  An empty pose set gives d = inf -> 0.  Index = short (clip call, lists in LDS) or
// int32 (whole recordings, lists in global memory).
template <typename Index>
__device__ __forceinline__ double beat_gahr(const Index* __restrict__ ev, int n_ev, const Index* __restrict__ pb, int n_pb, int fps,
                                            double sigma) {
    double acc = 0.0;
    int j = 0;
    for (int i = 0; i < n_ev; ++i) {
        const double a = (double)(ev[i] * 512) / 22050.0;
        while (j < n_pb && (double)pb[j] / (double)fps < a) ++j;
        double d = INFINITY;
        if (j < n_pb) d = fmin(d, fabs((double)pb[j] / (double)fps - a));
        if (j > 0) d = fmin(d, fabs((double)pb[j - 1] / (double)fps - a));
        acc += exp(-(d * d) / (2.0 * (sigma * sigma)));
    }
    return acc / (double)n_ev;
}
