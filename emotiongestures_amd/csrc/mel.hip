// Mel front-end: extract_melspectrogram (utils/train_utils_BEAT.py:186-190) = librosa.feature.melspectrogram(
// n_fft=1024, hop=512, power=2) -> power_to_db(ref=np.max) -> float16, then the loader's column slice
// (data_loader/lmdb_loader_BEAT_full.py:229).  librosa defaults: centred frames with zero padding, periodic Hann,
// Slaney mel basis (fmin 0, fmax sr/2, slaney norm), amin 1e-10, top_db 80.
//
// kernel 1: one workgroup per (frame pair, clip): the two windowed frames go from the clip straight into registers (coalesced 4-byte loads,
//           hop 512 => each sample is read by two pairs, L2 absorbs it), one 1024-point complex radix-4 Stockham FFT with four points per
//           thread in registers (5 passes, 8-byte LDS exchanges, twiddles from an LDS copy of the table), |X|^2, then the banded 128x513 mel
//           projection against the transposed filter table [513][128].  EG_MEL_FFT=2 keeps the earlier all-in-LDS radix-2 kernel for A/B runs.
// kernel 2: one workgroup per clip: max reduction, dB, floor, fp16 rounding, slice.
#include "common.h"
#include "beat_shared.h"
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace {

// Two frames per transform: frame 2j is the real part and frame 2j+1 the imaginary part of ONE 1024-point complex FFT; their spectra separate
// as X0[k] = (Z[k] + conj Z[N-k]) / 2, X1[k] = (Z[k] - conj Z[N-k]) / 2i.  Halves the butterflies per frame (the first version transformed one
// real frame with a zero imaginary part).  The cross-talk between the two frames is bounded by fp32 round-off of the louder one (power floor
// ~4e-15 of its power: 60 dB below the 80 dB clamp of power_to_db).
// Radix-2 form (EG_MEL_FFT=2, this round's A/B reference): everything in LDS, bit-reversed staging, 10 stages of 512 butterflies.
__global__ __launch_bounds__(256) void mel_power_radix2_kernel(const float* __restrict__ audio, int n_samples, const float* __restrict__ melfb_t,
                                                               const float* __restrict__ window, const float* __restrict__ twiddle,
                                                               const int* __restrict__ band, float* __restrict__ melpow, int n_frames) {
    __shared__ float re[1024], im[1024];
    const int f0 = blockIdx.x * 2, f1 = f0 + 1, b = blockIdx.y, tid = threadIdx.x;
    const float* clip = audio + (size_t)b * n_samples;
    for (int i = tid; i < 1024; i += 256) {
        const int s0 = f0 * 512 - 512 + i, s1 = s0 + 512;
        const float wv = window[i];
        const int r = (int)(__brev((unsigned)i) >> 22);       // 10-bit reversal
        re[r] = (s0 >= 0 && s0 < n_samples) ? clip[s0] * wv : 0.f;
        im[r] = (f1 < n_frames && s1 >= 0 && s1 < n_samples) ? clip[s1] * wv : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 10; ++s) {
        const int half = 1 << s;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = tid + u * 256;
            const int pos = j & (half - 1), i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half;
            const int tw = pos << (9 - s);
            const float c = twiddle[2 * tw], sn = twiddle[2 * tw + 1];     // exp(-2*pi*i*tw/1024) = c + i*sn
            const float xr = re[i1], xi = im[i1];
            const float tr = xr * c - xi * sn, ti = xr * sn + xi * c;
            const float ar = re[i0], ai = im[i0];
            re[i0] = ar + tr; im[i0] = ai + ti;
            re[i1] = ar - tr; im[i1] = ai - ti;
        }
        __syncthreads();
    }
    // power spectra of the two frames, bins 0..512: thread tid takes k = tid, tid + 256 (and 512 on thread 0)
    float pa[3], pb[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int k = u < 2 ? tid + u * 256 : 512, nk = (1024 - k) & 1023;
        pa[u] = pb[u] = 0.f;
        if (u < 2 || tid == 0) {
            const float zr = re[k], zi = im[k], yr = re[nk], yi = im[nk];
            const float r0 = 0.5f * (zr + yr), i0 = 0.5f * (zi - yi);      // X0[k]
            const float r1 = 0.5f * (zi + yi), i1 = 0.5f * (yr - zr);      // X1[k]
            pa[u] = r0 * r0 + i0 * i0;
            pb[u] = r1 * r1 + i1 * i1;
        }
    }
    __syncthreads();
    re[tid] = pa[0]; re[tid + 256] = pa[1];
    im[tid] = pb[0]; im[tid + 256] = pb[1];
    if (tid == 0) { re[512] = pa[2]; im[512] = pb[2]; }
    __syncthreads();
    // mel projection: the Slaney filters are triangles, so mel m only touches bins [band[2m], band[2m+1]) (~2*513 non-zeros in total instead of
    // 128*513); thread (m = tid & 127, frame = tid >> 7) sums its band in bin order
    const int m = tid & 127, fr = tid >> 7, f = f0 + fr;
    const float* pw = fr ? im : re;
    const int b0 = band[2 * m], b1 = band[2 * m + 1];
    float s = 0.f;
    for (int k = b0; k < b1; ++k) s += melfb_t[k * 128 + m] * pw[k];
    if (f < n_frames) melpow[((size_t)b * 128 + m) * n_frames + f] = s;
}

// ---- radix-4 Stockham transform, four points per thread in registers -------------------------------------------------------------------
// Pass p (NS = 4^p, p = 0..4), thread j = 0..255:  v[r] = in[j + 256 r] * exp(-2 pi i r k / (4 NS)),  k = j mod NS;  4-point DFT of v;
// out[4 (j - k) + k + r NS] = y[r].  After the fifth pass `out` is the spectrum in natural order (autosort: no digit reversal anywhere).
// Pass 0 has k = 0 (no twiddle) and its inputs j + 256 r are the coalesced global loads themselves, so nothing is staged.
//
// Exchange layout: complex element i lives in float2 slot i ^ (5 * ((i >> 4) & 3)) -- bits 4..5 of i are XORed into bits 0..1 and 2..3.
// Bank arithmetic (8-byte accesses; a write is served in groups of 16 consecutive lanes over 32 four-byte banks, so a group is conflict-free
// when its 16 slots differ mod 16; a read in groups of 32 lanes over 64 banks, conflict-free when its 32 slots differ mod 32):
//   reads  i = j + 256 r: a group's 32 lanes cover one aligned run of 32 elements; the swizzle permutes each aligned 16 within itself -> distinct.
//   writes NS = 1:  i = 4 j + r; lanes l = 0..15 of a group have i mod 16 = 4 (l & 3) + r, four lanes per residue (4-way) unswizzled;
//                   bits 4..5 of i are l >> 2, so the slot mod 16 is 4 ((l & 3) ^ (l >> 2)) + (r ^ (l >> 2)) -> distinct.
//   writes NS = 4:  i = 16 (j >> 2) + (j & 3) + 4 r; i mod 16 = (l & 3) + 4 r (4-way unswizzled), bits 4..5 = l >> 2, slot mod 16 =
//                   ((l & 3) ^ (l >> 2)) + 4 (r ^ (l >> 2)) -> distinct.
//   writes NS >= 16: a group's 16 lanes write one aligned run of 16 elements -> distinct.
__device__ __forceinline__ int fft_slot(int i) { return i ^ (5 * ((i >> 4) & 3)); }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// the three twiddles of pass NS for thread j: exp(-2 pi i r t / 1024), t = k * 256 / NS, r = 1..3.  The table holds t < 512; 3 t can reach 765,
// and exp(-2 pi i (t + 512) / 1024) = -exp(-2 pi i t / 1024) exactly.
// `tw` is the workgroup's LDS copy of the table, entry t in slot t + (t >> 4): one pad per 16 entries takes the strides 16, 32 and 48 of pass 16
// (16-way on one bank unpadded) apart; what is left is 4-way in pass 64 and 3-way in pass 256 on 12 reads per thread in all, counted by
// tools/mel_fft_walk.py (twiddle_read_conflicts).
__device__ __forceinline__ int tw_slot(int t) { return t + (t >> 4); }
template <int NS>
__device__ __forceinline__ void fft_twiddles(const float2* tw, int j, float2 (&w)[3]) {
    const int t = (j & (NS - 1)) * (256 / NS), t3 = 3 * t;
    w[0] = tw[tw_slot(t)];
    w[1] = tw[tw_slot(2 * t)];
    const float2 x = tw[tw_slot(t3 & 511)];
    w[2] = t3 < 512 ? x : make_float2(-x.x, -x.y);
}

template <int NS>
__device__ __forceinline__ void fft_pass(float2 (&v)[4], const float2 (&w)[3], float2* __restrict__ out, int j) {
    if (NS > 1) {
#pragma unroll
        for (int r = 1; r < 4; ++r) v[r] = cmul(v[r], w[r - 1]);
    }
    const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);      // -i (v1 - v3)
    const int k = j & (NS - 1), base = ((j - k) << 2) + k;
    out[fft_slot(base)] = make_float2(a0.x + a2.x, a0.y + a2.y);
    out[fft_slot(base + NS)] = make_float2(a1.x + a3.x, a1.y + a3.y);
    out[fft_slot(base + 2 * NS)] = make_float2(a0.x - a2.x, a0.y - a2.y);
    out[fft_slot(base + 3 * NS)] = make_float2(a1.x - a3.x, a1.y - a3.y);
}

__device__ __forceinline__ void fft_gather(float2 (&v)[4], const float2* __restrict__ in, int j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = in[fft_slot(j + 256 * r)];
}

__global__ __launch_bounds__(256) void mel_power_kernel(const float* __restrict__ audio, int n_samples, const float* __restrict__ melfb_t,
                                                        const float* __restrict__ window, const float* __restrict__ twiddle,
                                                        const int* __restrict__ band, float* __restrict__ melpow, int n_frames) {
    __shared__ float2 za[1024], zb[1024];          // ping-pong: one barrier per exchange
    const int f0 = blockIdx.x * 2, f1 = f0 + 1, b = blockIdx.y, tid = threadIdx.x;
    const float* clip = audio + (size_t)b * n_samples;
    // sample i = tid + 256 q of frame f0 is clip[s0 + 256 q]; of frame f1 it is clip[s0 + 512 + 256 q]: six distinct loads for the eight points
    float raw[6];
    const int s0 = f0 * 512 - 512 + tid;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int s = s0 + 256 * u;
        raw[u] = (s >= 0 && s < n_samples) ? clip[s] : 0.f;
    }
    float2 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float wv = window[tid + 256 * q];
        v[q] = make_float2(raw[q] * wv, f1 < n_frames ? raw[q + 2] * wv : 0.f);
    }
    // the twiddle table goes to LDS once per workgroup (two coalesced 8-byte loads per thread; zb is free until the second pass writes it)
    {
        const float2* tw = reinterpret_cast<const float2*>(twiddle);
        const float2 ta = tw[tid], tb = tw[tid + 256];
        zb[tw_slot(tid)] = ta;
        zb[tw_slot(tid + 256)] = tb;
    }
    // projection: thread (m = tid >> 1, frame = tid & 1) -- the two frames of a mel in neighbouring lanes read the same filter value, so a wave's
    // filter loads ask for 32 different table lines, not 64; the band limits are requested here, ahead of the transform
    const int m = tid >> 1, fr = tid & 1, f = f0 + fr;
    const int b0 = band[2 * m], b1 = band[2 * m + 1];
    __syncthreads();
    // every pass's twiddles depend on tid alone: read once into registers; the barrier after the first pass orders these reads before the
    // second pass's writes to zb
    float2 w1[3], w2[3], w3[3], w4[3];
    fft_twiddles<4>(zb, tid, w1);
    fft_twiddles<16>(zb, tid, w2);
    fft_twiddles<64>(zb, tid, w3);
    fft_twiddles<256>(zb, tid, w4);
    float2 none[3];
    fft_pass<1>(v, none, za, tid);
    __syncthreads();
    fft_gather(v, za, tid);
    fft_pass<4>(v, w1, zb, tid);
    __syncthreads();
    fft_gather(v, zb, tid);
    fft_pass<16>(v, w2, za, tid);
    __syncthreads();
    fft_gather(v, za, tid);
    fft_pass<64>(v, w3, zb, tid);
    __syncthreads();
    fft_gather(v, zb, tid);
    fft_pass<256>(v, w4, za, tid);
    __syncthreads();
    // power spectra of the two frames, bins 0..512: thread tid takes k = tid, tid + 256 (and 512 on thread 0)
    float pa[3], pb[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int k = u < 2 ? tid + u * 256 : 512, nk = (1024 - k) & 1023;
        pa[u] = pb[u] = 0.f;
        if (u < 2 || tid == 0) {
            const float2 z = za[fft_slot(k)], y = za[fft_slot(nk)];
            const float r0 = 0.5f * (z.x + y.x), i0 = 0.5f * (z.y - y.y);      // X0[k]
            const float r1 = 0.5f * (z.y + y.y), i1 = 0.5f * (y.x - z.x);      // X1[k]
            pa[u] = r0 * r0 + i0 * i0;
            pb[u] = r1 * r1 + i1 * i1;
        }
    }
    // zb is free: its last readers passed the barrier above.  Powers in bin order, frame f0 then frame f1.
    float* re = reinterpret_cast<float*>(zb);
    float* im = re + 1024;
    re[tid] = pa[0]; re[tid + 256] = pa[1];
    im[tid] = pb[0]; im[tid + 256] = pb[1];
    if (tid == 0) { re[512] = pa[2]; im[512] = pb[2]; }
    __syncthreads();
    // mel projection, each sum in bin order as in the radix-2 form.  Eight filter loads are in flight at a time (the widest band has 24 bins:
    // three round trips to the table instead of one per bin)
    const float* pw = fr ? im : re;
    float s = 0.f;
    for (int k0 = b0; k0 < b1; k0 += 8) {
        float wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = k0 + u < b1 ? melfb_t[(k0 + u) * 128 + m] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + u < b1) s += wv[u] * pw[k0 + u];
    }
    if (f < n_frames) melpow[((size_t)b * 128 + m) * n_frames + f] = s;
}

// one workgroup of 1024 threads per clip (the clip maximum couples all its bins; with 256 threads the 64 workgroups of a 64-clip step ran 43 us)
__global__ __launch_bounds__(1024) void mel_db_kernel(const float* __restrict__ melpow, float* __restrict__ spec, int n_frames,
                                                      int out_frames) {
    __shared__ float red[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* p = melpow + (size_t)b * 128 * n_frames;
    float mx = 0.f;
    for (int i = tid; i < 128 * n_frames; i += 1024) mx = fmaxf(mx, p[i]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
    // power_to_db(ref=np.max): 10*log10(max(amin,S)) - 10*log10(max(amin,max S)) = 10*log10(max(amin,S)/ref); the ratio
    // form makes the peak (and an all-silent clip) exactly 0 dB, as in exact arithmetic.  max(db) = 0 => floor = -top_db.
    const float inv_ref = 1.0f / fmaxf(1e-10f, mx);
    const float floor_db = -80.f;
    for (int i = tid; i < 128 * out_frames; i += 1024) {
        const int m = i / out_frames, f = i - m * out_frames;
        float db = 10.f * log10f(fmaxf(1e-10f, p[m * n_frames + f]) * inv_ref);
        db = fmaxf(db, floor_db);
        spec[((size_t)b * 128 + m) * out_frames + f] = __half2float(__float2half_rn(db));
    }
}

double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

}  // namespace

namespace {

// Slaney mel filterbank (librosa.filters.mel, sr 16 kHz, fmin 0, fmax sr/2, slaney norm) TRANSPOSED [n_fft/2+1][128], per-mel non-zero bin
// range [128][2] (begin, end), periodic Hann [n_fft], twiddles (cos, -sin) [n_fft/2][2].  Shared by the n_fft 1024 spectrogram front-end and
// the n_fft 2048 onset front-end of the beat score.
void mel_tables_host(int n_fft, float* h_melfb_t, float* h_window, float* h_twiddle, int32_t* h_band) {
    const int n_mels = 128, n_bins = n_fft / 2 + 1;
    const double sr = 16000.0;
    double hz[130];
    const double m_lo = hz_to_mel(0.0), m_hi = hz_to_mel(sr / 2);
    for (int i = 0; i < n_mels + 2; ++i) hz[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    for (int m = 0; m < n_mels; ++m) {
        const double enorm = 2.0 / (hz[m + 2] - hz[m]);
        for (int k = 0; k < n_bins; ++k) {
            const double fk = (sr / 2) * k / (n_bins - 1);
            const double lower = (fk - hz[m]) / (hz[m + 1] - hz[m]);
            const double upper = (hz[m + 2] - fk) / (hz[m + 2] - hz[m + 1]);
            double w = lower < upper ? lower : upper;
            if (w < 0) w = 0;
            h_melfb_t[k * 128 + m] = (float)(w * enorm);
        }
        int lo = n_bins, hi = 0;
        for (int k = 0; k < n_bins; ++k)
            if (h_melfb_t[k * 128 + m] != 0.f) { if (k < lo) lo = k; hi = k + 1; }
        if (lo > hi) lo = hi = 0;
        h_band[2 * m] = lo; h_band[2 * m + 1] = hi;
    }
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n_fft; ++i) h_window[i] = (float)(0.5 - 0.5 * cos(2.0 * pi * i / n_fft));
    for (int t = 0; t < n_fft / 2; ++t) {
        h_twiddle[2 * t] = (float)cos(2.0 * pi * t / n_fft);
        h_twiddle[2 * t + 1] = (float)(-sin(2.0 * pi * t / n_fft));
    }
}

}  // namespace

// Host tables: Slaney mel filterbank TRANSPOSED [513][128], periodic Hann [1024], twiddles (cos, -sin) [512][2],
// per-mel non-zero bin range [128][2] (begin, end).
extern "C" int eg_mel_tables(float* h_melfb_t, float* h_window, float* h_twiddle, int32_t* h_band) {
    EG_REQUIRE(h_melfb_t && h_window && h_twiddle && h_band, EG_ERR_BAD_ARG, "eg_mel_tables: null pointer");
    mel_tables_host(1024, h_melfb_t, h_window, h_twiddle, h_band);
    return EG_OK;
}

extern "C" int64_t eg_mel_workspace_bytes(int32_t batch, int32_t n_samples) {
    const int n_frames = 1 + n_samples / 512;
    return (int64_t)batch * 128 * n_frames * (int64_t)sizeof(float);
}

extern "C" int eg_melspectrogram(const float* audio, int32_t batch, int32_t n_samples, const float* d_melfb_t,
                                 const float* d_window, const float* d_twiddle, const int32_t* d_band, float* spec, int32_t out_frames,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    EG_REQUIRE(audio && d_melfb_t && d_window && d_twiddle && d_band && spec && workspace, EG_ERR_BAD_ARG, "eg_melspectrogram: null pointer");
    EG_REQUIRE(batch > 0 && n_samples >= 512, EG_ERR_BAD_ARG, "eg_melspectrogram: batch=%d n_samples=%d", batch, n_samples);
    const int n_frames = 1 + n_samples / 512;
    EG_REQUIRE(out_frames > 0 && out_frames <= n_frames, EG_ERR_BAD_ARG, "eg_melspectrogram: out_frames=%d of %d", out_frames, n_frames);
    EG_REQUIRE(workspace_bytes >= eg_mel_workspace_bytes(batch, n_samples), EG_ERR_WORKSPACE, "eg_melspectrogram: workspace too small");
    // EG_MEL_FFT (read per call, like EG_GEMM_TILE): unset, empty or "4" = the register radix-4 transform; "2" = the radix-2 LDS transform
    // (A/B runs and the accuracy comparison of tests/test_gpu_mel_fft.py, this round only).  Anything else is refused before any launch.
    const char* fft = getenv("EG_MEL_FFT");
    const bool radix2 = fft && !strcmp(fft, "2");
    EG_REQUIRE(!fft || !fft[0] || radix2 || !strcmp(fft, "4"), EG_ERR_BAD_ARG, "EG_MEL_FFT=\"%s\": accepted values are \"4\" and \"2\" (unset or empty: 4)", fft);
    hipStream_t st = (hipStream_t)stream;
    float* melpow = reinterpret_cast<float*>(workspace);
    if (radix2)
        hipLaunchKernelGGL(mel_power_radix2_kernel, dim3((n_frames + 1) / 2, batch), dim3(256), 0, st, audio, n_samples, d_melfb_t, d_window,
                           d_twiddle, d_band, melpow, n_frames);
    else
        hipLaunchKernelGGL(mel_power_kernel, dim3((n_frames + 1) / 2, batch), dim3(256), 0, st, audio, n_samples, d_melfb_t, d_window, d_twiddle,
                           d_band, melpow, n_frames);
    int rc = eg_check_launch("mel_power");
    if (rc) return rc;
    hipLaunchKernelGGL(mel_db_kernel, dim3(batch), dim3(1024), 0, st, melpow, spec, n_frames, out_frames);
    return eg_check_launch("mel_db");
}

// ==== Beat-alignment score (model/Beat_score_v2.py:51-197, alignment(sigma, order)) ===================================================
// Audio half = alignment.load_audio restated from librosa 0.10's documented routines (librosa itself is not pinned against here):
//   onset_strength(y, sr=16000): |STFT|^2 (n_fft 2048, hop 512, centred, zero pad, periodic Hann) -> 128 Slaney mels (fmax 8000)
//     -> power_to_db(ref=1.0, amin 1e-10, top_db 80 below the CLIP max) -> mean over mels of max(0, db[t] - db[t-1]), left-padded by
//     lag + n_fft/(2 hop) = 3 frames and trimmed to T = 1 + n/512;
//   onset_detect(onset_envelope=oenv) with librosa's default sr 22050: x = (oenv - min) / (max + tiny), peak_pick(pre_max 1, post_max 1,
//     pre_avg 4, post_avg 5, wait 1, delta 0.07);
//   onset_backtrack(events, oenv) and onset_backtrack(events, rms) with rms = feature.rms(S=|X|) (DC and Nyquist bins halved).
// Pose half = load_pose: velocity L2 norms of 8 joint groups (pose columns 18:42 and 150:174), beats = argrelextrema(np.less, order,
// mode clip); the four right-side curves are sliced [t_start*fps : t_end*fps], the left ones are not (upstream quirk, kept).
// Score = calculate_align: GAHR over 3 audio x 8 pose beat sets in fp64, audio beat times frame*512/22050 (librosa's default sr on 16 kHz
// audio, upstream quirk, kept), pose beat times idx/fps.
//
// kernel 1 (beat_stft_kernel): one workgroup per (frame pair, clip); two real frames as one 2048-point complex radix-2 FFT in LDS (as
//           mel_power_kernel), epilogue: the 128 mel powers as dB (banded Slaney filters) and the frame RMS; the spectrum stays in LDS.
// kernel 2 (beat_align_kernel): one workgroup per clip: clip dB max, floor, flux -> oenv, normalisation, peak candidates (parallel), the
//           wait-suppressed scan (one lane), both backtracks, pose velocity norms and extrema straight from [B, F, D], 24 GAHR terms.
#define EG_BEAT_MAX_EVENTS (EG_BEAT_MAX_FRAMES / 2 + 1)

namespace {

__global__ __launch_bounds__(256) void beat_stft_kernel(const float* __restrict__ audio, int n_samples, const float* __restrict__ melfb_t,
                                                        const float* __restrict__ window, const float* __restrict__ twiddle,
                                                        const int* __restrict__ band, float* __restrict__ meldb, float* __restrict__ rms,
                                                        int n_frames) {
    const int b = blockIdx.y;
    beat_stft_frames(audio + (size_t)b * n_samples, n_samples, melfb_t, window, twiddle, band, meldb + (size_t)b * 128 * n_frames,
                     rms + (size_t)b * n_frames, n_frames, blockIdx.x * 2);
}

__device__ double gahr(const short* __restrict__ ev, int n_ev, const short* __restrict__ pb, int n_pb, int fps, double sigma) {
    return beat_gahr(ev, n_ev, pb, n_pb, fps, sigma);
}

__global__ __launch_bounds__(256) void beat_align_kernel(const float* __restrict__ meldb, const float* __restrict__ rms_ws, int n_frames,
                                                         const float* __restrict__ pose, int pose_frames, int pose_dim, int fps, int r_lo,
                                                         int r_hi, double sigma, int order, double* __restrict__ score,
                                                         int* __restrict__ n_audio_beats, float* __restrict__ oenv_out,
                                                         float* __restrict__ rms_out, uint8_t* __restrict__ audio_mask,
                                                         uint8_t* __restrict__ pose_mask) {
    __shared__ float oenv[EG_BEAT_MAX_FRAMES], x[EG_BEAT_MAX_FRAMES], rms[EG_BEAT_MAX_FRAMES];
    __shared__ uint8_t fl[3][EG_BEAT_MAX_FRAMES];          // peak candidates, oenv minima, rms minima; then the three beat counts
    uint8_t* cand = fl[0];
    uint8_t* min_o = fl[1];
    uint8_t* min_r = fl[2];
    __shared__ short ev[3][EG_BEAT_MAX_EVENTS];
    __shared__ float vel[8][EG_BEAT_MAX_FRAMES];
    __shared__ short pbeat[8][EG_BEAT_MAX_EVENTS];
    __shared__ int n_pb[8];
    __shared__ float redf[2][4];
    __shared__ int n_ev_s, any_s;
    __shared__ double g24[24];
    const int b = blockIdx.x, tid = threadIdx.x, T = n_frames;
    const float* db = meldb + (size_t)b * 128 * T;

    // ---- onset envelope: clip dB max -> floor, flux, mean over the 128 bands (fixed order)
    float mx = -INFINITY;
    for (int i = tid; i < 128 * T; i += 256) mx = fmaxf(mx, db[i]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) redf[0][tid >> 6] = mx;
    __syncthreads();
    const float floor_db = fmaxf(fmaxf(redf[0][0], redf[0][1]), fmaxf(redf[0][2], redf[0][3])) - 80.f;
    for (int t = tid; t < T; t += 256) {
        float s = 0.f;
        if (t >= 3)
#pragma unroll 8
            for (int m = 0; m < 128; ++m) {
                const float cur = fmaxf(db[m * T + t - 2], floor_db), prev = fmaxf(db[m * T + t - 3], floor_db);
                s += fmaxf(0.f, cur - prev);
            }
        oenv[t] = s / 128.f;
        rms[t] = rms_ws[(size_t)b * T + t];
    }
    __syncthreads();
    // ---- onset_detect normalisation: x = (oenv - min) / (max(oenv - min) + tiny(float32))
    float lo = INFINITY, hi = -INFINITY;
    for (int t = tid; t < T; t += 256) { lo = fminf(lo, oenv[t]); hi = fmaxf(hi, oenv[t]); }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((tid & 63) == 0) { redf[0][tid >> 6] = lo; redf[1][tid >> 6] = hi; }
    if (tid == 0) any_s = 0;
    __syncthreads();
    lo = fminf(fminf(redf[0][0], redf[0][1]), fminf(redf[0][2], redf[0][3]));
    hi = fmaxf(fmaxf(redf[1][0], redf[1][1]), fmaxf(redf[1][2], redf[1][3]));
    const float den = (hi - lo) + 1.17549435e-38f;
    int bad = 0, nz = 0;
    for (int t = tid; t < T; t += 256) {
        const float v = (oenv[t] - lo) / den;
        x[t] = v;
        bad |= !isfinite(v);
        nz |= v != 0.f;
    }
    if (bad) atomicOr(&any_s, 2);           // flags only (order-free): 1 = some x != 0, 2 = a non-finite x
    if (nz) atomicOr(&any_s, 1);
    __syncthreads();
    const bool detect = any_s == 1;
    // peak candidates: x[n] == max(x[n-1 : n+1]) and x[n] >= mean(x[n-4 : n+5]) + delta (windows clipped to the clip); fp32, fixed order
    for (int t = tid; t < T; t += 256) {
        const float v = x[t];
        const bool is_max = t == 0 || v >= x[t - 1];
        const int a0 = t - 4 < 0 ? 0 : t - 4, a1 = t + 5 > T ? T : t + 5;
        float s = 0.f;
        for (int i = a0; i < a1; ++i) s += x[i];
        // peak_pick's numba loop: fp32 running sum, mean and threshold in fp64 with delta cast to fp32 (its guvectorize signature)
        cand[t] = detect && is_max && (double)v >= (double)s / (double)(a1 - a0) + (double)0.07f;
        // onset_backtrack minima (frame 0 always): e[i] <= e[i-1] and e[i] < e[i+1]
        min_o[t] = t == 0 || (t < T - 1 && oenv[t] <= oenv[t - 1] && oenv[t] < oenv[t + 1]);
        min_r[t] = t == 0 || (t < T - 1 && rms[t] <= rms[t - 1] && rms[t] < rms[t + 1]);
    }
    __syncthreads();
    if (tid == 0) {                         // wait = 1: after an accepted peak the next frame is skipped
        int n = 0, c = 0;
        while (n < T) {
            if (cand[n]) { ev[0][c++] = (short)n; n += 2; } else ++n;
        }
        n_ev_s = c;
    }
    __syncthreads();
    const int n_ev = n_ev_s;
    for (int i = tid; i < n_ev; i += 256) {       // backtrack: the largest minimum <= the event
        int j = ev[0][i];
        while (!min_o[j]) --j;
        ev[1][i] = (short)j;
        j = ev[0][i];
        while (!min_r[j]) --j;
        ev[2][i] = (short)j;
    }
    if (n_audio_beats && tid == 0) n_audio_beats[b] = n_ev;
    for (int t = tid; t < T; t += 256) {
        if (oenv_out) oenv_out[(size_t)b * T + t] = oenv[t];
        if (rms_out) rms_out[(size_t)b * T + t] = rms[t];
    }
    __syncthreads();
    if (audio_mask) {                       // onset_raw as 0/1; the backtracked sets as multiplicities (two events can share a minimum)
        for (int t = tid; t < T; t += 256) fl[0][t] = fl[1][t] = fl[2][t] = 0;      // free once the backtracks above are done
        __syncthreads();
        if (tid < 3)
            for (int i = 0; i < n_ev; ++i) {
                const int f = ev[tid][i];
                fl[tid][f] = (uint8_t)min(255, fl[tid][f] + 1);
            }
        __syncthreads();
        uint8_t* am = audio_mask + (size_t)b * 3 * T;
        for (int t = tid; t < T; t += 256) { am[t] = fl[0][t]; am[T + t] = fl[1][t]; am[2 * T + t] = fl[2][t]; }
    }
    if (!pose) return;

    // ---- pose half: vel = p[t+1] - p[t] on columns 18:42 ++ 150:174, per-group L2 norm summed in numpy's order (no FMA contraction)
    const int L = pose_frames - 1;
    const float* pp = pose + (size_t)b * pose_frames * pose_dim;
    for (int i = tid; i < 8 * L; i += 256) {
        const int g = i / L, t = i - g * L;          // g = vel column group 0..7 (right shoulder, arm, fore arm, wrist, left ...)
        const int c0 = g < 4 ? 18 + 6 * g : 150 + 6 * (g - 4);
        const float* r0 = pp + (size_t)t * pose_dim + c0;
        const float* r1 = r0 + pose_dim;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float d = __fsub_rn(r1[c], r0[c]);
            s = c == 0 ? __fmul_rn(d, d) : __fadd_rn(s, __fmul_rn(d, d));
        }
        vel[g][t] = __fsqrt_rn(s);
    }
    __syncthreads();
    // argrelextrema(np.less, order, mode='clip') per returned set q (upstream order: right arm, shoulder, fore arm, wrist, left arm, ...);
    // lane q compacts its own set, so each list is ascending
    if (tid < 8) {
        const int q = tid;
        const int g = q == 0 ? 1 : q == 1 ? 0 : q == 4 ? 5 : q == 5 ? 4 : q;
        const int s0 = q < 4 ? min(r_lo, L) : 0, s1 = q < 4 ? min(r_hi, L) : L;
        const int len = s1 > s0 ? s1 - s0 : 0;
        const float* c = &vel[g][s0];
        int cnt = 0;
        for (int i = 0; i < len; ++i) {
            bool ok = true;
            for (int k = 1; k <= order && ok; ++k) {
                const int ip = i + k < len ? i + k : len - 1, im_ = i - k > 0 ? i - k : 0;
                ok = c[i] < c[ip] && c[i] < c[im_];
            }
            if (ok) pbeat[q][cnt++] = (short)i;
        }
        n_pb[q] = cnt;
        if (pose_mask) {
            uint8_t* pm = pose_mask + ((size_t)b * 8 + q) * L;
            for (int i = 0; i < L; ++i) pm[i] = 0;
            for (int i = 0; i < cnt; ++i) pm[pbeat[q][i]] = 1;
        }
    }
    __syncthreads();
    // ---- calculate_align: 24 GAHR terms (audio set major), summed in upstream's order, / 24
    if (tid < 24 && n_ev > 0) g24[tid] = gahr(ev[tid / 8], n_ev, pbeat[tid % 8], n_pb[tid % 8], fps, sigma);
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < 24; ++i) acc += g24[i];
        score[b] = n_ev > 0 ? acc / 24.0 : (double)NAN;
    }
}

}  // namespace

// Host tables of the onset front-end: Slaney filterbank TRANSPOSED [1025][128], periodic Hann [2048], twiddles (cos, -sin) [1024][2],
// per-mel non-zero bin range [128][2].
extern "C" int eg_beat_tables(float* h_melfb_t, float* h_window, float* h_twiddle, int32_t* h_band) {
    EG_REQUIRE(h_melfb_t && h_window && h_twiddle && h_band, EG_ERR_BAD_ARG, "eg_beat_tables: null pointer");
    mel_tables_host(2048, h_melfb_t, h_window, h_twiddle, h_band);
    return EG_OK;
}

extern "C" int64_t eg_beat_workspace_bytes(int32_t batch, int32_t n_samples) {
    const int n_frames = 1 + n_samples / 512;
    return (int64_t)batch * 129 * n_frames * (int64_t)sizeof(float);      // mel dB [B,128,T] + rms [B,T]
}

extern "C" int eg_beat_align(const float* audio, int32_t batch, int32_t n_samples, const float* pose, int32_t frames, int32_t pose_dim,
                             int32_t pose_fps, int32_t t_start, int32_t t_end, double sigma, int32_t order, const float* d_melfb_t,
                             const float* d_window, const float* d_twiddle, const int32_t* d_band, void* workspace, int64_t workspace_bytes,
                             double* score, int32_t* n_audio_beats, float* oenv, float* rms, uint8_t* audio_beats, uint8_t* pose_beats,
                             void* stream) {
    EG_REQUIRE(audio && d_melfb_t && d_window && d_twiddle && d_band && workspace, EG_ERR_BAD_ARG, "eg_beat_align: null pointer");
    EG_REQUIRE(batch > 0 && n_samples >= 2048, EG_ERR_BAD_ARG, "eg_beat_align: batch=%d n_samples=%d (needs >= 2048)", batch, n_samples);
    const int n_frames = 1 + n_samples / 512;
    EG_REQUIRE(n_frames <= EG_BEAT_MAX_FRAMES, EG_ERR_BAD_ARG, "eg_beat_align: %d onset frames (n_samples=%d) exceed %d", n_frames, n_samples,
               EG_BEAT_MAX_FRAMES);
    EG_REQUIRE(workspace_bytes >= eg_beat_workspace_bytes(batch, n_samples), EG_ERR_WORKSPACE, "eg_beat_align: workspace too small");
    if (pose) {
        EG_REQUIRE(score, EG_ERR_BAD_ARG, "eg_beat_align: null score");
        EG_REQUIRE(pose_dim >= 174, EG_ERR_BAD_ARG, "eg_beat_align: pose_dim=%d (the beat joints are columns 18:42 and 150:174)", pose_dim);
        EG_REQUIRE(frames >= 2 && frames - 1 <= EG_BEAT_MAX_FRAMES, EG_ERR_BAD_ARG, "eg_beat_align: frames=%d (2..%d)", frames,
                   EG_BEAT_MAX_FRAMES + 1);
        EG_REQUIRE(pose_fps > 0 && order >= 1 && sigma > 0.0, EG_ERR_BAD_ARG, "eg_beat_align: pose_fps=%d order=%d sigma=%g", pose_fps,
                   order, sigma);
        EG_REQUIRE(t_start >= 0 && t_start < t_end && (int64_t)t_end * pose_fps < (1 << 30), EG_ERR_BAD_ARG,
                   "eg_beat_align: t_start=%d t_end=%d", t_start, t_end);
    }
    hipStream_t st = (hipStream_t)stream;
    float* meldb = reinterpret_cast<float*>(workspace);
    float* rms_ws = meldb + (size_t)batch * 128 * n_frames;
    hipLaunchKernelGGL(beat_stft_kernel, dim3((n_frames + 1) / 2, batch), dim3(256), 0, st, audio, n_samples, d_melfb_t, d_window, d_twiddle,
                       d_band, meldb, rms_ws, n_frames);
    int rc = eg_check_launch("beat_stft");
    if (rc) return rc;
    const int r_lo = pose ? t_start * pose_fps : 0, r_hi = pose ? t_end * pose_fps : 0;
    hipLaunchKernelGGL(beat_align_kernel, dim3(batch), dim3(256), 0, st, meldb, rms_ws, n_frames, pose, frames, pose_dim, pose_fps, r_lo, r_hi,
                       sigma, order, score, n_audio_beats, oenv, rms, audio_beats, pose_beats);
    return eg_check_launch("beat_align");
}
