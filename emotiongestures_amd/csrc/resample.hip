// Polyphase resampler (include/emogest.h: eg_resample_plan, eg_resample_filter, eg_resample, eg_resample_stream_*): audio at any common rate
// to the model's rate on the device, offline for whole (ragged) recordings and push by push for a live stream.
//   y[n] = sum_i x[i] * h[half + (n - delay)*M - i*L],  h = firwin(2*half + 1, 1 / max(L, M), kaiser beta 5) * L  (scipy's resample_poly design)
// With p = half + (n - delay)*M, i_hi = floor(p / L) and phase = p - i_hi*L the sum is sum_{j < K} x[i_hi - j] * bank[phase][j], bank[phase][j] =
// h[phase + j*L] (0 past the last tap).  One device function (resample_dot) computes that sum for the offline kernel and for the stream
// kernel from an LDS copy of the input span, in the order j = 0 .. K-1 with one fmaf per tap, so a stream reproduces the delayed offline
// signal bit for bit.  Every output element has one owning thread; plain vector stores, no atomics.
#include "common.h"
#include <math.h>
#include <vector>

namespace {

constexpr int TILE = EG_RESAMPLE_TILE;                  // outputs of one workgroup
constexpr int THREADS = 256;
constexpr int PER = TILE / THREADS;                     // outputs per thread and pass, THREADS apart (lane-consecutive outputs: the x reads of a wave are M/L apart)
constexpr int LDS_FLOATS = 16000;                       // 64000 bytes: bank (when it is kept there) + input span
constexpr int MAX_LM = EG_RESAMPLE_MAX_FACTOR;
constexpr int MAX_U = 65535;
constexpr int SPAN_PAD = 8;                             // the span starts up to 3 floats early (16-byte loads) and is staged in whole quads

enum { MODE_L1 = 0, MODE_BANK_LDS = 1, MODE_BANK_GLOBAL = 2 };

struct Geo {                                            // what a kernel needs of the plan, by value
    int L, M, half, K, pitch;
    int bank_lds;                                       // floats of LDS the bank takes (0: it stays in global memory), a multiple of 4
    int sub;                                            // outputs per staged span (<= TILE)
};

__host__ __device__ inline long long floordiv(long long a, long long b) {      // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ inline long long out_len(long long n_in, int L, int M) { return (n_in * L + M - 1) / M; }

// The one arithmetic of the library's resamplers: R outputs, each its own chain acc = fmaf(x[idx - j], row[j], acc), j ascending.
template <int R>
__device__ __forceinline__ void resample_dot(const float* xs, const int (&idx)[R], const float* const (&rows)[R], int K, float (&acc)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int j = 0; j < K; ++j) {                       // unrolled for wider coefficient loads only: every chain keeps its order
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(xs[idx[r] - j], rows[r][j], acc[r]);
    }
}

// A row of an offline call: samples [0, len), zero outside; nothing outside is read.
struct RowSrc {
    const float* x;
    long long len;
    bool vec;                                           // x + 4k is 16-byte aligned
    __device__ __forceinline__ f4 quad(long long i) const {
        if (vec && i >= 0 && i + 3 < len) return *reinterpret_cast<const f4*>(x + i);
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (i + e >= 0 && i + e < len) ? x[i + e] : 0.f;
        return v;
    }
};
// A row of a push: local index l in [-Hs, 0) is the history, [0, m) the real samples of the chunk, everything else zero.
struct PushSrc {
    const float* hist;
    const float* chunk;
    int Hs, m;
    __device__ __forceinline__ f4 quad(long long i) const {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long l = i + e;
            v[e] = l < -(long long)Hs ? 0.f : (l < 0 ? hist[Hs + l] : (l < m ? chunk[l] : 0.f));
        }
        return v;
    }
};

// Outputs [n_begin, n_begin + count) of one row (count <= TILE) -> out[0 .. count).  The whole workgroup calls it with the same arguments.
template <int MODE, class Src>
__device__ __forceinline__ void resample_tile(const Src& src, const float* __restrict__ bank, const Geo g, long long n_begin, int count, long long delay,
                                              float* __restrict__ out, float* lds) {
    const int tid = threadIdx.x;
    float* xs = lds + g.bank_lds;
    if (MODE == MODE_BANK_LDS) {
        for (int k = tid; k < g.L * g.pitch; k += THREADS) lds[k] = bank[k];
    }
    for (int s = 0; s < count; s += g.sub) {
        const int ns = count - s < g.sub ? count - s : g.sub;
        const long long p0 = g.half + (n_begin + s - delay) * g.M;
        const long long i0 = floordiv(p0, g.L);
        const int ph0 = (int)(p0 - i0 * g.L);
        const long long lo4 = (i0 - (g.K - 1)) & ~3ll;                           // floor to a multiple of 4 (two's complement)
        const int top = (int)(i0 - lo4) + (ph0 + (ns - 1) * g.M) / g.L;         // last LDS index read
        if (s) __syncthreads();                                                 // the previous span has been consumed
        for (int q = tid; 4 * q <= top; q += THREADS) *reinterpret_cast<f4*>(xs + 4 * q) = src.quad(lo4 + 4 * q);
        __syncthreads();
        for (int d0 = 0; d0 < ns; d0 += TILE) {
            int idx[PER];
            const float* rows[PER];
            float acc[PER];
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                int d = d0 + r * THREADS + tid;
                d = d < ns ? d : ns - 1;                                         // a lane without an output repeats the last one and stores nothing
                const int q = ph0 + d * g.M;
                const int adv = MODE == MODE_L1 ? q : q / g.L;
                idx[r] = (int)(i0 - lo4) + adv;
                rows[r] = MODE == MODE_L1 ? bank : (MODE == MODE_BANK_LDS ? lds : bank) + (q - adv * g.L) * g.pitch;
            }
            resample_dot<PER>(xs, idx, rows, g.K, acc);
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int d = d0 + r * THREADS + tid;
                if (d < ns) out[s + d] = acc[r];
            }
        }
    }
}

// grid (output tile, row).  Row u: its ceil(len_u * L / M) samples, then zeros up to out_stride.
template <int MODE>
__global__ __launch_bounds__(THREADS) void resample_kernel(const float* __restrict__ x, long long in_stride, const long long* __restrict__ d_len,
                                                           const float* __restrict__ bank, Geo g, long long delay, float* __restrict__ y,
                                                           long long out_stride, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int u = blockIdx.y;
    const long long len = d_len[u];
    const long long n_out = out_len(len, g.L, g.M);
    const long long t0 = (long long)blockIdx.x * TILE;
    const int width = (int)(out_stride - t0 < TILE ? out_stride - t0 : TILE);
    long long left = n_out - t0;
    const int count = (int)(left < 0 ? 0 : (left < width ? left : width));
    float* yr = y + (size_t)u * out_stride + t0;
    if (count > 0) {
        const RowSrc src = {x + (size_t)u * in_stride, len, vec != 0};
        resample_tile<MODE>(src, bank, g, t0, count, delay, yr, lds);
    }
    for (int d = count + threadIdx.x; d < width; d += THREADS) yr[d] = 0.f;
}

// grid (output tile, row): out[u, 0 .. hop) from [history | chunk] in local indices, delay = the plan's D.
template <int MODE>
__global__ __launch_bounds__(THREADS) void resample_push_kernel(const float* __restrict__ hist, const float* __restrict__ chunk, int hop_in,
                                                                const int* __restrict__ ends, const float* __restrict__ bank, Geo g, int Hs, int D,
                                                                float* __restrict__ out, int hop) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int u = blockIdx.y;
    const int e = ends ? ends[u] : -1;
    const int m = e < 0 ? hop_in : (e < hop_in ? e : hop_in);
    const long long real = e < 0 ? hop : out_len(m, g.L, g.M);
    const int t0 = blockIdx.x * TILE;
    const int width = hop - t0 < TILE ? hop - t0 : TILE;
    long long left = real - t0;
    const int count = (int)(left < 0 ? 0 : (left < width ? left : width));
    float* yr = out + (size_t)u * hop + t0;
    if (count > 0) {
        const PushSrc src = {hist + (size_t)u * Hs, chunk + (size_t)u * hop_in, Hs, m};
        resample_tile<MODE>(src, bank, g, t0, count, D, yr, lds);
    }
    for (int d = count + threadIdx.x; d < width; d += THREADS) yr[d] = 0.f;
}

// hist[u, k] = sample hop_in - Hs + k of the chunk (zero from the row's end on): one thread per element, its own launch.
__global__ __launch_bounds__(THREADS) void resample_history_kernel(float* __restrict__ hist, const float* __restrict__ chunk, int hop_in,
                                                                   const int* __restrict__ ends, int Hs, int total) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int u = i / Hs, k = i - u * Hs;
    const int e = ends ? ends[u] : -1;
    const int m = e < 0 ? hop_in : (e < hop_in ? e : hop_in);
    const int l = hop_in - Hs + k;
    hist[i] = l < m ? chunk[(size_t)u * hop_in + l] : 0.f;
}

__global__ __launch_bounds__(THREADS) void resample_reset_kernel(float* __restrict__ hist, const int* __restrict__ mask, int Hs, int total) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    if (!mask || mask[i / Hs] != 0) hist[i] = 0.f;
}

// ---- host: plan and filter ---------------------------------------------------------------------------------------------------------
long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

int make_plan(const char* who, int rate_in, int rate_out, EgResamplePlan* p) {
    EG_REQUIRE(rate_in > 0 && rate_out > 0, EG_ERR_BAD_ARG, "%s: rate_in=%d rate_out=%d (need > 0)", who, rate_in, rate_out);
    const long long g = gcd_ll(rate_in, rate_out);
    const long long L = rate_out / g, M = rate_in / g;
    EG_REQUIRE(L <= MAX_LM && M <= MAX_LM, EG_ERR_UNSUPPORTED,
               "%s: %d Hz -> %d Hz is the ratio L=%lld / M=%lld: supported up to max(L, M) <= %d", who, rate_in, rate_out, L, M, MAX_LM);
    const int mx = (int)(L > M ? L : M);
    p->L = (int)L; p->M = (int)M;
    p->half = 10 * mx;
    p->K = (2 * p->half + 1 + p->L - 1) / p->L;
    p->D = (p->half + p->M - 1) / p->M;
    p->Hs = (int)((((long long)p->D * p->M + p->half) + L - 1) / L);
    p->pitch = p->K | 1;
    p->bank_floats = p->L * p->pitch;
    return EG_OK;
}

double bessel_i0(double x) {                            // sum_k ((x/2)^k / k!)^2
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// firwin(2*half + 1, fc, window=("kaiser", 5.0)) * L in float64.
void design(const EgResamplePlan& p, std::vector<double>& h) {
    const int n = 2 * p.half + 1;
    const double fc = 1.0 / (double)(p.L > p.M ? p.L : p.M), beta = 5.0, pi = 3.14159265358979323846;
    h.resize(n);
    const double i0b = bessel_i0(beta);
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double t = (double)(k - p.half);
        const double a = pi * (fc * t);                 // np.sinc's order: where fc * t is a whole number the tap is the rounding noise of sin, and the definition's noise is this one
        const double sinc = t == 0.0 ? 1.0 : sin(a) / a;
        const double r = t / (double)p.half;
        const double w = bessel_i0(beta * sqrt(fmax(0.0, 1.0 - r * r))) / i0b;
        h[k] = fc * sinc * w;
        sum += h[k];
    }
    for (int k = 0; k < n; ++k) h[k] = h[k] / sum * (double)p.L;
}

// LDS split and the outputs per staged span.  The bank stays in global memory when it would leave no room for a span.
int make_geo(const char* who, const EgResamplePlan& p, Geo* g) {
    g->L = p.L; g->M = p.M; g->half = p.half; g->K = p.K; g->pitch = p.pitch;
    g->bank_lds = 0;
    const int need_min = p.K + SPAN_PAD + 1 + (p.M + p.L - 1) / p.L;            // a span of at least two outputs
    if (p.L > 1) {
        const int b = (p.bank_floats + 3) / 4 * 4;
        if (b + need_min + 1024 <= LDS_FLOATS) g->bank_lds = b;
    }
    const long long cap = LDS_FLOATS - g->bank_lds;                              // span floats: ((L-1) + (sub-1)*M) / L + K + SPAN_PAD <= cap
    EG_REQUIRE(cap >= p.K + SPAN_PAD + 1, EG_ERR_UNSUPPORTED, "%s: K=%d taps per output do not fit the LDS span", who, p.K);
    long long sub = 1 + ((cap - p.K - SPAN_PAD) * p.L - (p.L - 1)) / p.M;
    g->sub = (int)(sub < 1 ? 1 : (sub > TILE ? TILE : sub));
    return EG_OK;
}
int span_floats(const Geo& g) { return (int)((((long long)g.L - 1) + (long long)(g.sub - 1) * g.M) / g.L) + g.K + SPAN_PAD; }
int mode_of(const Geo& g) { return g.L == 1 ? MODE_L1 : (g.bank_lds ? MODE_BANK_LDS : MODE_BANK_GLOBAL); }

}  // namespace

extern "C" int eg_resample_plan(int32_t rate_in, int32_t rate_out, EgResamplePlan* plan) {
    EG_REQUIRE(plan, EG_ERR_BAD_ARG, "eg_resample_plan: null plan");
    return make_plan("eg_resample_plan", rate_in, rate_out, plan);
}

extern "C" int64_t eg_resample_out_length(int64_t n_in, int32_t rate_in, int32_t rate_out) {
    EgResamplePlan p;
    if (n_in < 0 || make_plan("eg_resample_out_length", rate_in, rate_out, &p) != EG_OK) return -1;
    return out_len(n_in, p.L, p.M);
}

extern "C" int eg_resample_filter(int32_t rate_in, int32_t rate_out, float* h_taps, float* h_bank) {
    EgResamplePlan p;
    int rc = make_plan("eg_resample_filter", rate_in, rate_out, &p);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(h_taps || h_bank, EG_ERR_BAD_ARG, "eg_resample_filter: null h_taps and null h_bank");
    std::vector<double> h;
    design(p, h);
    const int n = 2 * p.half + 1;
    if (h_taps) for (int k = 0; k < n; ++k) h_taps[k] = (float)h[k];
    if (h_bank) {
        for (int ph = 0; ph < p.L; ++ph)
            for (int j = 0; j < p.pitch; ++j) {
                const long long k = ph + (long long)j * p.L;
                h_bank[ph * p.pitch + j] = (j < p.K && k < n) ? (float)h[k] : 0.f;
            }
    }
    return EG_OK;
}

extern "C" int eg_resample(const float* x, int32_t U, int64_t in_stride, const int64_t* lengths, const int64_t* d_lengths, int32_t rate_in,
                           int32_t rate_out, const float* d_bank, int64_t delay, float* y, int64_t out_stride, void* stream) {
    const char* who = "eg_resample";
    EG_REQUIRE(x, EG_ERR_BAD_ARG, "%s: null x", who);
    EG_REQUIRE(lengths, EG_ERR_BAD_ARG, "%s: null lengths", who);
    EG_REQUIRE(d_lengths, EG_ERR_BAD_ARG, "%s: null d_lengths", who);
    EG_REQUIRE(d_bank, EG_ERR_BAD_ARG, "%s: null d_bank", who);
    EG_REQUIRE(y, EG_ERR_BAD_ARG, "%s: null y", who);
    EG_REQUIRE(eg_aligned16(y) && eg_aligned16(d_bank), EG_ERR_ALIGN, "%s: y / d_bank not 16-byte aligned", who);
    EgResamplePlan p;
    int rc = make_plan(who, rate_in, rate_out, &p);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(U >= 1 && U <= MAX_U, EG_ERR_BAD_ARG, "%s: U=%d (1..%d)", who, U, MAX_U);
    EG_REQUIRE(in_stride >= 1 && in_stride < (1ll << 40), EG_ERR_BAD_ARG, "%s: in_stride=%lld (1..2^40)", who, (long long)in_stride);
    EG_REQUIRE(delay >= 0 && delay < (1ll << 31), EG_ERR_BAD_ARG, "%s: delay=%lld (0..2^31)", who, (long long)delay);
    long long max_out = 0;
    for (int u = 0; u < U; ++u) {
        EG_REQUIRE(lengths[u] >= 1 && lengths[u] <= in_stride, EG_ERR_BAD_ARG, "%s: lengths[%d]=%lld (1..in_stride=%lld)", who, u,
                   (long long)lengths[u], (long long)in_stride);
        const long long n = out_len(lengths[u], p.L, p.M);
        max_out = n > max_out ? n : max_out;
    }
    EG_REQUIRE(out_stride >= max_out, EG_ERR_BAD_ARG, "%s: out_stride=%lld < %lld output samples of the longest row", who, (long long)out_stride,
               max_out);
    const long long gx = (out_stride + TILE - 1) / TILE;
    EG_REQUIRE(gx <= 0x7fffffffll, EG_ERR_UNSUPPORTED, "%s: out_stride=%lld: grid range", who, (long long)out_stride);
    Geo g;
    rc = make_geo(who, p, &g);
    if (rc != EG_OK) return rc;
    const int vec = eg_aligned16(x) && in_stride % 4 == 0;
    const size_t lds = (size_t)(g.bank_lds + span_floats(g)) * sizeof(float);
    const dim3 grid((unsigned)gx, (unsigned)U), block(THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long* dl = reinterpret_cast<const long long*>(d_lengths);
    switch (mode_of(g)) {
        case MODE_L1: hipLaunchKernelGGL(resample_kernel<MODE_L1>, grid, block, lds, st, x, (long long)in_stride, dl, d_bank, g, (long long)delay, y, (long long)out_stride, vec); break;
        case MODE_BANK_LDS: hipLaunchKernelGGL(resample_kernel<MODE_BANK_LDS>, grid, block, lds, st, x, (long long)in_stride, dl, d_bank, g, (long long)delay, y, (long long)out_stride, vec); break;
        default: hipLaunchKernelGGL(resample_kernel<MODE_BANK_GLOBAL>, grid, block, lds, st, x, (long long)in_stride, dl, d_bank, g, (long long)delay, y, (long long)out_stride, vec); break;
    }
    return eg_check_launch("resample");
}

extern "C" int64_t eg_resample_stream_state_bytes(int32_t rows, int32_t rate_in, int32_t rate_out) {
    EgResamplePlan p;
    if (rows < 1 || rows > MAX_U || make_plan("eg_resample_stream_state_bytes", rate_in, rate_out, &p) != EG_OK) return 0;
    return eg_round_up((int64_t)rows * p.Hs * (int64_t)sizeof(float), 16);
}

extern "C" int eg_resample_stream_reset(void* state, int32_t rows, int32_t rate_in, int32_t rate_out, const int32_t* row_mask, void* stream) {
    const char* who = "eg_resample_stream_reset";
    EG_REQUIRE(state, EG_ERR_BAD_ARG, "%s: null state", who);
    EG_REQUIRE(rows >= 1 && rows <= MAX_U, EG_ERR_BAD_ARG, "%s: rows=%d (1..%d)", who, rows, MAX_U);
    EgResamplePlan p;
    int rc = make_plan(who, rate_in, rate_out, &p);
    if (rc != EG_OK) return rc;
    const int total = rows * p.Hs;
    hipLaunchKernelGGL(resample_reset_kernel, dim3((unsigned)eg_cdiv(total, THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), row_mask, p.Hs, total);
    return eg_check_launch("resample_reset");
}

extern "C" int eg_resample_stream_push(void* state, int32_t rows, int32_t rate_in, int32_t rate_out, const float* d_bank, const float* chunk_in,
                                       int32_t hop_in, const int32_t* ends_in, float* out, int32_t hop_out, void* stream) {
    const char* who = "eg_resample_stream_push";
    EG_REQUIRE(state, EG_ERR_BAD_ARG, "%s: null state", who);
    EG_REQUIRE(d_bank, EG_ERR_BAD_ARG, "%s: null d_bank", who);
    EG_REQUIRE(chunk_in, EG_ERR_BAD_ARG, "%s: null chunk_in", who);
    EG_REQUIRE(out, EG_ERR_BAD_ARG, "%s: null out", who);
    EG_REQUIRE(rows >= 1 && rows <= MAX_U, EG_ERR_BAD_ARG, "%s: rows=%d (1..%d)", who, rows, MAX_U);
    EgResamplePlan p;
    int rc = make_plan(who, rate_in, rate_out, &p);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(hop_in >= 1 && hop_out >= 1, EG_ERR_BAD_ARG, "%s: hop_in=%d hop_out=%d (need >= 1)", who, hop_in, hop_out);
    EG_REQUIRE((long long)hop_out * p.M == (long long)hop_in * p.L, EG_ERR_BAD_ARG,
               "%s: hop_in=%d is not hop_out * M / L = %d * %d / %d: a push must carry a whole number of input samples", who, hop_in, hop_out, p.M, p.L);
    EG_REQUIRE(hop_in >= p.Hs, EG_ERR_BAD_ARG, "%s: hop_in=%d < Hs=%d: the history is the last Hs samples of one chunk", who, hop_in, p.Hs);
    EG_REQUIRE((long long)rows * hop_in < (1ll << 31) && (long long)rows * hop_out < (1ll << 31), EG_ERR_UNSUPPORTED,
               "%s: rows * hop: index range (< 2^31)", who);
    Geo g;
    rc = make_geo(who, p, &g);
    if (rc != EG_OK) return rc;
    const size_t lds = (size_t)(g.bank_lds + span_floats(g)) * sizeof(float);
    const dim3 grid((unsigned)eg_cdiv(hop_out, TILE), (unsigned)rows), block(THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* hist = static_cast<float*>(state);
    switch (mode_of(g)) {
        case MODE_L1: hipLaunchKernelGGL(resample_push_kernel<MODE_L1>, grid, block, lds, st, hist, chunk_in, hop_in, ends_in, d_bank, g, p.Hs, p.D, out, hop_out); break;
        case MODE_BANK_LDS: hipLaunchKernelGGL(resample_push_kernel<MODE_BANK_LDS>, grid, block, lds, st, hist, chunk_in, hop_in, ends_in, d_bank, g, p.Hs, p.D, out, hop_out); break;
        default: hipLaunchKernelGGL(resample_push_kernel<MODE_BANK_GLOBAL>, grid, block, lds, st, hist, chunk_in, hop_in, ends_in, d_bank, g, p.Hs, p.D, out, hop_out); break;
    }
    rc = eg_check_launch("resample_push");
    if (rc != EG_OK) return rc;
    const int total = rows * p.Hs;
    hipLaunchKernelGGL(resample_history_kernel, dim3((unsigned)eg_cdiv(total, THREADS)), block, 0, st, hist, chunk_in, hop_in, ends_in, p.Hs, total);
    return eg_check_launch("resample_history");
}
