// Smoothed output (include/emogest.h: eg_smooth_design, eg_smooth_tile_frames, eg_smooth_tile_cols, eg_smooth_tracks, eg_smooth_stream_*):
// a Savitzky-Golay filter along the time axis of whole gesture tracks.  One table C[K][K]: row i gives the d-th derivative at window position
// i of the least-squares polynomial through K samples.  For a row with n >= K valid frames
//   head      i < half:            y[i] = sum_j C[i][j] x[j]
//   interior  half <= i < n-half:  y[i] = sum_j C[half][j] x[i - half + j]
//   tail      i >= n - half:       y[i] = sum_j C[K - (n - i)][j] x[n - K + j]
// and zeros from frame n on: scipy.signal.savgol_filter(mode="interp").  Every output element is smooth_element: acc = 0, then
// acc = fmaf(c[j], x[j], acc) for j = 0 .. K-1 -- the offline kernel, the stream's push and its tail all call it, so they agree bit for bit.
// The offline kernel is a memory-bound stream.  A workgroup owns TF frames x TC columns of one row: it stages the frames it needs (the tile,
// half a window on either side, and for a tile that holds tail frames the row's last K frames) through LDS with 16-byte loads -- a frame's
// column segment starts on any float (D is no multiple of 4), so every staged frame keeps its own shift of 0..3 floats --, then lane = column
// and every wave takes FR consecutive frames: a thread reads K + FR - 1 values of its column into registers once and makes FR outputs from
// them ((K + FR - 1) / FR LDS reads per output instead of K), with the centre row of the table in scalar registers (K is a template argument,
// so the window is indexed at compile time).  A tile with its whole halo staged reads through four addresses (the shift has period 4 in the
// frame index) and immediate offsets; a row's first and last tiles clamp every read into the staged range.  The at most K - 1 head and tail frames of a row read their window from LDS term by term with a
// wave-uniform table row.  Consecutive lanes hold consecutive columns: LDS and global accesses are conflict-free and coalesced.  One owning
// thread per output element, plain vector stores, no atomics; the grid depends on (rows, T, D) only.
#include "rows.h"
#include <math.h>

// The arithmetic of one output element: c(j) the j-th weight, x(j) the j-th sample of the window.
template <class CF, class XF>
__device__ __forceinline__ float smooth_element(const int K, CF c, XF x) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) acc = fmaf(c(j), x(j), acc);
    return acc;
}

namespace {

constexpr int MAXK = EG_SMOOTH_MAX_WINDOW;
constexpr int TF = EG_SMOOTH_TILE_FRAMES;               // frames of one workgroup
constexpr int TC = EG_SMOOTH_TILE_COLS;                 // columns of one workgroup: one per lane
constexpr int WAVES = 4;
constexpr int THREADS = WAVES * EG_WAVE;
constexpr int FR = TF / WAVES;                          // consecutive frames of one thread
constexpr int PITCH = TC + 4;                           // LDS floats per staged frame: TC columns behind a shift of 0..3, whole quads
static_assert(TC == EG_WAVE && TF % WAVES == 0 && PITCH % 4 == 0, "lane = column; a wave owns FR frames; staged frames start on a quad");

struct Args {
    const float* src;                                   // track [B, T, D]
    const float* table;                                 // device fp32 [K][K]
    const int* frames;                                  // device [B / draws] or null
    float* dst;
    int B, T, D, draws, frame_unit, ftiles, ctiles;
};

template <int K>
__global__ __launch_bounds__(THREADS) void smooth_tracks_kernel(const Args a) {
    constexpr int HALF = K / 2;
    constexpr int SLOTS = TF + 2 * HALF;                // staged frames at most (a tile that reaches down to n - K holds exactly K)
    __shared__ __attribute__((aligned(16))) float lds[SLOTS * PITCH];
    const int tid = threadIdx.x, lane = tid & (EG_WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / EG_WAVE);
    const int D = a.D;
    int blk = blockIdx.x;                               // column tiles fastest: neighbours share cache lines
    const int ct = blk % a.ctiles; blk /= a.ctiles;
    const int ft = blk % a.ftiles, b = blk / a.ftiles;
    const int c0 = ct * TC, w = min(TC, D - c0);
    const int k0 = ft * TF, cnt = min(TF, a.T - k0);
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T, K);    // the host refuses n < K
    const int live = max(0, min(cnt, n - k0));
    const long long row0 = (long long)b * a.T * D;
    const int col = lane;
    const bool own = col < w;
    if (live > 0) {
        // frames [s0, s1) of the row, columns [c0, c0 + w): frame s at lds[(s - s0) * PITCH + shift(s) + col]
        const int s0 = max(0, min(k0 - HALF, n - K)), s1 = min(n, k0 + TF + HALF);
        const long long total = (long long)a.B * a.T * D;
        for (int s = s0 + tid / 32; s < s1; s += THREADS / 32) {
            const long long g = row0 + (long long)s * D + c0, lo4 = g & ~3ll;
            const long long q = lo4 + 4 * (tid & 31);
            if (q < g + w) {
                f4 v;
                if (q + 3 < total) {
                    v = *reinterpret_cast<const f4*>(a.src + q);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = q + e < total ? a.src[q + e] : 0.f;
                }
                *reinterpret_cast<f4*>(lds + (s - s0) * PITCH + 4 * (tid & 31)) = v;
            }
        }
        __syncthreads();
        const int nslots = s1 - s0;
        const int sh0 = (int)((row0 + c0) & 3), dD = D & 3;
        auto at = [&](int s) -> const float* {          // frame s, clamped into the staged range (a clamped frame feeds no output that is kept)
            const int sl = min(max(s - s0, 0), nslots - 1);
            return lds + sl * PITCH + ((sh0 + (s0 + sl) * dD) & 3) + col;
        };
        const int f0 = k0 + wave * FR;                  // this wave's frames [f0, f0 + FR)
        if (f0 < k0 + live) {
            // the centre row, read once and held in scalar registers: read inside the loop below it would be fetched again behind every store
            // (the output may alias the table as far as the compiler knows), K vector loads per frame
            float cc[K];
#pragma unroll
            for (int j = 0; j < K; ++j)
                cc[j] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.table[HALF * K + j])));
            float r[K + FR - 1];
            if (s0 == k0 - HALF && s1 == k0 + TF + HALF) {
                // a tile with its whole halo staged: no frame needs the clamp, and the shift has period 4 in the frame index, so four
                // addresses and the read's immediate offset serve every read
                const int slot0 = wave * FR, sb = sh0 + (s0 + slot0) * dD;
                const float* p4[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) p4[q] = lds + slot0 * PITCH + ((sb + q * dD) & 3) + col;
#pragma unroll
                for (int m = 0; m < K + FR - 1; ++m) r[m] = p4[m & 3][m * PITCH];
            } else {
#pragma unroll
                for (int m = 0; m < K + FR - 1; ++m) r[m] = *at(f0 - HALF + m);
            }
            const int i_end = min(f0 + FR, k0 + live);
#pragma unroll
            for (int f = 0; f < FR; ++f) {              // the interior frames, from the register window
                const int i = f0 + f;
                if (i >= HALF && i < min(i_end, n - HALF)) {
                    const float y = smooth_element(K, [&](int j) { return cc[j]; }, [&](int j) { return r[f + j]; });
                    if (own) a.dst[row0 + (long long)i * D + c0 + col] = y;
                }
            }
#pragma unroll 1
            for (int i = f0; i < i_end; ++i) {          // head and tail frames: their own table row on the row's first / last K frames
                if (i >= HALF && i < n - HALF) continue;
                const int trow = i < HALF ? i : K - (n - i), x0 = i < HALF ? 0 : n - K;
                const float* __restrict__ ce = a.table + __builtin_amdgcn_readfirstlane(trow) * K;
                const float y = smooth_element(K, [&](int j) { return ce[j]; }, [&](int j) { return *at(x0 + j); });
                if (own) a.dst[row0 + (long long)i * D + c0 + col] = y;
            }
        }
    }
    if (own)
        for (int i = k0 + live + wave; i < k0 + cnt; i += WAVES) a.dst[row0 + (long long)i * D + c0 + col] = 0.f;
}

// ---- stream -----------------------------------------------------------------------------------------------------------------------------
// state: history [rows][K - 1][D] fp32 | count [rows] int32 (valid steps so far).
struct SArgs {
    float* hist;
    int* count;
    const float* table;
    const float* chunk;                                 // push: the step's rows [rows, H, D]; tail: the tail rows [rows, P, D]
    const int* valid;                                   // device int32 [rows] or null (all valid)
    float* out;
    int rows, H, D, K;
};

// out [rows, H, D]: for a valid row in its s-th valid step the smoothed frames [sH - half, (s + 1)H - half) of its track.  In local indices
// W = [history (K - 1) | chunk (H)]: output o is frame sH - half + o, an interior frame reads W[o .. o + K).
__global__ __launch_bounds__(256) void smooth_push_kernel(const SArgs a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int D = a.D, K = a.K, half = K / 2, HD = a.H * D;
    if (e >= (long long)a.rows * HD) return;
    const int u = (int)(e / HD), rem = (int)(e - (long long)u * HD), o = rem / D, c = rem - o * D;
    float y = 0.f;
    if (!a.valid || a.valid[u] != 0) {
        const float* hs = a.hist + (long long)u * (K - 1) * D + c;
        const float* ch = a.chunk + (long long)u * HD + c;
        const bool first = a.count[u] == 0;
        const int i = o - half;                         // the frame, in a first step
        if (!first || i >= half) {
            const float* __restrict__ cc = a.table + half * K;
            y = smooth_element(K, [&](int j) { return cc[j]; },
                               [&](int j) { const int l = o + j; return l < K - 1 ? hs[(long long)l * D] : ch[(long long)(l - (K - 1)) * D]; });
        } else if (i >= 0) {                            // head: x[0 .. K) is the start of the first chunk (K <= H)
            const float* __restrict__ ce = a.table + i * K;
            y = smooth_element(K, [&](int j) { return ce[j]; }, [&](int j) { return ch[(long long)j * D]; });
        }
    }
    a.out[e] = y;
}

// The new history (the last K - 1 rows of the chunk: K <= H) and the count, for the valid rows: a launch of its own.
__global__ __launch_bounds__(256) void smooth_state_kernel(const SArgs a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int D = a.D, K = a.K, KD = (K - 1) * D;
    if (e >= (long long)a.rows * KD) return;
    const int u = (int)(e / KD), rem = (int)(e - (long long)u * KD);
    if (a.valid && a.valid[u] == 0) return;
    a.hist[e] = a.chunk[((long long)u * a.H + (a.H - (K - 1))) * D + rem];
    if (rem == 0) a.count[u] += 1;
}

__global__ __launch_bounds__(256) void smooth_reset_kernel(const SArgs a) {         // a.valid: the row mask
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int KD = (a.K - 1) * a.D;
    if (e >= (long long)a.rows * KD) return;
    const int u = (int)(e / KD);
    if (a.valid && a.valid[u] == 0) return;
    a.hist[e] = 0.f;
    if (e - (long long)u * KD == 0) a.count[u] = 0;
}

// out [rows, P + half, D]: the last P + half smoothed frames of every row's track, whose last P raw frames are chunk [rows, P, D] (a.H = P).
// W = [history (K - 1) | tail (P)]: output o < P is interior and reads W[o .. o + K); o >= P is tail frame n - (P + half - o) and reads the
// last K, W[P - 1 .. P - 1 + K).  A row without a valid step has no track of K frames: zeros.
__global__ __launch_bounds__(256) void smooth_tail_kernel(const SArgs a) {
    const int D = a.D, K = a.K, half = K / 2, P = a.H, OD = (P + half) * D;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)a.rows * OD) return;
    const int u = (int)(e / OD), rem = (int)(e - (long long)u * OD), o = rem / D, c = rem - o * D;
    float y = 0.f;
    if (a.count[u] > 0) {
        const float* hs = a.hist + (long long)u * (K - 1) * D + c;
        const float* ch = a.chunk + (long long)u * P * D + c;
        const int trow = o < P ? half : K - (P + half - o), base = o < P ? o : P - 1;
        const float* __restrict__ ct = a.table + trow * K;
        y = smooth_element(K, [&](int j) { return ct[j]; },
                           [&](int j) { const int l = base + j; return l < K - 1 ? hs[(long long)l * D] : ch[(long long)(l - (K - 1)) * D]; });
    }
    a.out[e] = y;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
int check_window(const char* who, int K) {
    EG_REQUIRE(K >= 3 && K <= MAXK, EG_ERR_UNSUPPORTED, "%s: window=%d (odd, 3..%d)", who, K, MAXK);
    EG_REQUIRE(K % 2 == 1, EG_ERR_BAD_ARG, "%s: window=%d is even (a Savitzky-Golay window is centred on a frame: odd, 3..%d)", who, K, MAXK);
    return EG_OK;
}

int check_design(const char* who, int K, int p, int d, double delta) {
    int rc = check_window(who, K);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(p >= 1 && p <= 5 && p <= K - 1, EG_ERR_BAD_ARG, "%s: polyorder=%d (1..min(5, window - 1) = %d)", who, p, K - 1 < 5 ? K - 1 : 5);
    EG_REQUIRE(d >= 0 && d <= 2, EG_ERR_BAD_ARG, "%s: deriv=%d (0..2)", who, d);
    EG_REQUIRE(d <= p, EG_ERR_BAD_ARG, "%s: deriv=%d > polyorder=%d (the derivative of the fitted polynomial would be zero)", who, d, p);
    EG_REQUIRE(isfinite(delta) && delta > 0.0, EG_ERR_BAD_ARG, "%s: delta=%g (the frame spacing 1 / fps: finite and > 0)", who, delta);
    return EG_OK;
}

int stream_checks(const char* who, const void* state, int rows, int D, int K) {
    EG_REQUIRE(state, EG_ERR_BAD_ARG, "%s: null state", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(state) & 3u) == 0, EG_ERR_ALIGN, "%s: state not 4-byte aligned", who);
    int rc = check_window(who, K);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(rows >= 1 && D >= 1, EG_ERR_BAD_ARG, "%s: rows=%d D=%d (need >= 1)", who, rows, D);
    EG_REQUIRE((long long)rows * (MAXK - 1) * D < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: rows=%d x D=%d: index range", who, rows, D);
    return EG_OK;
}

SArgs stream_args(void* state, int rows, int H, int D, int K, const float* table, const float* chunk, const int* valid, float* out) {
    float* hist = static_cast<float*>(state);
    return {hist, reinterpret_cast<int*>(hist + (long long)rows * (K - 1) * D), table, chunk, valid, out, rows, H, D, K};
}

int launch_elems(void (*kernel)(SArgs), const SArgs& a, long long elems, void* stream, const char* what) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return eg_check_launch(what);
}

}  // namespace

extern "C" int32_t eg_smooth_tile_frames(void) { return TF; }
extern "C" int32_t eg_smooth_tile_cols(void) { return TC; }

extern "C" int eg_smooth_design(int32_t K, int32_t p, int32_t d, double delta, double* table64, float* table32) {
#pragma clang fp contract(off)
    const char* who = "eg_smooth_design";
    int rc = check_design(who, K, p, d, delta);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(table64 || table32, EG_ERR_BAD_ARG, "%s: null table64 and table32", who);
    const int half = K / 2, m = p + 1;
    // A[j][q] = t_j^q with t_j = j - half (centred), A = Q R by modified Gram-Schmidt, every column orthogonalised twice
    double Q[MAXK][6], R[6][6] = {};
    for (int q = 0; q < m; ++q) {
        double v[MAXK];
        for (int j = 0; j < K; ++j) v[j] = pow((double)(j - half), q);
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < q; ++s) {
                double dot = 0.0;
                for (int j = 0; j < K; ++j) dot += Q[j][s] * v[j];
                for (int j = 0; j < K; ++j) v[j] -= dot * Q[j][s];
                R[s][q] += dot;
            }
        double nrm = 0.0;
        for (int j = 0; j < K; ++j) nrm += v[j] * v[j];
        nrm = sqrt(nrm);
        R[q][q] = nrm;
        for (int j = 0; j < K; ++j) Q[j][q] = v[j] / nrm;
    }
    // the polynomial's coefficients are a = R^-1 Q^T x; its d-th derivative at t_i is g_i . a with g_i[q] = q! / (q - d)! t_i^(q - d) / delta^d,
    // so row i of the table is Q z with R^T z = g_i
    const double scale = pow(delta, -(double)d);
    for (int i = 0; i < K; ++i) {
        const double t = (double)(i - half);
        double g[6], z[6];
        for (int q = 0; q < m; ++q) {
            double f = 1.0;
            for (int s = 0; s < d; ++s) f *= (double)(q - s);
            g[q] = q < d ? 0.0 : f * pow(t, q - d) * scale;
        }
        for (int q = 0; q < m; ++q) {
            double s = g[q];
            for (int r = 0; r < q; ++r) s -= R[r][q] * z[r];
            z[q] = s / R[q][q];
        }
        for (int j = 0; j < K; ++j) {
            double c = 0.0;
            for (int q = 0; q < m; ++q) c += Q[j][q] * z[q];
            if (table64) table64[i * K + j] = c;
            if (table32) table32[i * K + j] = (float)c;
        }
    }
    return EG_OK;
}

extern "C" int eg_smooth_tracks(const float* track, int32_t rows, int32_t T, int32_t D, int32_t K, const float* d_table, const int32_t* frames,
                                const int32_t* d_frames, int32_t draws, int32_t frame_unit, float* out, void* stream) {
    const char* who = "eg_smooth_tracks";
    EG_REQUIRE(track, EG_ERR_BAD_ARG, "%s: null track", who);
    EG_REQUIRE(out, EG_ERR_BAD_ARG, "%s: null out", who);
    EG_REQUIRE(d_table, EG_ERR_BAD_ARG, "%s: null d_table", who);
    EG_REQUIRE(eg_aligned16(track) && eg_aligned16(out) && eg_aligned16(d_table), EG_ERR_ALIGN, "%s: track / out / d_table not 16-byte aligned", who);
    EG_REQUIRE(rows >= 1 && T >= 1 && D >= 1, EG_ERR_BAD_ARG, "%s: rows=%d frames=%d columns=%d (need >= 1)", who, rows, T, D);
    int rc = egi_check_rows(who, rows, T, nullptr, d_frames, false, draws, frame_unit, 0, "");
    if (rc != EG_OK) return rc;
    rc = check_window(who, K);
    if (rc != EG_OK) return rc;
    const long long elems = (long long)rows * T * D;
    const long long ftiles = ((long long)T + TF - 1) / TF, ctiles = ((long long)D + TC - 1) / TC;
    EG_REQUIRE(ftiles * ctiles * rows <= 0x7fffffffll && elems < (1ll << 40), EG_ERR_UNSUPPORTED, "%s: rows=%d x frames=%d x columns=%d: grid / index range",
               who, rows, T, D);
    {
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(track), y0 = reinterpret_cast<uintptr_t>(out), nb = (uintptr_t)elems * 4u;
        EG_REQUIRE(x0 + nb <= y0 || y0 + nb <= x0, EG_ERR_BAD_ARG, "%s: out overlaps track (every output reads %d input frames: not in place)", who, K);
    }
    char why[64];
    snprintf(why, sizeof why, "window=%d (there is no shrinking window)", K);
    rc = egi_check_rows(who, rows, T, frames, d_frames, true, draws, frame_unit, K, why);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(frames || T >= K, EG_ERR_BAD_ARG, "%s: frames=%d < window=%d (there is no shrinking window)", who, T, K);
    const Args a = {track, d_table, d_frames, out, rows, T, D, draws, frame_unit, (int)ftiles, (int)ctiles};
    const dim3 grid((unsigned)(ftiles * ctiles * rows));
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (K) {
#define EG_SMOOTH_CASE(KK) case KK: hipLaunchKernelGGL(smooth_tracks_kernel<KK>, grid, dim3(THREADS), 0, st, a); break;
        EG_SMOOTH_CASE(3) EG_SMOOTH_CASE(5) EG_SMOOTH_CASE(7) EG_SMOOTH_CASE(9) EG_SMOOTH_CASE(11) EG_SMOOTH_CASE(13) EG_SMOOTH_CASE(15)
        EG_SMOOTH_CASE(17) EG_SMOOTH_CASE(19) EG_SMOOTH_CASE(21) EG_SMOOTH_CASE(23) EG_SMOOTH_CASE(25) EG_SMOOTH_CASE(27) EG_SMOOTH_CASE(29)
        EG_SMOOTH_CASE(31)
#undef EG_SMOOTH_CASE
    }
    return eg_check_launch("smooth_tracks");
}

extern "C" int64_t eg_smooth_stream_state_bytes(int32_t rows, int32_t D, int32_t K) {
    if (check_window("eg_smooth_stream_state_bytes", K) != EG_OK) return 0;
    if (rows < 1 || D < 1) {
        eg_set_error("eg_smooth_stream_state_bytes: rows=%d D=%d (need >= 1)", rows, D);
        return 0;
    }
    return 4ll * ((long long)rows * (K - 1) * D + rows);
}

extern "C" int eg_smooth_stream_reset(void* state, int32_t rows, int32_t D, int32_t K, const int32_t* row_mask, void* stream) {
    const char* who = "eg_smooth_stream_reset";
    int rc = stream_checks(who, state, rows, D, K);
    if (rc != EG_OK) return rc;
    const SArgs a = stream_args(state, rows, 0, D, K, nullptr, nullptr, row_mask, nullptr);
    return launch_elems(smooth_reset_kernel, a, (long long)rows * (K - 1) * D, stream, "smooth_stream_reset");
}

extern "C" int eg_smooth_stream_push(void* state, int32_t rows, int32_t H, int32_t D, int32_t K, const float* d_table, const float* chunk,
                                     const int32_t* d_valid, float* out, void* stream) {
    const char* who = "eg_smooth_stream_push";
    int rc = stream_checks(who, state, rows, D, K);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(d_table && chunk && out, EG_ERR_BAD_ARG, "%s: null d_table / chunk / out", who);
    EG_REQUIRE(H >= K, EG_ERR_BAD_ARG, "%s: window=%d > H=%d frames per step (the head rows need x[0 .. window) inside the first chunk)", who, K, H);
    EG_REQUIRE((long long)rows * H * D < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: rows=%d x H=%d x D=%d: index range", who, rows, H, D);
    const SArgs a = stream_args(state, rows, H, D, K, d_table, chunk, d_valid, out);
    rc = launch_elems(smooth_push_kernel, a, (long long)rows * H * D, stream, "smooth_stream_push");
    if (rc != EG_OK) return rc;
    return launch_elems(smooth_state_kernel, a, (long long)rows * (K - 1) * D, stream, "smooth_stream_state");
}

extern "C" int eg_smooth_stream_tail(const void* state, int32_t rows, int32_t P, int32_t D, int32_t K, const float* d_table, const float* tail_rows,
                                     float* out, void* stream) {
    const char* who = "eg_smooth_stream_tail";
    int rc = stream_checks(who, state, rows, D, K);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(d_table && tail_rows && out, EG_ERR_BAD_ARG, "%s: null d_table / tail_rows / out", who);
    EG_REQUIRE(P >= 1, EG_ERR_BAD_ARG, "%s: P=%d tail rows (need >= 1: the last window of a track reaches one frame behind the history)", who, P);
    EG_REQUIRE((long long)rows * (P + K / 2) * D < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: rows=%d x P=%d x D=%d: index range", who, rows, P, D);
    const SArgs a = stream_args(const_cast<void*>(state), rows, P, D, K, d_table, tail_rows, nullptr, out);
    return launch_elems(smooth_tail_kernel, a, (long long)rows * (P + K / 2) * D, stream, "smooth_stream_tail");
}
