// Motion statistics of whole tracks (include/emogest.h: eg_kin_tile_frames, eg_kin_edges2, eg_kin_workspace_bytes, eg_kin_stats): per row and
// joint the mean speed, acceleration and jerk and a histogram of the speeds, from joint positions p [rows, T, J, 3] in one read.
//   d1[t] = p[t+1] - p[t], d2[t] = d1[t+1] - d1[t], d3[t] = d2[t+1] - d2[t]   in fp32, one IEEE subtraction each (no product: nothing to contract)
//   s2_k[t, j] = (x*x + y*y) + z*z of d_k[t, j] in fp64: every square of a widened fp32 is exact, so each of the two sums rounds once with or
//                without a fused multiply-add -- the file needs no contraction pragma
//   mean[b, k, j] = (sum_t sqrt(s2_k[t, j])) * fps^k / (n - k);   hist[b, j, e] += 1 for edges2[e] <= s2_1 < edges2[e+1], column B from edges2[B] on
// Stage 1: a workgroup owns TF difference indices [t0, t0 + TF) of one row and stages the frames [t0, min(t0 + TF + 3, n)) -- one contiguous
// span of the row -- into LDS with 16-byte loads on the aligned body and scalar loads at its two ends.  A tile is RUNS runs of RUN consecutive
// indices; thread i of the RUNS * J a workgroup has (rounded up to whole waves: every lane works whatever J is) owns run i / J of joint i % J
// and walks it in ascending t with d1[t], d1[t + 1] and d2[t] in registers (one LDS frame read and nine subtractions per sample), adds its
// three fp64 sums and bins its speed samples into an LDS histogram [J][B + 1] with integer LDS atomics (order-free).  The RUNS runs of a
// joint are added in ascending order and the tile's [3, J] partials stored to the workspace; the tile's non-zero bins go to
// `hist` (zeroed by a launch of its own ahead of this one) with integer atomics.  Stage 2: one thread per (row, k, j) adds the row's own
// ceil((n - 1) / TF) tile partials in ascending tile order, then scales and divides.  A row's figures depend on its own n and on TF only.
#include "rows.h"
#include <math.h>

namespace {

constexpr int TF = EG_KIN_TILE_FRAMES;                  // difference indices of one workgroup
constexpr int MAXJ = EG_KIN_MAX_JOINTS;
constexpr int MAXB = EG_KIN_MAX_BINS;
constexpr int RUNS = 16;                                // runs of one tile: RUNS * J threads (1024 at J = 64)
constexpr int RUN = TF / RUNS;                          // consecutive difference indices of one thread
constexpr int MAX_THREADS = RUNS * MAXJ;
constexpr int HALO = 3;                                 // d3[t] reads p[t .. t + 3]
static_assert(TF % RUNS == 0 && MAX_THREADS <= 1024 && MAX_THREADS % EG_WAVE == 0, "a thread owns one run of one joint");

struct Args {
    const float* p;                                     // joints [rows, T, J, 3]
    const int* frames;                                  // device [rows / draws] or null
    const double* edges2;                               // device [bins + 1]
    double* part;                                       // workspace [rows, tiles, 3, J]
    double* mean;                                       // [rows, 3, J]
    int* hist;                                          // [rows, J, bins + 1]
    double scale[3];                                    // fps, fps^2, fps^3
    int rows, T, J, bins, draws, frame_unit, tiles, top;   // top: the largest power of two <= bins
};

// LDS, in this order: edges2 [E rounded up to even] fp64 | run sums [RUNS][3][J] fp64 | staged frames [(TF + HALO) * 3J + 4 rounded up to 4]
// fp32 | histogram [J][E] int32
__host__ __device__ inline int lds_edges(int bins) { return (bins + 2) & ~1; }
__host__ __device__ inline int lds_stage(int J) { return ((TF + HALO) * 3 * J + 4 + 3) & ~3; }
inline int threads_of(int J) { return (RUNS * J + EG_WAVE - 1) / EG_WAVE * EG_WAVE; }
inline size_t lds_bytes(int J, int bins) {
    return 8u * (size_t)(lds_edges(bins) + RUNS * 3 * J) + 4u * (size_t)(lds_stage(J) + J * (bins + 1));
}

__device__ __forceinline__ double sq3(float x, float y, float z) {
    const double dx = x, dy = y, dz = z;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(MAX_THREADS) void kin_tiles_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int J = a.J, E = a.bins + 1, J3 = 3 * J;
    double* l_edges = reinterpret_cast<double*>(lds_raw);
    double* l_run = l_edges + lds_edges(a.bins);
    float* l_p = reinterpret_cast<float*>(l_run + RUNS * J3);                          // RUNS * 3J doubles: a multiple of 16 bytes
    int* l_hist = reinterpret_cast<int*>(l_p + lds_stage(J));
    const int tid = threadIdx.x, threads = blockDim.x;
    const int tile = blockIdx.x % a.tiles, b = blockIdx.x / a.tiles;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T, 4);   // the host refuses n < 4
    const int t0 = tile * TF;
    if (t0 >= n - 1) return;                            // no difference starts here (block-uniform): stage 2 reads the row's own tiles only
    const int s1 = min(t0 + TF + HALO, n);              // frames [t0, s1) of the row
    const long long g0 = ((long long)b * a.T + t0) * J3, g1 = ((long long)b * a.T + s1) * J3;
    const int shift = egi_stage_exact(l_p, a.p, g0, g1, tid, threads);                // element g of the span sits at l_p[g - (g0 & ~3)]
    for (int i = tid; i < E; i += threads) l_edges[i] = a.edges2[i];
    for (int i = tid; i < J * E; i += threads) l_hist[i] = 0;
    __syncthreads();
    if (tid < RUNS * J) {
        const int run = tid / J, j = tid - run * J;
        double s[3] = {0.0, 0.0, 0.0};
        const float* col = l_p + shift + 3 * j;         // frame f of the tile: col[f * J3 + c]
        int t = t0 + run * RUN;
        const int t_end = min(t + RUN, n - 1);
        // rolling state: the last frame read (t + 2), d1[t], d1[t + 1] and d2[t]; a frame from n on reads as 0 and only feeds sums that are
        // masked off below (every sample adds a square root or +0.0, which leaves a sum of positive terms as it is: no branch in the loop)
        auto frame = [&](int f, float* v) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = f < s1 ? col[(f - t0) * J3 + c] : 0.f;
        };
        float p0[3], p1[3], pl[3], d1a[3], d1b[3], d2a[3];
        frame(t, p0);
        frame(t + 1, p1);
        frame(t + 2, pl);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            d1a[c] = p1[c] - p0[c];
            d1b[c] = pl[c] - p1[c];
            d2a[c] = d1b[c] - d1a[c];
        }
        for (; t < t_end; ++t) {
            float pn[3], d1c[3], d2b[3], d3[3];
            frame(t + 3, pn);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d1c[c] = pn[c] - pl[c];
                d2b[c] = d1c[c] - d1b[c];
                d3[c] = d2b[c] - d2a[c];
            }
            const double v = sq3(d1a[0], d1a[1], d1a[2]);
            const double r2 = sqrt(sq3(d2a[0], d2a[1], d2a[2])), r3 = sqrt(sq3(d3[0], d3[1], d3[2]));
            s[0] += sqrt(v);
            s[1] += t < n - 2 ? r2 : 0.0;
            s[2] += t < n - 3 ? r3 : 0.0;
            int pos = 0;                                // the last edge that is not above v (edges2[0] = 0; a NaN sample: the overflow column)
            for (int st = a.top; st > 0; st >>= 1) {    // a.top: the largest power of two <= bins (wave-uniform trip count, no branch inside)
                const int e = pos + st;
                const double edge = l_edges[min(e, a.bins)];
                pos = (e <= a.bins && !(v < edge)) ? e : pos;
            }
            atomicAdd(&l_hist[j * E + pos], 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d1a[c] = d1b[c];
                d1b[c] = d1c[c];
                d2a[c] = d2b[c];
                pl[c] = pn[c];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) l_run[(run * 3 + k) * J + j] = s[k];
    }
    __syncthreads();
    for (int i = tid; i < J3; i += threads) {           // i = k * J + j
        double acc = l_run[i];
#pragma unroll
        for (int r = 1; r < RUNS; ++r) acc += l_run[r * J3 + i];
        a.part[((long long)b * a.tiles + tile) * J3 + i] = acc;
    }
    int* h = a.hist + (long long)b * J * E;
    for (int i = tid; i < J * E; i += threads) {
        const int c = l_hist[i];
        if (c != 0) atomicAdd(h + i, c);
    }
}

// hist = 0 ahead of stage 1, as a launch: a memset node of this size came back with other values from the second replay of a captured graph on.
__global__ __launch_bounds__(256) void kin_zero_kernel(int* __restrict__ hist, long long count) {
    const long long q = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (q + 4 <= count) {
        *reinterpret_cast<f4*>(hist + q) = f4{0.f, 0.f, 0.f, 0.f};
    } else {
        for (long long e = q; e < count; ++e) hist[e] = 0;
    }
}

__global__ __launch_bounds__(256) void kin_means_kernel(const Args a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int J = a.J, J3 = 3 * J;
    if (e >= (long long)a.rows * J3) return;
    const int b = (int)(e / J3), i = (int)(e - (long long)b * J3), k = i / J;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T, 4);
    double m = 0.0;
    if (n >= 4) {
        const int nt = (n - 1 + TF - 1) / TF;
        m = egi_sum_tiles(a.part + (long long)b * a.tiles * J3 + i, J3, nt) * a.scale[k] / (double)(n - 1 - k);
    }
    a.mean[e] = m;
}

long long tiles_of(int T) { return ((long long)T - 1 + TF - 1) / TF; }

int check_shape(const char* who, int rows, int T, int J, int bins) {
    EG_REQUIRE(rows >= 1, EG_ERR_BAD_ARG, "%s: rows=%d (need >= 1)", who, rows);
    EG_REQUIRE(T >= 4, EG_ERR_BAD_ARG, "%s: frames=%d (need >= 4: the jerk reads four positions)", who, T);
    EG_REQUIRE(J >= 1 && J <= MAXJ, EG_ERR_UNSUPPORTED, "%s: joints=%d (1..%d)", who, J, MAXJ);
    EG_REQUIRE(bins >= 1 && bins <= MAXB, EG_ERR_UNSUPPORTED, "%s: bins=%d (1..%d)", who, bins, MAXB);
    EG_REQUIRE(tiles_of(T) * rows <= 0x7fffffffll && (long long)rows * T * J * 3 < (1ll << 40), EG_ERR_UNSUPPORTED,
               "%s: rows=%d x frames=%d x joints=%d: grid / index range", who, rows, T, J);
    return EG_OK;
}

}  // namespace

extern "C" int32_t eg_kin_tile_frames(void) { return TF; }

extern "C" int eg_kin_edges2(const double* edges, int32_t n_edges, double fps, double* edges2) {
    const char* who = "eg_kin_edges2";
    EG_REQUIRE(edges && edges2, EG_ERR_BAD_ARG, "%s: null edges / edges2", who);
    EG_REQUIRE(n_edges >= 2 && n_edges <= MAXB + 1, EG_ERR_BAD_ARG, "%s: n_edges=%d (2..%d: 1..%d bins)", who, n_edges, MAXB + 1, MAXB);
    EG_REQUIRE(isfinite(fps) && fps > 0.0, EG_ERR_BAD_ARG, "%s: fps=%g (finite and > 0)", who, fps);
    for (int e = 0; e < n_edges; ++e) EG_REQUIRE(isfinite(edges[e]), EG_ERR_BAD_ARG, "%s: edges[%d]=%g is not finite", who, e, edges[e]);
    EG_REQUIRE(edges[0] == 0.0, EG_ERR_BAD_ARG, "%s: edges[0]=%g (the first bin starts at 0 m/s)", who, edges[0]);
    for (int e = 1; e < n_edges; ++e)
        EG_REQUIRE(edges[e] > edges[e - 1], EG_ERR_BAD_ARG, "%s: edges[%d]=%g <= edges[%d]=%g (strictly ascending)", who, e, edges[e], e - 1, edges[e - 1]);
    for (int e = 0; e < n_edges; ++e) {
        const double q = edges[e] / fps;
        edges2[e] = q * q;
    }
    return EG_OK;
}

extern "C" int64_t eg_kin_workspace_bytes(int32_t rows, int32_t T, int32_t J, int32_t bins) {
    if (check_shape("eg_kin_workspace_bytes", rows, T, J, bins) != EG_OK) return 0;
    return 8ll * rows * tiles_of(T) * 3 * J;
}

extern "C" int eg_kin_stats(const float* joints, int32_t rows, int32_t T, int32_t J, const int32_t* frames, const int32_t* d_frames, int32_t draws,
                            int32_t frame_unit, double fps, const double* d_edges2, int32_t bins, void* workspace, int64_t workspace_bytes,
                            double* mean, int32_t* hist, void* stream) {
    const char* who = "eg_kin_stats";
    EG_REQUIRE(joints, EG_ERR_BAD_ARG, "%s: null joints", who);
    EG_REQUIRE(d_edges2, EG_ERR_BAD_ARG, "%s: null d_edges2", who);
    EG_REQUIRE(workspace, EG_ERR_BAD_ARG, "%s: null workspace", who);
    EG_REQUIRE(mean, EG_ERR_BAD_ARG, "%s: null mean", who);
    EG_REQUIRE(hist, EG_ERR_BAD_ARG, "%s: null hist", who);
    EG_REQUIRE(eg_aligned16(joints) && eg_aligned16(workspace) && eg_aligned16(mean) && eg_aligned16(hist), EG_ERR_ALIGN,
               "%s: joints / workspace / mean / hist not 16-byte aligned", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_edges2) & 7u) == 0, EG_ERR_ALIGN, "%s: d_edges2 not 8-byte aligned", who);
    int rc = check_shape(who, rows, T, J, bins);
    if (rc != EG_OK) return rc;
    rc = egi_check_rows(who, rows, T, nullptr, d_frames, false, draws, frame_unit, 0, "");
    if (rc != EG_OK) return rc;
    EG_REQUIRE(isfinite(fps) && fps > 0.0, EG_ERR_BAD_ARG, "%s: fps=%g (finite and > 0)", who, fps);
    rc = egi_check_rows(who, rows, T, frames, d_frames, true, draws, frame_unit, 4, "4 (the jerk reads four positions)");
    if (rc != EG_OK) return rc;
    const long long tiles = tiles_of(T), need = 8ll * rows * tiles * 3 * J;
    EG_REQUIRE(workspace_bytes >= need, EG_ERR_BAD_ARG, "%s: workspace of %lld bytes, need %lld (eg_kin_workspace_bytes)", who,
               (long long)workspace_bytes, need);
    int top = 1;
    while (2 * top <= bins) top *= 2;
    Args a = {joints, d_frames, d_edges2, static_cast<double*>(workspace), mean, hist, {fps, fps * fps, fps * fps * fps}, rows, T, J, bins, draws,
              frame_unit, (int)tiles, top};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t smem = lds_bytes(J, bins);
    if (int rc2 = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(kin_tiles_kernel), smem, who)) return rc2;
    const long long cells = (long long)rows * J * (bins + 1);
    hipLaunchKernelGGL(kin_zero_kernel, dim3((unsigned)((cells + 1023) / 1024)), dim3(256), 0, st, hist, cells);
    rc = eg_check_launch("kin_zero");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(kin_tiles_kernel, dim3((unsigned)(tiles * rows)), dim3(threads_of(J)), smem, st, a);
    rc = eg_check_launch("kin_tiles");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(kin_means_kernel, dim3((unsigned)(((long long)rows * 3 * J + 255) / 256)), dim3(256), 0, st, a);
    return eg_check_launch("kin_means");
}
