// Joint-space scores of whole tracks (include/emogest.h: eg_jointscore_tile_frames, eg_srgr_workspace_bytes, eg_srgr_tracks,
// eg_l1div_workspace_bytes, eg_l1div_tracks): the reference's SRGR and L1div (model/Beat_score_v2.py) per row of a batch of tracks.
//   SRGR   d[t, j] = (|rx - gx| + |ry - gy|) + |rz - gz|: fp32 subtractions, fp64 additions of the widened absolute values; hit = d < threshold;
//          hits[b, j] = sum_t hit;  weighted[b] = sum_t double(w[t]) * sum_j hit[t, j];  srgr = weighted * scale / (n J)
//   L1div  mean[b, c] = (sum_t double(x[t, c])) / n;  l1_sum[b] = sum_t sum_c |double(x[t, c]) - mean[b, c]|;  l1div = l1_sum / n
// There is no product of two rounded values anywhere (w * count is exact), so the file needs no contraction pragma.
// A workgroup owns TF frames of one row.  The tile is one contiguous span of the row, staged into LDS with 16-byte loads on the aligned body and
// scalar loads at its two ends (rows.h: egi_stage_exact); consecutive lanes then work on consecutive (frame, joint) or
// (run, column) items, so LDS reads are stride-3 or stride-1 (conflict-free) and the hit flags [TF][J | 1] are read along either axis without
// a conflict.  Every tile stores its partials -- fp64 sums and, for the hits, int32 [J] -- to the workspace with plain stores; a finalise launch
// adds a row's own ceil(n / TF) tiles in ascending order.  No atomics, no memset, nothing to zero: a tile past n is never read.
// SRGR with draws > 1: the takes of a recording are consecutive workgroups (draw fastest in blockIdx), so the target tile they share is fetched
// from memory once and found in cache by the others.
#include "rows.h"
#include <math.h>

namespace {

constexpr int TF = EG_JOINTSCORE_TILE_FRAMES;           // frames of one workgroup
constexpr int MAXJ = EG_SRGR_MAX_JOINTS;
constexpr int MAXD = EG_L1DIV_MAX_COLS;
constexpr int THREADS = 256;
constexpr int RUNS = 8;                                 // L1 diversity: runs of one tile; item (run, column) walks RUN frames in ascending order
constexpr int RUN = TF / RUNS;
static_assert(TF % RUNS == 0 && TF <= 64 && 64 + MAXJ <= THREADS && MAXD >= 282 && MAXD >= 3 * MAXJ, "tile constants");

// floats of a staged tile of `width` columns: TF * width elements behind a shift of up to 3, rounded up to a multiple of 4
__host__ __device__ inline int stage_floats(int width) { return (TF * width + 6) & ~3; }

// ---- SRGR -------------------------------------------------------------------------------------------------------------------------------
struct SrgrArgs {
    const float *r, *g, *w;                             // results [rows, T, J, 3], targets [rows / draws, T, J, 3], weights [rows / draws, T] or null
    const int* frames;                                  // device [rows / draws] or null
    double* part_w;                                     // workspace [rows, tiles]
    int* part_h;                                        // workspace [rows, tiles, J]
    double *srgr, *recall;                              // [rows]
    int* hits;                                          // [rows, J]
    double threshold, scale;
    int rows, T, J, draws, frame_unit, tiles;
};

// LDS, in this order: weighted frames [TF] fp64 | staged results | staged targets (stage_floats(3J) fp32 each) | hit flags [TF][J | 1] int32
inline size_t srgr_lds_bytes(int J) { return 8u * TF + 4u * (size_t)(2 * stage_floats(3 * J) + TF * (J | 1)); }

__global__ __launch_bounds__(THREADS) void srgr_tiles_kernel(const SrgrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int J = a.J, J3 = 3 * J, JP = J | 1;
    double* l_v = reinterpret_cast<double*>(lds_raw);
    float* l_r = reinterpret_cast<float*>(l_v + TF);    // TF doubles: a multiple of 16 bytes
    float* l_g = l_r + stage_floats(J3);
    int* l_hit = reinterpret_cast<int*>(l_g + stage_floats(J3));
    const int tid = threadIdx.x;
    const int draw = blockIdx.x % a.draws, ut = blockIdx.x / a.draws, tile = ut % a.tiles, u = ut / a.tiles;
    const int b = u * a.draws + draw;
    const int n = egi_valid_frames(a.frames, u, a.frame_unit, a.T);
    const int t0 = tile * TF;
    if (t0 >= n) return;                                // no frame of the row here (block-uniform): the finalise reads the row's own tiles only
    const int nt = min(TF, n - t0);                     // frames [t0, t0 + nt) of the row
    const long long rb = ((long long)b * a.T + t0) * J3, gb = ((long long)u * a.T + t0) * J3;
    const int shift_r = egi_stage_exact(l_r, a.r, rb, rb + (long long)nt * J3, tid, THREADS);
    const int shift_g = egi_stage_exact(l_g, a.g, gb, gb + (long long)nt * J3, tid, THREADS);
    __syncthreads();
    for (int i = tid; i < nt * J; i += THREADS) {       // i = t * J + j: consecutive lanes, consecutive joints
        const int t = i / J, j = i - t * J;
        const float* pr = l_r + shift_r + t * J3 + 3 * j;
        const float* pg = l_g + shift_g + t * J3 + 3 * j;
        const double dx = fabsf(pr[0] - pg[0]), dy = fabsf(pr[1] - pg[1]), dz = fabsf(pr[2] - pg[2]);
        const double d = (dx + dy) + dz;
        l_hit[t * JP + j] = d < a.threshold ? 1 : 0;    // a NaN is a miss
    }
    __syncthreads();
    if (tid < TF) {                                     // frame tid: its hit count times its weight (exact)
        double v = 0.0;
        if (tid < nt) {
            int c = 0;
            for (int j = 0; j < J; ++j) c += l_hit[tid * JP + j];
            const double w = a.w ? (double)a.w[(long long)u * a.T + t0 + tid] : 1.0;
            v = w * (double)c;
        }
        l_v[tid] = v;
    } else if (tid >= 64 && tid < 64 + J) {             // joint tid - 64: its hits in the tile
        const int j = tid - 64;
        int c = 0;
        for (int t = 0; t < nt; ++t) c += l_hit[t * JP + j];
        a.part_h[((long long)b * a.tiles + tile) * J + j] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int t = 0; t < TF; ++t) acc += l_v[t];     // ascending; a frame from nt on adds +0.0
        a.part_w[(long long)b * a.tiles + tile] = acc;
    }
}

// One workgroup of two waves per row: thread j < J adds joint j's hits over the row's tiles, thread 64 the weighted sums; then thread 64 adds
// the J counts (integers: order-free) and writes the row's two figures.
constexpr int FINAL_THREADS = 128;
static_assert(MAXJ <= 64 && FINAL_THREADS > 64, "joints in wave 0, the sums in wave 1");
__global__ __launch_bounds__(FINAL_THREADS) void srgr_final_kernel(const SrgrArgs a) {
    __shared__ int l_c[MAXJ];
    const int J = a.J, b = blockIdx.x, tid = threadIdx.x;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T);
    const int nt = (n + TF - 1) / TF;
    double acc = 0.0;
    if (tid < J) {
        const int c = egi_sum_tiles(a.part_h + (long long)b * a.tiles * J + tid, J, nt);
        a.hits[(long long)b * J + tid] = c;
        l_c[tid] = c;
    } else if (tid == 64) {
        acc = egi_sum_tiles(a.part_w + (long long)b * a.tiles, 1, nt);
    }
    __syncthreads();
    if (tid == 64) {
        long long total = 0;
        for (int j = 0; j < J; ++j) total += l_c[j];
        const double cells = (double)n * (double)J;
        a.srgr[b] = n > 0 ? acc * a.scale / cells : 0.0;
        a.recall[b] = n > 0 ? (double)total / cells : 0.0;
    }
}

// ---- L1 diversity -----------------------------------------------------------------------------------------------------------------------
struct L1Args {
    const float* x;                                     // [rows, T, D]
    const int* frames;                                  // device [rows / draws] or null
    double* part_c;                                     // workspace [rows, tiles, D]: column sums of a tile
    double* part_s;                                     // workspace [rows, tiles]: deviations of a tile
    double *mean, *l1_sum, *l1div;                      // [rows, D], [rows], [rows]
    int rows, T, D, draws, frame_unit, tiles;
};

// LDS, in this order: reduction [THREADS] fp64 | run sums [RUNS][D] fp64 | staged tile stage_floats(D) fp32
inline size_t l1_lds_bytes(int D) { return 8u * (size_t)(THREADS + RUNS * D) + 4u * (size_t)stage_floats(D); }

// DEV = false: part_c[tile, c] = sum over the tile's frames of x[t, c].  DEV = true: part_s[tile] = sum over frames and columns of |x - mean|.
// Order: item (run, c) adds its RUN frames ascending; the RUNS runs of a column ascending; (DEV) thread i adds its columns i, i + THREADS, ...
// ascending and the THREADS thread sums fold by halves -- all of it fixed by D and the constants above.
template <bool DEV>
__global__ __launch_bounds__(THREADS) void l1_tiles_kernel(const L1Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int D = a.D;
    double* l_red = reinterpret_cast<double*>(lds_raw);
    double* l_run = l_red + THREADS;
    float* l_x = reinterpret_cast<float*>(l_run + RUNS * D);       // (THREADS + RUNS * D) doubles: a multiple of 16 bytes
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % a.tiles, b = blockIdx.x / a.tiles;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T);
    const int t0 = tile * TF;
    if (t0 >= n) return;                                // block-uniform
    const int nt = min(TF, n - t0);
    const long long xb = ((long long)b * a.T + t0) * D;
    const int shift = egi_stage_exact(l_x, a.x, xb, xb + (long long)nt * D, tid, THREADS);
    __syncthreads();
    for (int i = tid; i < RUNS * D; i += THREADS) {     // i = run * D + c: consecutive lanes, consecutive columns
        const int run = i / D, c = i - run * D;
        const int f1 = min(run * RUN + RUN, nt);
        const double m = DEV ? a.mean[(long long)b * D + c] : 0.0;
        double s = 0.0;
        for (int f = run * RUN; f < f1; ++f) {
            const double v = (double)l_x[shift + f * D + c];
            s += DEV ? fabs(v - m) : v;
        }
        l_run[i] = s;
    }
    __syncthreads();
    double mine = 0.0;
    for (int c = tid; c < D; c += THREADS) {
        double acc = l_run[c];
#pragma unroll
        for (int r = 1; r < RUNS; ++r) acc += l_run[r * D + c];
        if (DEV) mine += acc;
        else a.part_c[((long long)b * a.tiles + tile) * D + c] = acc;
    }
    if (DEV) {
        l_red[tid] = mine;
        __syncthreads();
        for (int s = THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) l_red[tid] += l_red[tid + s];
            __syncthreads();
        }
        if (tid == 0) a.part_s[(long long)b * a.tiles + tile] = l_red[0];
    }
}

__global__ __launch_bounds__(THREADS) void l1_means_kernel(const L1Args a) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int D = a.D;
    if (e >= (long long)a.rows * D) return;
    const int b = (int)(e / D), c = (int)(e - (long long)b * D);
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T);
    const int nt = (n + TF - 1) / TF;
    const double acc = egi_sum_tiles(a.part_c + (long long)b * a.tiles * D + c, D, nt);
    a.mean[e] = n > 0 ? acc / (double)n : 0.0;
}

__global__ __launch_bounds__(THREADS) void l1_final_kernel(const L1Args a) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= a.rows) return;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T);
    const int nt = (n + TF - 1) / TF;
    const double acc = egi_sum_tiles(a.part_s + (long long)b * a.tiles, 1, nt);
    a.l1_sum[b] = acc;
    a.l1div[b] = n > 0 ? acc / (double)n : 0.0;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
long long tiles_of(int T) { return ((long long)T + TF - 1) / TF; }

// rows, T and the width of a frame (3J or D): the part of the shape both calls share
int check_shape(const char* who, int rows, int T, long long width) {
    EG_REQUIRE(rows >= 1, EG_ERR_BAD_ARG, "%s: rows=%d (need >= 1)", who, rows);
    EG_REQUIRE(T >= 1, EG_ERR_BAD_ARG, "%s: frames=%d (need >= 1)", who, T);
    EG_REQUIRE(tiles_of(T) * rows <= 0x7fffffffll && (long long)rows * T < (1ll << 40) / width, EG_ERR_UNSUPPORTED,
               "%s: rows=%d x frames=%d x %lld columns: grid / index range", who, rows, T, width);
    return EG_OK;
}
int check_joints(const char* who, int J) {
    EG_REQUIRE(J >= 1 && J <= MAXJ, EG_ERR_UNSUPPORTED, "%s: joints=%d (1..%d)", who, J, MAXJ);
    return EG_OK;
}
int check_cols(const char* who, int D) {
    EG_REQUIRE(D >= 1 && D <= MAXD, EG_ERR_UNSUPPORTED, "%s: columns=%d (1..%d)", who, D, MAXD);
    return EG_OK;
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline long long srgr_bytes(int rows, int T, int J) { return (8ll + 4ll * J) * rows * tiles_of(T); }
inline long long l1_bytes(int rows, int T, int D) { return 8ll * rows * tiles_of(T) * (D + 1); }

}  // namespace

extern "C" int32_t eg_jointscore_tile_frames(void) { return TF; }

extern "C" int64_t eg_srgr_workspace_bytes(int32_t rows, int32_t T, int32_t J) {
    const char* who = "eg_srgr_workspace_bytes";
    if (check_joints(who, J) != EG_OK || check_shape(who, rows, T, 3ll * J) != EG_OK) return 0;
    return srgr_bytes(rows, T, J);
}

extern "C" int eg_srgr_tracks(const float* results, const float* targets, const float* semantic, int32_t rows, int32_t T, int32_t J,
                              const int32_t* frames, const int32_t* d_frames, int32_t draws, int32_t frame_unit, double threshold, double scale,
                              void* workspace, int64_t workspace_bytes, double* srgr, double* recall, int32_t* hits, void* stream) {
    const char* who = "eg_srgr_tracks";
    EG_REQUIRE(results, EG_ERR_BAD_ARG, "%s: null results", who);
    EG_REQUIRE(targets, EG_ERR_BAD_ARG, "%s: null targets", who);
    EG_REQUIRE(workspace, EG_ERR_BAD_ARG, "%s: null workspace", who);
    EG_REQUIRE(srgr, EG_ERR_BAD_ARG, "%s: null srgr", who);
    EG_REQUIRE(recall, EG_ERR_BAD_ARG, "%s: null recall", who);
    EG_REQUIRE(hits, EG_ERR_BAD_ARG, "%s: null hits", who);
    EG_REQUIRE(eg_aligned16(results) && eg_aligned16(targets) && eg_aligned16(workspace), EG_ERR_ALIGN,
               "%s: results / targets / workspace not 16-byte aligned", who);
    EG_REQUIRE(aligned8(srgr) && aligned8(recall), EG_ERR_ALIGN, "%s: srgr / recall not 8-byte aligned", who);
    EG_REQUIRE(aligned4(hits) && aligned4(semantic), EG_ERR_ALIGN, "%s: hits / semantic not 4-byte aligned", who);
    int rc = check_joints(who, J);
    if (rc != EG_OK) return rc;
    rc = check_shape(who, rows, T, 3ll * J);
    if (rc != EG_OK) return rc;
    rc = egi_check_rows(who, rows, T, frames, d_frames, true, draws, frame_unit, 1, "1");
    if (rc != EG_OK) return rc;
    EG_REQUIRE(isfinite(threshold), EG_ERR_BAD_ARG, "%s: threshold=%g is not finite", who, threshold);
    EG_REQUIRE(isfinite(scale), EG_ERR_BAD_ARG, "%s: scale=%g is not finite", who, scale);
    const long long tiles = tiles_of(T), need = srgr_bytes(rows, T, J);
    EG_REQUIRE(workspace_bytes >= need, EG_ERR_BAD_ARG, "%s: workspace of %lld bytes, need %lld (eg_srgr_workspace_bytes)", who,
               (long long)workspace_bytes, need);
    double* part_w = static_cast<double*>(workspace);
    SrgrArgs a = {results, targets, semantic, d_frames, part_w, reinterpret_cast<int*>(part_w + (long long)rows * tiles), srgr, recall, hits,
                  threshold, scale, rows, T, J, draws, frame_unit, (int)tiles};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t smem = srgr_lds_bytes(J);
    if (int rc2 = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(srgr_tiles_kernel), smem, who)) return rc2;
    hipLaunchKernelGGL(srgr_tiles_kernel, dim3((unsigned)(tiles * rows)), dim3(THREADS), smem, st, a);
    rc = eg_check_launch("srgr_tiles");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(srgr_final_kernel, dim3((unsigned)rows), dim3(FINAL_THREADS), 0, st, a);
    return eg_check_launch("srgr_final");
}

extern "C" int64_t eg_l1div_workspace_bytes(int32_t rows, int32_t T, int32_t D) {
    const char* who = "eg_l1div_workspace_bytes";
    if (check_cols(who, D) != EG_OK || check_shape(who, rows, T, D) != EG_OK) return 0;
    return l1_bytes(rows, T, D);
}

extern "C" int eg_l1div_tracks(const float* x, int32_t rows, int32_t T, int32_t D, const int32_t* frames, const int32_t* d_frames, int32_t draws,
                               int32_t frame_unit, void* workspace, int64_t workspace_bytes, double* mean, double* l1_sum, double* l1div,
                               void* stream) {
    const char* who = "eg_l1div_tracks";
    EG_REQUIRE(x, EG_ERR_BAD_ARG, "%s: null x", who);
    EG_REQUIRE(workspace, EG_ERR_BAD_ARG, "%s: null workspace", who);
    EG_REQUIRE(mean, EG_ERR_BAD_ARG, "%s: null mean", who);
    EG_REQUIRE(l1_sum, EG_ERR_BAD_ARG, "%s: null l1_sum", who);
    EG_REQUIRE(l1div, EG_ERR_BAD_ARG, "%s: null l1div", who);
    EG_REQUIRE(eg_aligned16(x) && eg_aligned16(workspace), EG_ERR_ALIGN, "%s: x / workspace not 16-byte aligned", who);
    EG_REQUIRE(aligned8(mean) && aligned8(l1_sum) && aligned8(l1div), EG_ERR_ALIGN, "%s: mean / l1_sum / l1div not 8-byte aligned", who);
    int rc = check_cols(who, D);
    if (rc != EG_OK) return rc;
    rc = check_shape(who, rows, T, D);
    if (rc != EG_OK) return rc;
    rc = egi_check_rows(who, rows, T, frames, d_frames, true, draws, frame_unit, 1, "1");
    if (rc != EG_OK) return rc;
    const long long tiles = tiles_of(T), need = l1_bytes(rows, T, D);
    EG_REQUIRE(workspace_bytes >= need, EG_ERR_BAD_ARG, "%s: workspace of %lld bytes, need %lld (eg_l1div_workspace_bytes)", who,
               (long long)workspace_bytes, need);
    double* part_c = static_cast<double*>(workspace);
    L1Args a = {x, d_frames, part_c, part_c + (long long)rows * tiles * D, mean, l1_sum, l1div, rows, T, D, draws, frame_unit, (int)tiles};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t smem = l1_lds_bytes(D);
    if (int rc2 = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(l1_tiles_kernel<false>), smem, who)) return rc2;
    if (int rc2 = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(l1_tiles_kernel<true>), smem, who)) return rc2;
    const dim3 grid((unsigned)(tiles * rows));
    hipLaunchKernelGGL(l1_tiles_kernel<false>, grid, dim3(THREADS), smem, st, a);
    rc = eg_check_launch("l1div_sums");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(l1_means_kernel, dim3((unsigned)(((long long)rows * D + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, a);
    rc = eg_check_launch("l1div_means");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(l1_tiles_kernel<true>, grid, dim3(THREADS), smem, st, a);
    rc = eg_check_launch("l1div_deviations");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(l1_final_kernel, dim3((unsigned)((rows + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, a);
    return eg_check_launch("l1div_final");
}
