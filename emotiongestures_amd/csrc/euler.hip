// The Euler filter (include/emogest.h: eg_angle_unwrap_workspace_bytes, eg_angle_unwrap): whole-period jumps taken out of angle tracks
// [rows, T, C] in place, every (row, column) a series of its own.
//   d_t = p_t - p_(t-1) in fp32;  k_t = nearbyint((double)d_t / P), k_0 = 0;  c_t = k_0 + .. + k_t (an integer);  out_t = fmaf(-(float)c_t, (float)P, p_t).
// The counts are integers, so the result does not depend on the tiling.  A tile is UT frames of a row; a thread owns one column of it and walks
// its frames in order with the frame before in a register.  Up to three launches:
//   totals   per tile and column: the sum of k_t over the tile's frames, and k of the tile's first frame on its own (that one reads the last
//            frame of the tile before from memory -- the only read across a tile edge, and it happens before anything is written);
//   scan     per row and column, over the tiles in order: the count at a tile's first frame = the totals before it + its own first k;
//   apply    walks the tile again from that count.  It reads and writes its own tile only, so in place is safe.
// A track of one tile needs the last launch alone.  The totals live in the caller's workspace; plain stores, one owner each, no atomics.
#include "rows.h"
#include <math.h>

namespace {

constexpr int UT = EG_UNWRAP_TILE_FRAMES;
constexpr int THREADS = 128;
constexpr int BATCH = 8;                                // loads in flight per thread

struct UArgs {
    float* p;
    const int* frames;
    int* ws;                                            // [2][rows, tiles, C]: totals -> starts | first k; null with one tile
    int rows, T, C, draws, frame_unit, tiles;
    double P;
    float P32;
};

__device__ __forceinline__ int jump(float cur, float prev, double P) { return (int)rint((double)(cur - prev) / P); }

// APPLY: write the frames; else: the totals of the tile.
template <bool APPLY>
__global__ __launch_bounds__(THREADS) void unwrap_kernel(const UArgs a) {
    const int c = blockIdx.y * THREADS + threadIdx.x;
    if (c >= a.C) return;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T);
    const int t0 = tile * UT, t1 = min(t0 + UT, n);
    const long long slot = ((long long)b * a.tiles + tile) * a.C + c, plane = (long long)a.rows * a.tiles * a.C;
    if (t0 >= t1) {
        if (!APPLY) { a.ws[slot] = 0; a.ws[plane + slot] = 0; }
        return;
    }
    float* p = a.p + ((long long)b * a.T + t0) * a.C + c;
    float prev = p[0];
    int cnt = 0, first = 0;
    if (APPLY) {
        cnt = a.ws ? a.ws[slot] : 0;
        p[0] = fmaf(-(float)cnt, a.P32, prev);
    } else if (t0 > 0) {
        first = jump(prev, p[-(long long)a.C], a.P);
        cnt = first;
    }
    for (int t = 1; t < t1 - t0; t += BATCH) {
        float v[BATCH];
#pragma unroll
        for (int e = 0; e < BATCH; ++e) v[e] = t + e < t1 - t0 ? p[(long long)(t + e) * a.C] : 0.f;
#pragma unroll
        for (int e = 0; e < BATCH; ++e)
            if (t + e < t1 - t0) {
                cnt += jump(v[e], prev, a.P);
                if (APPLY) p[(long long)(t + e) * a.C] = fmaf(-(float)cnt, a.P32, v[e]);
                prev = v[e];
            }
    }
    if (!APPLY) { a.ws[slot] = cnt; a.ws[plane + slot] = first; }
}

// One thread per (row, column): totals -> the count at every tile's first frame.
__global__ __launch_bounds__(THREADS) void unwrap_scan_kernel(const UArgs a) {
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= (long long)a.rows * a.C) return;
    const int b = (int)(q / a.C), c = (int)(q - (long long)b * a.C);
    const long long plane = (long long)a.rows * a.tiles * a.C;
    int* tot = a.ws + (long long)b * a.tiles * a.C + c;
    int run = 0;
    for (int tile = 0; tile < a.tiles; ++tile) {
        int* s = tot + (long long)tile * a.C;
        const int total = s[0];
        s[0] = run + s[plane];
        run += total;
    }
}

long long unwrap_bytes(const char* who, int rows, int T, int C) {
    if (rows < 1 || T < 1 || C < 1) {
        eg_set_error("%s: rows=%d frames=%d columns=%d (need >= 1)", who, rows, T, C);
        return 0;
    }
    const long long tiles = ((long long)T + UT - 1) / UT;
    if (tiles * rows > 0x7fffffffll || C > (1 << 20) || (long long)rows * C > 0x7fffffffll || (long long)rows * T * C >= (1ll << 40)) {
        eg_set_error("%s: rows=%d x frames=%d x columns=%d: grid / index range", who, rows, T, C);
        return 0;
    }
    return eg_round_up(tiles * rows * C * 2 * (long long)sizeof(int), 256);
}

}  // namespace

extern "C" int64_t eg_angle_unwrap_workspace_bytes(int32_t rows, int32_t T, int32_t C) {
    return unwrap_bytes("eg_angle_unwrap_workspace_bytes", rows, T, C);
}

extern "C" int eg_angle_unwrap(float* angles, int32_t rows, int32_t T, int32_t C, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                               double period, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "eg_angle_unwrap";
    EG_REQUIRE(angles, EG_ERR_BAD_ARG, "%s: null angles", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(angles) & 3u) == 0, EG_ERR_ALIGN, "%s: angles not 4-byte aligned", who);
    const long long need = unwrap_bytes(who, rows, T, C);
    if (need <= 0) return EG_ERR_BAD_ARG;
    if (int rc = egi_check_rows(who, rows, T, nullptr, d_frames, false, draws, frame_unit, 0, "")) return rc;
    EG_REQUIRE(isfinite(period) && period > 0.0 && isfinite((float)period) && (float)period > 0.f, EG_ERR_BAD_ARG,
               "%s: period=%g (need finite and > 0)", who, period);
    const int tiles = (int)(((long long)T + UT - 1) / UT);
    if (tiles > 1) {
        EG_REQUIRE(workspace, EG_ERR_BAD_ARG, "%s: null workspace", who);
        EG_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, EG_ERR_ALIGN, "%s: workspace not 4-byte aligned", who);
        EG_REQUIRE(workspace_bytes >= need, EG_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", who, (long long)workspace_bytes, need);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const UArgs a = {angles, d_frames, tiles > 1 ? static_cast<int*>(workspace) : nullptr, rows, T, C, draws, frame_unit, tiles, period, (float)period};
    const dim3 grid((unsigned)((long long)tiles * rows), (unsigned)((C + THREADS - 1) / THREADS)), block(THREADS);
    if (tiles > 1) {
        hipLaunchKernelGGL(unwrap_kernel<false>, grid, block, 0, st, a);
        int rc = eg_check_launch("angle_unwrap_totals");
        if (rc != EG_OK) return rc;
        hipLaunchKernelGGL(unwrap_scan_kernel, dim3((unsigned)(((long long)rows * C + THREADS - 1) / THREADS)), block, 0, st, a);
        rc = eg_check_launch("angle_unwrap_scan");
        if (rc != EG_OK) return rc;
    }
    hipLaunchKernelGGL(unwrap_kernel<true>, grid, block, 0, st, a);
    return eg_check_launch("angle_unwrap");
}
