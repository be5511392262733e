// BVH text of whole takes (include/emogest.h: eg_bvh_text_decimal, eg_bvh_text_workspace_bytes, eg_bvh_text_measure, eg_bvh_text_write): the
// MOTION lines of every take, "%.6f" of fp32 values joined by one space and ended by '\n', formatted on the device.  The decimal text is
// egi_decimal6 (bvhtext.h).  A tile is TF frames of one row; a wave owns a line at a time and walks its channels 64 at a time, so the place
// of a value inside its line is a wave scan of the widths and no workgroup barrier is needed until the tile is complete.
//   measure  lens    per tile: the length of every line (0 behind the row's last frame), their exclusive scan inside the tile into line_off,
//                    the tile's total and its count of values that are not writable -> workspace;
//            scan    one workgroup: the exclusive scan of the tile totals in (row, tile) order, the grand total, the counts per row;
//            apply   line_off[row, frame] += the start of its tile.  Integers throughout: plain stores, one owner each, no atomics, no memset.
//   write    one launch: a workgroup formats its tile into LDS at the byte the text has in memory modulo 16, then streams it out: 16-byte
//            stores over the aligned interior, byte stores for the head and the tail (a tile starts and ends at any byte).
#include "rows.h"
#include "bvhtext.h"

namespace {

constexpr int TF = EG_BVH_TEXT_TILE_FRAMES;
constexpr int THREADS = 256, WAVES = THREADS / EG_WAVE;
constexpr int SCAN_THREADS = 1024;
constexpr int SLOT = EG_BVH_TEXT_MAX_WIDTH + 1;                  // a value and the byte behind it
constexpr int CONST_PITCH = 20;

struct TArgs {
    const float* euler;
    const float* root;
    const int* src;                                     // [C]
    const int* clen;                                    // [C]
    const unsigned char* ctext;                         // [C][20]
    const int* frames;
    int rows, T, J3, C, draws, frame_unit, tiles;
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Channel c of frame t of row b: the table entry, clamped so that a device table that differs from the checked host copy stays in range.
// Returns the width of the text; `is_const`: it comes from the table, else d holds the value's decimal.
__device__ __forceinline__ int channel(const TArgs& a, int b, int t, int c, bool& is_const, EgiDecimal& d) {
    int s = a.src[c];
    if (s >= a.J3) s = a.J3 - 1;
    if (s < -3 || (s < 0 && !a.root)) {
        is_const = true;
        const int w = a.clen[c];
        return w < 8 ? 8 : (w > EG_BVH_TEXT_MAX_WIDTH ? EG_BVH_TEXT_MAX_WIDTH : w);
    }
    is_const = false;
    const float v = s >= 0 ? a.euler[((long long)b * a.T + t) * a.J3 + s] : a.root[((long long)(b / a.draws) * a.T + t) * 3 + (-1 - s)];
    d = egi_decimal6(v);
    return d.width;
}

__global__ __launch_bounds__(THREADS) void bvh_text_lens_kernel(const TArgs a, long long* __restrict__ line_off, long long* __restrict__ tot,
                                                                int* __restrict__ bad) {
    __shared__ int s_len[TF];
    __shared__ int s_bad[WAVES];
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T, 1);
    const int t0 = tile * TF, wave = threadIdx.x / EG_WAVE, lane = threadIdx.x % EG_WAVE;
    int nbad = 0;
    for (int f = wave; f < TF; f += WAVES) {
        const int t = t0 + f;
        int len = 0;
        if (t < n) {
            for (int c = lane; c < a.C; c += EG_WAVE) {
                bool is_const;
                EgiDecimal d;
                len += channel(a, b, t, c, is_const, d) + 1;
                nbad += !is_const && !d.ok;
            }
        }
        len = wave_sum_i(len);
        if (lane == 0) s_len[f] = len;
    }
    nbad = wave_sum_i(nbad);
    if (lane == 0) s_bad[wave] = nbad;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int f = 0; f < TF; ++f) {
            if (t0 + f < a.T) line_off[(long long)b * a.T + t0 + f] = run;
            run += s_len[f];
        }
        int nb = 0;
        for (int w = 0; w < WAVES; ++w) nb += s_bad[w];
        tot[blockIdx.x] = run;
        bad[blockIdx.x] = nb;
    }
}

// One workgroup: tot [N] (N = rows * tiles, row-major) -> its exclusive scan in place; the grand total to line_off[rows * T] and the summary;
// the counts of a row's tiles added in ascending order.
__global__ __launch_bounds__(SCAN_THREADS) void bvh_text_scan_kernel(long long* __restrict__ tot, const int* __restrict__ bad, long long N, int rows,
                                                                     int tiles, long long* __restrict__ line_end, long long* __restrict__ total,
                                                                     int* __restrict__ row_bad) {
    __shared__ long long s[SCAN_THREADS];
    const int tid = threadIdx.x;
    const long long per = (N + SCAN_THREADS - 1) / SCAN_THREADS;
    const long long i0 = tid * per < N ? tid * per : N, i1 = i0 + per < N ? i0 + per : N;
    long long local = 0;
    for (long long i = i0; i < i1; ++i) local += tot[i];
    s[tid] = local;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {
        const long long v = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    long long run = s[tid] - local;
    for (long long i = i0; i < i1; ++i) {
        const long long v = tot[i];
        tot[i] = run;
        run += v;
    }
    if (tid == SCAN_THREADS - 1) {
        *line_end = s[tid];
        *total = s[tid];
    }
    for (int r = tid; r < rows; r += SCAN_THREADS) row_bad[r] = egi_sum_tiles<int>(bad + (long long)r * tiles, 1, tiles);
}

__global__ __launch_bounds__(THREADS) void bvh_text_apply_kernel(long long* __restrict__ line_off, const long long* __restrict__ tot, int rows, int T,
                                                                 int tiles) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (long long)rows * T) return;
    const int b = (int)(i / T), t = (int)(i - (long long)b * T);
    line_off[i] += tot[(long long)b * tiles + t / TF];
}

// cap: the bytes of LDS behind `lds` (a multiple of 16).  Every LDS store is checked against cap and every global store against text_bytes: a
// line_off that does not belong to these inputs gives wrong text, nothing out of range.
__global__ __launch_bounds__(THREADS) void bvh_text_write_kernel(const TArgs a, const long long* __restrict__ line_off, unsigned char* __restrict__ text,
                                                                 long long text_bytes, int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T, 1);
    const int t0 = tile * TF;
    if (t0 >= n) return;                                                   // the whole workgroup
    const int nf = min(TF, n - t0), wave = threadIdx.x / EG_WAVE, lane = threadIdx.x % EG_WAVE;
    const long long* lo = line_off + (long long)b * a.T + t0;
    const long long start = lo[0], base = start & ~15ll;
    const long long end = lo[nf];      // the entry behind the tile's last line: the next frame of the row, the next row, or line_off[rows * T]
    auto put = [&](long long p, unsigned char ch) {
        if (p >= 0 && p < cap) lds[p] = ch;
    };
    for (int f = wave; f < nf; f += WAVES) {
        const int t = t0 + f;
        long long at = lo[f] - base;
        for (int c0 = 0; c0 < a.C; c0 += EG_WAVE) {
            const int c = c0 + lane;
            bool is_const = true;
            EgiDecimal d;
            int w = 0;
            if (c < a.C) w = channel(a, b, t, c, is_const, d) + 1;
            int x = w;
#pragma unroll
            for (int o = 1; o < EG_WAVE; o <<= 1) {
                const int y = __shfl_up(x, o, 64);
                if (lane >= o) x += y;
            }
            if (c < a.C) {
                const long long p = at + x - w;
                if (is_const) {
                    const unsigned char* src = a.ctext + (long long)c * CONST_PITCH;
                    for (int i = 0; i < w - 1; ++i) put(p + i, src[i]);
                } else {
                    egi_decimal6_put(d, [&](int i, unsigned char ch) { put(p + i, ch); });
                }
                put(p + w - 1, c == a.C - 1 ? (unsigned char)'\n' : (unsigned char)' ');
            }
            at += __shfl(x, EG_WAVE - 1, 64);
        }
    }
    __syncthreads();
    const long long hi = min(min(end, text_bytes), base + cap);
    if (start < 0 || start >= hi) return;
    const long long a0 = min((start + 15) & ~15ll, hi), a1 = max(a0, hi & ~15ll);
    for (long long g = start + threadIdx.x; g < a0; g += THREADS) text[g] = lds[g - base];
    for (long long g = a0 + 16ll * threadIdx.x; g < a1; g += 16ll * THREADS)
        *reinterpret_cast<uint4*>(text + g) = *reinterpret_cast<const uint4*>(lds + (g - base));
    for (long long g = a1 + threadIdx.x; g < hi; g += THREADS) text[g] = lds[g - base];
}

long long text_ws_bytes(const char* who, int rows, int T, int C) {
    if (rows < 1 || T < 1 || C < 1 || C > EG_BVH_TEXT_MAX_CHANNELS) {
        eg_set_error("%s: rows=%d frames=%d channels=%d (need rows, frames >= 1 and channels in 1..%d)", who, rows, T, C, EG_BVH_TEXT_MAX_CHANNELS);
        return 0;
    }
    const long long tiles = ((long long)T + TF - 1) / TF;
    if (tiles * rows > 0x7fffffffll || (long long)rows * T > 0x7fffffffll) {
        eg_set_error("%s: rows=%d x frames=%d: grid / index range", who, rows, T);
        return 0;
    }
    return eg_round_up(tiles * rows * 8, 256) + eg_round_up(tiles * rows * 4, 256);
}

int lds_cap(int C) { return (int)eg_round_up((long long)TF * C * SLOT + 16, 16); }

// Everything both calls check, in one order and one wording; fills the kernels' arguments.
int check_args(const char* who, const EgBvhTextArgs* in, TArgs* out) {
    EG_REQUIRE(in, EG_ERR_BAD_ARG, "%s: null argument block", who);
    EG_REQUIRE(in->euler && in->table && in->d_table, EG_ERR_BAD_ARG, "%s: null euler, table or d_table", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(in->euler) & 3u) == 0 && (reinterpret_cast<uintptr_t>(in->root_position) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(in->d_table) & 3u) == 0 && (reinterpret_cast<uintptr_t>(in->table) & 3u) == 0, EG_ERR_ALIGN,
               "%s: euler, root_position, table or d_table not 4-byte aligned", who);
    if (text_ws_bytes(who, in->rows, in->T, in->C) <= 0) return EG_ERR_BAD_ARG;
    EG_REQUIRE(in->J3 >= 1, EG_ERR_BAD_ARG, "%s: J3=%d (need >= 1)", who, in->J3);
    EG_REQUIRE((long long)in->rows * in->T * in->J3 < (1ll << 40), EG_ERR_BAD_ARG, "%s: rows=%d x frames=%d x J3=%d: index range", who, in->rows,
               in->T, in->J3);
    if (int rc = egi_check_rows(who, in->rows, in->T, in->frames, in->d_frames, true, in->draws, in->frame_unit, 1, "1")) return rc;
    const int C = in->C;
    const int32_t* src = static_cast<const int32_t*>(in->table);
    const int32_t* clen = src + C;
    for (int c = 0; c < C; ++c) {
        EG_REQUIRE(src[c] >= -4 && src[c] < in->J3, EG_ERR_BAD_ARG, "%s: src[%d]=%d (need -4 .. J3 - 1 = %d)", who, c, src[c], in->J3 - 1);
        EG_REQUIRE(src[c] >= 0 || src[c] == -4 || in->root_position, EG_ERR_BAD_ARG, "%s: src[%d]=%d names root_position, which is null", who, c,
                   src[c]);
        EG_REQUIRE(src[c] != -4 || (clen[c] >= 8 && clen[c] <= EG_BVH_TEXT_MAX_WIDTH), EG_ERR_BAD_ARG, "%s: const_len[%d]=%d (need 8 .. %d)", who, c,
                   clen[c], EG_BVH_TEXT_MAX_WIDTH);
    }
    const int* d_src = static_cast<const int*>(in->d_table);
    *out = {in->euler, in->root_position, d_src, d_src + C, reinterpret_cast<const unsigned char*>(d_src + 2 * C), in->d_frames,
            in->rows, in->T, in->J3, C, in->draws, in->frame_unit, (int)(((long long)in->T + TF - 1) / TF)};
    return EG_OK;
}

}  // namespace

extern "C" int32_t eg_bvh_text_decimal(float v, char out[20]) {
    const EgiDecimal d = egi_decimal6(v);
    if (!d.ok || !out) return -1;
    egi_decimal6_put(d, [&](int i, unsigned char ch) { out[i] = (char)ch; });
    out[d.width] = 0;
    return d.width;
}

extern "C" int32_t eg_bvh_text_tile_frames(void) { return TF; }

extern "C" int64_t eg_bvh_text_table_bytes(int32_t C) {
    if (C < 1 || C > EG_BVH_TEXT_MAX_CHANNELS) {
        eg_set_error("eg_bvh_text_table_bytes: channels=%d (need 1..%d)", C, EG_BVH_TEXT_MAX_CHANNELS);
        return 0;
    }
    return (int64_t)C * (8 + CONST_PITCH);
}

extern "C" int64_t eg_bvh_text_workspace_bytes(int32_t rows, int32_t T, int32_t C) {
    return text_ws_bytes("eg_bvh_text_workspace_bytes", rows, T, C);
}

extern "C" int eg_bvh_text_measure(const EgBvhTextArgs* in, void* workspace, int64_t workspace_bytes, int64_t* line_off, void* summary,
                                   void* stream) {
    const char* who = "eg_bvh_text_measure";
    TArgs a;
    if (int rc = check_args(who, in, &a)) return rc;
    EG_REQUIRE(workspace && line_off && summary, EG_ERR_BAD_ARG, "%s: null workspace, line_off or summary", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(line_off) & 7u) == 0 &&
               (reinterpret_cast<uintptr_t>(summary) & 7u) == 0, EG_ERR_ALIGN, "%s: workspace, line_off or summary not 8-byte aligned", who);
    const long long need = text_ws_bytes(who, a.rows, a.T, a.C);
    EG_REQUIRE(workspace_bytes >= need, EG_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", who, (long long)workspace_bytes, need);
    const long long N = (long long)a.rows * a.tiles;
    long long* tot = static_cast<long long*>(workspace);
    int* bad = reinterpret_cast<int*>(static_cast<char*>(workspace) + eg_round_up(N * 8, 256));
    long long* off = reinterpret_cast<long long*>(line_off);
    long long* total = static_cast<long long*>(summary);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bvh_text_lens_kernel, dim3((unsigned)N), dim3(THREADS), 0, st, a, off, tot, bad);
    if (int rc = eg_check_launch("bvh_text_lens")) return rc;
    hipLaunchKernelGGL(bvh_text_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, tot, bad, N, a.rows, a.tiles, off + (long long)a.rows * a.T, total,
                       reinterpret_cast<int*>(total + 1));
    if (int rc = eg_check_launch("bvh_text_scan")) return rc;
    hipLaunchKernelGGL(bvh_text_apply_kernel, dim3((unsigned)(((long long)a.rows * a.T + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, off, tot,
                       a.rows, a.T, a.tiles);
    return eg_check_launch("bvh_text_apply");
}

extern "C" int eg_bvh_text_write(const EgBvhTextArgs* in, const int64_t* line_off, void* text, int64_t text_bytes, void* stream) {
    const char* who = "eg_bvh_text_write";
    TArgs a;
    if (int rc = check_args(who, in, &a)) return rc;
    EG_REQUIRE(line_off && text, EG_ERR_BAD_ARG, "%s: null line_off or text", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(line_off) & 7u) == 0, EG_ERR_ALIGN, "%s: line_off not 8-byte aligned", who);
    EG_REQUIRE(eg_aligned16(text), EG_ERR_ALIGN, "%s: text not 16-byte aligned", who);
    EG_REQUIRE(text_bytes >= 1, EG_ERR_BAD_ARG, "%s: text_bytes=%lld (need >= 1)", who, (long long)text_bytes);
    const int cap = lds_cap(a.C);
    if (cap > 64 * 1024)
        if (int rc = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(bvh_text_write_kernel), (size_t)cap, who)) return rc;
    hipLaunchKernelGGL(bvh_text_write_kernel, dim3((unsigned)((long long)a.rows * a.tiles)), dim3(THREADS), (size_t)cap,
                       static_cast<hipStream_t>(stream), a, reinterpret_cast<const long long*>(line_off), static_cast<unsigned char*>(text),
                       (long long)text_bytes, cap);
    return eg_check_launch("bvh_text_write");
}
