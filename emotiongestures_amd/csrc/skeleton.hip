// Skeleton output (include/emogest.h: eg_skeleton_check, eg_skeleton_out_frames, eg_skeleton_tile_frames, eg_skeleton_joints,
// eg_skeleton_dir_vec): whole gesture tracks in the model's coordinates (K bone direction vectors per frame) -> joint positions, and back.
//   forward   x_k = track[b, t, 3k .. 3k+2] (+ mean_k) (unit: / max(|x_k|, 1e-12));  p[0] = 0,  p[child_k] = p[parent_k] + len_k * x_k in table order;
//             output frame k' of a row with n valid frames: lo = min(floor(k' M / L), n - 2), f = (k' M - lo L) / L, joints = p(lo) + (p(lo+1) - p(lo)) f
//             (linear interpolation, extrapolated past the last frame; L / M = 1: joints = p(k') and nothing is blended); zeros from ceil(n L / M) on.
//   inverse   d = p[child_k] - p[parent_k], d / max(|d|, 1e-12) (- mean_k); zeros from frame n on.
// Both are memory-bound streams: a workgroup stages the source frames of a tile of TF output frames through LDS with 16-byte loads (the span
// starts up to 3 floats early, as in resample.hip: 3K and 3J are no multiples of 4), walks the tree with one thread per (source frame,
// coordinate) column of a transposed LDS tile p[joint][column] -- a thread's parent reads are its own earlier writes, so the chain needs no
// barrier, and the rows of the tile are conflict-free -- and writes the outputs coalesced, 16 bytes per lane where a quad lies inside the tile.
// The bone table is an argument, read once per workgroup; nothing about a particular body is built in.  Every output element has one owning
// thread; plain vector stores, no atomics, nothing device-scope; the grid depends on the shapes only.
//   rotations (eg_skeleton_rest_check, eg_skeleton_levels, eg_skeleton_rotations): one local rotation per bone relative to a rest pose.  The grid,
//             the staging and the frame handling are the forward kernel's (tile_of, Walk, stage_pass), but the vectors are blended, not the results,
//             and the chain is a dependent run of
//             quaternion products, so it is walked level by level: the host orders the bones by depth, one thread owns one (output frame, bone of
//             the level), one barrier per level.  The global rotations live in an LDS tile g[bone][component][frame] (lanes of consecutive frames
//             on consecutive banks); x is blended and normalised in registers as it is read; every (frame, bone) leaves as one aligned 16-byte store.
#include "common.h"
#include <math.h>

namespace {

constexpr int TF = EG_SKELETON_TILE_FRAMES;             // output frames of one workgroup
constexpr int SLOTS = TF + 2;                           // source frames of one pass: TF output frames at L >= M touch at most TF + 1
constexpr int NC = 3 * SLOTS;                           // columns of the joint tile: (source frame, coordinate)
constexpr int THREADS = 128;
constexpr int MAX_K = EG_SKELETON_MAX_BONES;
constexpr int MAX_LM = EG_SKELETON_MAX_FACTOR;
constexpr int TAB = 64;                                 // LDS words per table column
constexpr int HEAD = 3 * TAB + 3 * TAB;                 // parent | child | length | mean [3 * 64]
static_assert(NC <= THREADS, "one thread per column of the joint tile");
static_assert(MAX_K < TAB, "table columns hold K <= 63 bones");

__host__ __device__ constexpr int round4(int v) { return (v + 3) & ~3; }
__host__ __device__ inline long long out_frames(long long n, int L, int M) { return (n * L + M - 1) / M; }

struct Args {
    const float* src;                                   // track [B, T, 3K] (forward) / joints [B, T, J, 3] (inverse)
    const int* table;                                   // device words: parent [K] | child [K] | length (fp32 bits) [K]
    const int* frames;                                  // device [B / draws] or null
    const float* mean;                                  // device [3K] or null
    float* dst;
    int B, T, K, draws, frame_unit, L, M, tiles;
    long long T_out;
};

// Floats [g0, g1) of base (16-byte aligned; `total` floats in all) -> lds[g - (g0 & ~3)].  Whole quads: the floats before g0 and after g1 that
// share a quad with the span are copied too (never used); nothing past `total` is read.
__device__ __forceinline__ void stage_span(const float* __restrict__ base, long long g0, long long g1, long long total, float* lds) {
    const long long lo4 = g0 & ~3ll;
    for (long long q = lo4 + 4ll * threadIdx.x; q < g1; q += 4ll * THREADS) {
        f4 v;
        if (q + 3 < total) {
            v = *reinterpret_cast<const f4*>(base + q);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = q + e < total ? base[q + e] : 0.f;
        }
        *reinterpret_cast<f4*>(lds + (q - lo4)) = v;
    }
}

// base[g] = f(fr, r) for g in [g0, g1), where g - origin = fr * row + r: 16-byte stores for the quads inside the range, single floats at its two
// ends.  One division per quad; (fr, r) then step with the element.
template <class F>
__device__ __forceinline__ void store_range(float* __restrict__ base, long long origin, int row, long long g0, long long g1, F f) {
    for (long long q = (g0 & ~3ll) + 4ll * threadIdx.x; q < g1; q += 4ll * THREADS) {
        const int rel = (int)(q - origin);                                      // >= -3: g0 >= origin
        int fr = rel >= 0 ? rel / row : -1;
        int r = rel >= 0 ? rel - fr * row : rel + row;
        const bool whole = q >= g0 && q + 4 <= g1;
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = whole || (q + e >= g0 && q + e < g1);
            v[e] = in ? f(fr, r) : 0.f;
            if (!whole && in) base[q + e] = v[e];
            if (++r == row) { r = 0; ++fr; }
        }
        if (whole) *reinterpret_cast<f4*>(base + q) = v;
    }
}

__device__ __forceinline__ int valid_frames(const Args& a, int b) {
    if (!a.frames) return a.T;
    const long long v = (long long)a.frames[b / a.draws] * a.frame_unit;
    return (int)(v < 0 ? 0 : (v > a.T ? a.T : v));
}

__device__ __forceinline__ void load_mean(const Args& a, float* mn) {
    if (a.mean)
        for (int r = threadIdx.x; r < 3 * a.K; r += THREADS) mn[r] = a.mean[r];
}

// The first HEAD words of LDS, filled by the workgroup.  The host table is checked; the device copy is the caller's.  Its joint numbers index
// LDS, so they are clamped to 0..K here: with a stale upload the result is unspecified, but every access stays inside the tile.
struct Head { int *ta, *tb; float *tl, *mn; };
__device__ __forceinline__ Head load_head(const Args& a, float* lds) {
    const Head h = {reinterpret_cast<int*>(lds), reinterpret_cast<int*>(lds) + TAB, lds + 2 * TAB, lds + 3 * TAB};
    for (int k = threadIdx.x; k < a.K; k += THREADS) {
        h.ta[k] = min(max(a.table[k], 0), a.K);
        h.tb[k] = min(max(a.table[a.K + k], 0), a.K);
        h.tl[k] = __int_as_float(a.table[2 * a.K + k]);
    }
    load_mean(a, h.mn);
    return h;
}

// What a workgroup owns.  grid: (tile of TF frames) x row, flattened: frames [k0, k0 + cnt) of the T_out frames of row b, the first `live` of
// them inside the row's own output (n valid source frames); the rest of the tile is the zero tail behind a ragged row.  NATIVE: L / M = 1.
// live64 is live before it is cut to 32 bits, and zero_tail's offset is made from it: do not fold the two.  With `live` alone the compiler narrows
// the selects, the joints prologue loses three scalar instructions, all code behind it moves by 12 bytes and the native kernel measures 1-2 % slower.
struct Tile { int b; long long k0; int cnt, n; long long live64; int live; };

template <bool NATIVE>
__device__ __forceinline__ Tile tile_of(const Args& a, long long T_out) {
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const long long k0 = (long long)tile * TF;
    const int cnt = (int)(T_out - k0 < TF ? T_out - k0 : TF);
    const int n = valid_frames(a, b);
    const long long n_out = NATIVE ? n : out_frames(n, a.L, a.M);
    const long long live = n_out - k0 < 0 ? 0 : (n_out - k0 < cnt ? n_out - k0 : cnt);
    return {b, k0, cnt, n, live, (int)live};
}

// Zeros in the frames [live, cnt) of a tile whose frames have `row` floats and start at float out0.
__device__ __forceinline__ void zero_tail(float* __restrict__ dst, long long out0, int row, const Tile& t) {
    if (t.live < t.cnt) store_range(dst, out0, row, out0 + t.live64 * row, out0 + (long long)t.cnt * row, [](int, int) { return 0.f; });
}

// The source frames of a tile of the forward kernels.  A pass makes the outputs [i, i1) of the tile from the source frames
// [s_base, s_base + nslots): as many outputs as SLOTS source frames reach (all of them unless the rate drops, M > L).
struct Pass { long long s_base; int i1, nslots; };
struct Blend { int slot; float f; };                    // output = frame(slot) + (frame(slot + 1) - frame(slot)) * f, slots counted from s_base

template <bool NATIVE>
struct Walk {
    long long k0;
    int n, L, M;
    __device__ __forceinline__ long long seg(long long kk) const {             // first source frame of output frame kk
        if (NATIVE) return kk;
        if (n < 2) return 0;
        const long long lo = kk * M / L;
        return lo < n - 2 ? lo : n - 2;
    }
    __device__ __forceinline__ Pass pass(int i, int live) const {
        const long long s_base = seg(k0 + i);
        int i1 = live;
        if (!NATIVE && M > L) {
            const long long jmax = ((s_base + SLOTS - 1) * L - 1) / M - k0;     // last output whose segment starts at or before s_base + SLOTS - 2
            i1 = jmax + 1 < live ? (int)(jmax + 1) : live;
            i1 = i1 > i ? i1 : i + 1;
        }
        return {s_base, i1, (int)(seg(k0 + i1 - 1) - s_base) + ((NATIVE || n < 2) ? 1 : 2)};
    }
    __device__ __forceinline__ Blend blend(const Pass& p, int fr) const {      // output frame fr of the tile; not NATIVE, n >= 2
        const long long kk = k0 + fr, lo = seg(kk);
        return {(int)(lo - p.s_base), (float)(kk * M - lo * L) / (float)L};
    }
};

// The pass that starts at output i of the tile (for (i = 0; i < live; i = p.i1)): its source frames staged into xin, one barrier behind the
// loads; returns where they start.  No barrier before the staging of a later pass: the last barrier of the caller's pass ended the reads of
// xin (joints: the one behind the chain; rotations: the one behind the last level), and the one here precedes every write of the caller's tile.
template <bool NATIVE>
__device__ __forceinline__ float* stage_pass(const Args& a, const Tile& t, const Walk<NATIVE>& w, int i, float* xin, Pass& p) {
    const int D = 3 * a.K;
    p = w.pass(i, t.live);
    const long long g0 = ((long long)t.b * a.T + p.s_base) * D;
    stage_span(a.src, g0, g0 + (long long)p.nslots * D, (long long)a.B * a.T * D, xin);
    __syncthreads();
    return xin + (int)(g0 & 3);
}

// NATIVE: L / M = 1.
template <bool UNIT, bool NATIVE>
__global__ __launch_bounds__(THREADS) void skeleton_joints_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = a.K, D = 3 * K, J3 = 3 * (K + 1), tid = threadIdx.x;
    float* xin = lds + HEAD;
    float* pj = xin + round4(SLOTS * D + 8);
    const Tile t = tile_of<NATIVE>(a, a.T_out);
    const long long out0 = ((long long)t.b * a.T_out + t.k0) * J3;
    zero_tail(a.dst, out0, J3, t);
    if (t.live == 0) return;
    const Head h = load_head(a, lds);
    for (int c = tid; c < NC; c += THREADS) pj[c] = 0.f;                        // the root joint, every column
    const bool has_mean = a.mean != nullptr;
    const Walk<NATIVE> w = {t.k0, t.n, a.L, a.M};
    Pass ps;
    for (int i = 0; i < t.live; i = ps.i1) {
        float* x = stage_pass(a, t, w, i, xin, ps);
        if (UNIT) {                                                             // one thread per (source frame, bone), in place
            for (int q = tid; q < ps.nslots * K; q += THREADS) {
                const int s = q / K, k = q - s * K;
                float* v = x + s * D + 3 * k;
                float v0 = v[0], v1 = v[1], v2 = v[2];
                if (has_mean) { v0 += h.mn[3 * k]; v1 += h.mn[3 * k + 1]; v2 += h.mn[3 * k + 2]; }
                const float d = fmaxf(sqrtf(v0 * v0 + v1 * v1 + v2 * v2), 1e-12f);
                v[0] = v0 / d; v[1] = v1 / d; v[2] = v2 / d;
            }
            __syncthreads();
        }
        if (tid < 3 * ps.nslots) {                                              // the chain: this thread's column of every joint
            const int s = tid / 3, c = tid - 3 * s;
            const float* xs = x + s * D + c;
            float* pc = pj + tid;
            float xv = xs[0];
            for (int k = 0; k < K; ++k) {
                const float xn = k + 1 < K ? xs[3 * (k + 1)] : 0.f;             // the next bone's vector is in flight while this one is added
                float v = xv;
                if (!UNIT && has_mean) v += h.mn[3 * k + c];
                pc[h.tb[k] * NC] = fmaf(h.tl[k], v, pc[h.ta[k] * NC]);
                xv = xn;
            }
        }
        __syncthreads();
        store_range(a.dst, out0, J3, out0 + (long long)i * J3, out0 + (long long)ps.i1 * J3, [&](int fr, int r) {
            const int jt = r / 3, c = r - 3 * jt;
            const float* row = pj + jt * NC + c;
            if (NATIVE) return row[3 * (fr - i)];
            if (t.n < 2) return row[0];
            const Blend bl = w.blend(ps, fr);
            const float p0 = row[3 * bl.slot], p1 = row[3 * bl.slot + 3];
            return fmaf(p1 - p0, bl.f, p0);
        });
    }
}

__global__ __launch_bounds__(THREADS) void skeleton_dir_vec_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = a.K, D = 3 * K, J3 = 3 * (K + 1);
    float* pin = lds + HEAD;
    const Tile t = tile_of<true>(a, a.T);
    const long long out0 = ((long long)t.b * a.T + t.k0) * D;
    zero_tail(a.dst, out0, D, t);
    if (t.live == 0) return;
    const Head h = load_head(a, lds);
    const bool has_mean = a.mean != nullptr;
    const long long g0 = ((long long)t.b * a.T + t.k0) * J3;
    stage_span(a.src, g0, g0 + (long long)t.live * J3, (long long)a.B * a.T * J3, pin);
    __syncthreads();
    const float* p = pin + (int)(g0 & 3);
    store_range(a.dst, out0, D, out0, out0 + (long long)t.live * D, [&](int fr, int r) {
        const int k = r / 3, c = r - 3 * k;
        const float* pa = p + fr * J3 + 3 * h.ta[k];
        const float* pb = p + fr * J3 + 3 * h.tb[k];
        const float d0 = pb[0] - pa[0], d1 = pb[1] - pa[1], d2 = pb[2] - pa[2];
        const float d = fmaxf(sqrtf(d0 * d0 + d1 * d1 + d2 * d2), 1e-12f);
        const float v = (c == 0 ? d0 : (c == 1 ? d1 : d2)) / d;
        return has_mean ? v - h.mn[r] : v;
    });
}

// ---- rotations ------------------------------------------------------------------------------------------------------------------------------
// The level table of eg_skeleton_levels (include/emogest.h): the level count | LEVEL_SLOTS level offsets | order [K] | bone parents [K] | rest [3K].
constexpr int LEVEL_SLOTS = 64;
constexpr int LV_FIRST = 1, LV_ORDER = LV_FIRST + LEVEL_SLOTS;
__host__ __device__ constexpr int lv_parents(int K) { return LV_ORDER + K; }
__host__ __device__ constexpr int lv_rest(int K) { return LV_ORDER + 2 * K; }
static_assert(lv_rest(1) + 3 == EG_SKELETON_LEVEL_WORDS(1) && lv_rest(MAX_K) + 3 * MAX_K == EG_SKELETON_LEVEL_WORDS(MAX_K), "the header's table size");
static_assert(MAX_K <= LEVEL_SLOTS, "a level per bone at most, and the offset behind the last one");
constexpr int LV_OFFS = round4(LV_ORDER);               // LDS words: level offsets [nlev + 1 <= LEVEL_SLOTS] (+ pad)
constexpr int RHEAD = LV_OFFS + 2 * TAB + 3 * TAB + 3 * TAB;    // offsets | order | bone parents | rest [3 * 64] | mean [3 * 64]
static_assert(RHEAD % 4 == 0, "the staged frames start on a quad");

struct Quat { float w, x, y, z; };

__device__ __forceinline__ Quat qmul(const Quat& p, const Quat& q) {             // Hamilton product
    return {p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z, p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y,
            p.w * q.y - p.x * q.z + p.y * q.w + p.z * q.x, p.w * q.z + p.x * q.y - p.y * q.x + p.z * q.w};
}

// conj(q) o v: v + 2 w (u x v) + 2 u x (u x v) with u = -q.xyz
__device__ __forceinline__ void rotate_back(const Quat& q, float& v0, float& v1, float& v2) {
    const float u0 = -q.x, u1 = -q.y, u2 = -q.z;
    const float t0 = 2.f * (u1 * v2 - u2 * v1), t1 = 2.f * (u2 * v0 - u0 * v2), t2 = 2.f * (u0 * v1 - u1 * v0);
    v0 += q.w * t0 + (u1 * t2 - u2 * t1);
    v1 += q.w * t1 + (u2 * t0 - u0 * t2);
    v2 += q.w * t2 + (u0 * t1 - u1 * t0);
}

// The shortest arc from the unit vector a to the unit (or zero) vector b; the half turn about a fixed axis perpendicular to a where they oppose.
__device__ __forceinline__ Quat arc(float a0, float a1, float a2, float b0, float b1, float b2) {
    const float c = a0 * b0 + a1 * b1 + a2 * b2;
    if (c >= -1.f + 1e-6f) {
        const float w = 1.f + c, x = a1 * b2 - a2 * b1, y = a2 * b0 - a0 * b2, z = a0 * b1 - a1 * b0;
        const float d = sqrtf(w * w + x * x + y * y + z * z);
        return {w / d, x / d, y / d, z / d};
    }
    const float m0 = fabsf(a0), m1 = fabsf(a1), m2 = fabsf(a2);
    float x, y, z;                                                              // a x e_m, m the first axis on which |a| is smallest
    if (m0 <= m1 && m0 <= m2) { x = 0.f; y = a2; z = -a1; }
    else if (m1 <= m2) { x = -a2; y = 0.f; z = a0; }
    else { x = a1; y = -a0; z = 0.f; }
    const float d = sqrtf(x * x + y * y + z * z);
    return {0.f, x / d, y / d, z / d};
}

// NATIVE: L / M = 1.  GLOBAL: the output holds G_k, else L_k.
// a.table is the level table of eg_skeleton_levels; as in load_head its numbers index LDS and the output, so they are clamped.
template <bool NATIVE, bool GLOBAL>
__global__ __launch_bounds__(THREADS) void skeleton_rotations_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = a.K, D = 3 * K, Q = 4 * K, tid = threadIdx.x;
    int* lv = reinterpret_cast<int*>(lds);
    int* ord = lv + LV_OFFS;
    int* pbt = ord + TAB;
    float* rs = lds + LV_OFFS + 2 * TAB;
    float* mn = rs + 3 * TAB;
    float* xin = lds + RHEAD;
    float* gt = xin + round4(SLOTS * D + 8);                                    // g[bone][component][frame of the tile]
    const Tile t = tile_of<NATIVE>(a, a.T_out);
    float* out = a.dst + ((long long)t.b * a.T_out + t.k0) * Q;                  // 16-byte aligned: Q is a multiple of 4
    for (int q = t.live * K + tid; q < t.cnt * K; q += THREADS) *reinterpret_cast<f4*>(out + 4ll * q) = f4{0.f, 0.f, 0.f, 0.f};
    if (t.live == 0) return;
    const int nlev = min(max(a.table[0], 1), K);
    for (int l = tid; l <= nlev; l += THREADS) lv[l] = min(max(a.table[LV_FIRST + l], 0), K);
    for (int k = tid; k < K; k += THREADS) {
        ord[k] = min(max(a.table[LV_ORDER + k], 0), K - 1);
        pbt[k] = min(max(a.table[lv_parents(K) + k], -1), K - 1);
    }
    for (int r = tid; r < D; r += THREADS) rs[r] = __int_as_float(a.table[lv_rest(K) + r]);
    const bool has_mean = a.mean != nullptr;
    load_mean(a, mn);
    // stage_pass' barrier also covers the tables, and the last level of the pass before
    const Walk<NATIVE> w = {t.k0, t.n, a.L, a.M};
    Pass ps;
    for (int i = 0; i < t.live; i = ps.i1) {
        const float* x = stage_pass(a, t, w, i, xin, ps);
        const int nf = ps.i1 - i;
        for (int l = 0; l < nlev; ++l) {
            const int b0 = lv[l], nb = max(lv[l + 1] - b0, 0);
            for (int q = tid; q < nf * nb; q += THREADS) {                       // one thread per (output frame, bone of the level)
                const int j = q / nf, fr = i + (q - j * nf);
                const int k = ord[min(b0 + j, K - 1)], p = pbt[k];
                float x0, x1, x2;
                if (NATIVE || t.n < 2) {
                    const float* xs = x + (NATIVE ? fr - i : 0) * D + 3 * k;
                    x0 = xs[0]; x1 = xs[1]; x2 = xs[2];
                    if (has_mean) { x0 += mn[3 * k]; x1 += mn[3 * k + 1]; x2 += mn[3 * k + 2]; }
                } else {                                                        // the vectors are blended, after the mean
                    const Blend bl = w.blend(ps, fr);
                    const float f = bl.f;
                    const float* xs = x + bl.slot * D + 3 * k;
                    float y0 = xs[0], y1 = xs[1], y2 = xs[2], z0 = xs[D], z1 = xs[D + 1], z2 = xs[D + 2];
                    if (has_mean) {
                        y0 += mn[3 * k]; y1 += mn[3 * k + 1]; y2 += mn[3 * k + 2];
                        z0 += mn[3 * k]; z1 += mn[3 * k + 1]; z2 += mn[3 * k + 2];
                    }
                    x0 = fmaf(z0 - y0, f, y0); x1 = fmaf(z1 - y1, f, y1); x2 = fmaf(z2 - y2, f, y2);
                }
                const float d = fmaxf(sqrtf(x0 * x0 + x1 * x1 + x2 * x2), 1e-12f);
                x0 /= d; x1 /= d; x2 /= d;
                Quat P = {1.f, 0.f, 0.f, 0.f};
                if (p >= 0) {
                    const float* gp = gt + p * 4 * TF + fr;
                    P = {gp[0], gp[TF], gp[2 * TF], gp[3 * TF]};
                    rotate_back(P, x0, x1, x2);                                 // the bone's direction seen from its parent's frame
                }
                const Quat Lq = arc(rs[3 * k], rs[3 * k + 1], rs[3 * k + 2], x0, x1, x2);
                const Quat G = p >= 0 ? qmul(P, Lq) : Lq;
                float* gk = gt + k * 4 * TF + fr;
                gk[0] = G.w; gk[TF] = G.x; gk[2 * TF] = G.y; gk[3 * TF] = G.z;
                const Quat& o = GLOBAL ? G : Lq;
                *reinterpret_cast<f4*>(out + ((long long)fr * K + k) * 4) = f4{o.w, o.x, o.y, o.z};
            }
            __syncthreads();                                                    // a level reads what the level before wrote
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
int check_table(const char* who, const int32_t* parents, const int32_t* children, const float* lengths, int K) {
    EG_REQUIRE(parents && children && lengths, EG_ERR_BAD_ARG, "%s: null parents / children / lengths", who);
    EG_REQUIRE(K >= 1 && K <= MAX_K, EG_ERR_UNSUPPORTED, "%s: bones=%d (1..%d)", who, K, MAX_K);
    bool made[MAX_K + 1] = {};
    made[0] = true;                                                             // the root
    for (int k = 0; k < K; ++k) {
        const int a = parents[k], b = children[k];
        EG_REQUIRE(b != 0, EG_ERR_BAD_ARG, "%s: bone %d: child is joint 0, the root", who, k);
        EG_REQUIRE(b >= 1 && b <= K, EG_ERR_BAD_ARG, "%s: bone %d: child=%d outside the joints 1..%d", who, k, b, K);
        EG_REQUIRE(!made[b], EG_ERR_BAD_ARG, "%s: bone %d: child=%d is the child of an earlier bone (used twice)", who, k, b);
        EG_REQUIRE(a >= 0 && a <= K && made[a], EG_ERR_BAD_ARG,
                   "%s: bone %d: parent=%d is neither the root nor the child of an earlier bone (the table must be in topological order)", who, k, a);
        EG_REQUIRE(isfinite(lengths[k]) && lengths[k] > 0.f, EG_ERR_BAD_ARG, "%s: bone %d: length=%g (need finite and > 0)", who, k, (double)lengths[k]);
        made[b] = true;
    }
    return EG_OK;
}

int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

int reduce_rate(const char* who, int& L, int& M) {
    EG_REQUIRE(L >= 1 && M >= 1, EG_ERR_BAD_ARG, "%s: rate L=%d / M=%d (need >= 1)", who, L, M);
    const int g = gcd_int(L, M);
    L /= g; M /= g;
    EG_REQUIRE(L <= MAX_LM && M <= MAX_LM, EG_ERR_UNSUPPORTED, "%s: the frame-rate ratio L=%d / M=%d: supported up to max(L, M) <= %d", who, L, M, MAX_LM);
    return EG_OK;
}

int common_checks(const char* who, const void* src, const void* dst, int B, int T, const int32_t* parents, const int32_t* children,
                  const float* lengths, int K, const void* d_table, int draws, int frame_unit, const void* d_mean) {
    EG_REQUIRE(src, EG_ERR_BAD_ARG, "%s: null input", who);
    EG_REQUIRE(dst, EG_ERR_BAD_ARG, "%s: null output", who);
    EG_REQUIRE(d_table, EG_ERR_BAD_ARG, "%s: null d_table", who);
    int rc = check_table(who, parents, children, lengths, K);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(eg_aligned16(src) && eg_aligned16(dst), EG_ERR_ALIGN, "%s: input / output not 16-byte aligned", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_table) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_mean) & 3u) == 0, EG_ERR_ALIGN,
               "%s: d_table / d_mean not 4-byte aligned", who);
    EG_REQUIRE(B >= 1 && T >= 1, EG_ERR_BAD_ARG, "%s: rows=%d frames=%d (need >= 1)", who, B, T);
    EG_REQUIRE(draws >= 1 && B % draws == 0, EG_ERR_BAD_ARG, "%s: rows=%d is not a multiple of draws=%d", who, B, draws);
    EG_REQUIRE(frame_unit >= 1, EG_ERR_BAD_ARG, "%s: frame_unit=%d (need >= 1)", who, frame_unit);
    return EG_OK;
}

// What eg_skeleton_joints and eg_skeleton_rotations check behind their own arguments, in the header's order -- the rate, out_stride, the grid
// and the index range of an output of `per_frame` floats per frame -- and the rest of the kernel's arguments: a.L, a.M, a.tiles, a.T_out.
int forward_args(const char* who, Args& a, int L, int M, long long out_stride, int per_frame) {
    int rc = reduce_rate(who, L, M);
    if (rc != EG_OK) return rc;
    const long long t_out = out_frames(a.T, L, M);
    EG_REQUIRE(out_stride >= t_out, EG_ERR_BAD_ARG, "%s: out_stride=%lld < %lld output frames of %d input frames at L=%d / M=%d", who, out_stride,
               t_out, a.T, L, M);
    const long long tiles = (out_stride + TF - 1) / TF;
    EG_REQUIRE(tiles * a.B <= 0x7fffffffll && (long long)a.B * out_stride * per_frame < (1ll << 40), EG_ERR_UNSUPPORTED,
               "%s: rows=%d x out_stride=%lld: grid / index range", who, a.B, out_stride);
    a.L = L; a.M = M; a.tiles = (int)tiles; a.T_out = out_stride;
    return EG_OK;
}

// One workgroup per tile of every row.
int launch(void (*kernel)(Args), const Args& a, size_t lds_floats, void* stream, const char* what) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)a.tiles * a.B)), dim3(THREADS), lds_floats * sizeof(float), static_cast<hipStream_t>(stream), a);
    return eg_check_launch(what);
}

int check_rest(const char* who, const double* rest, int K) {
    EG_REQUIRE(rest, EG_ERR_BAD_ARG, "%s: null rest", who);
    for (int k = 0; k < K; ++k) {
        const double* r = rest + 3 * k;
        EG_REQUIRE(isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]), EG_ERR_BAD_ARG, "%s: rest row %d: (%g, %g, %g) is not finite", who, k, r[0],
                   r[1], r[2]);
        const double nrm = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        EG_REQUIRE(nrm >= 1e-6, EG_ERR_BAD_ARG, "%s: rest row %d: norm=%g (need >= 1e-6: a rest direction)", who, k, nrm);
    }
    return EG_OK;
}

}  // namespace

extern "C" int eg_skeleton_check(const int32_t* parents, const int32_t* children, const float* lengths, int32_t bones) {
    return check_table("eg_skeleton_check", parents, children, lengths, bones);
}

extern "C" int64_t eg_skeleton_out_frames(int64_t n, int32_t L, int32_t M) {
    int l = L, m = M;
    if (n < 0 || n >= (1ll << 40) || reduce_rate("eg_skeleton_out_frames", l, m) != EG_OK) return -1;
    return out_frames(n, l, m);
}

extern "C" int32_t eg_skeleton_tile_frames(void) { return TF; }

extern "C" int eg_skeleton_joints(const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children, const float* lengths,
                                  int32_t bones, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                                  const float* d_mean, int32_t unit, int32_t L, int32_t M, float* joints, int64_t out_stride, void* stream) {
    const char* who = "eg_skeleton_joints";
    int rc = common_checks(who, track, joints, rows, T, parents, children, lengths, bones, d_table, draws, frame_unit, d_mean);
    if (rc != EG_OK) return rc;
    Args a = {track, static_cast<const int*>(d_table), d_frames, d_mean, joints, rows, T, bones, draws, frame_unit};
    rc = forward_args(who, a, L, M, out_stride, 3 * (bones + 1));
    if (rc != EG_OK) return rc;
    const bool native = a.L == 1 && a.M == 1;
    return launch(unit ? (native ? skeleton_joints_kernel<true, true> : skeleton_joints_kernel<true, false>)
                       : (native ? skeleton_joints_kernel<false, true> : skeleton_joints_kernel<false, false>),
                  a, HEAD + round4(SLOTS * 3 * bones + 8) + (bones + 1) * NC, stream, "skeleton_joints");
}

extern "C" int eg_skeleton_dir_vec(const float* joints, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children, const float* lengths,
                                   int32_t bones, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                                   const float* d_mean, float* dir_vec, void* stream) {
    const char* who = "eg_skeleton_dir_vec";
    int rc = common_checks(who, joints, dir_vec, rows, T, parents, children, lengths, bones, d_table, draws, frame_unit, d_mean);
    if (rc != EG_OK) return rc;
    const long long tiles = ((long long)T + TF - 1) / TF;
    EG_REQUIRE(tiles * rows <= 0x7fffffffll && (long long)rows * T * 3 * (bones + 1) < (1ll << 40), EG_ERR_UNSUPPORTED,
               "%s: rows=%d x frames=%d: grid / index range", who, rows, T);
    Args a = {joints, static_cast<const int*>(d_table), d_frames, d_mean, dir_vec, rows, T, bones, draws, frame_unit, 1, 1, (int)tiles, T};
    return launch(skeleton_dir_vec_kernel, a, HEAD + round4(TF * 3 * (bones + 1) + 8), stream, "skeleton_dir_vec");
}

extern "C" int eg_skeleton_rest_check(const double* rest, int32_t bones) {
    const char* who = "eg_skeleton_rest_check";
    EG_REQUIRE(bones >= 1 && bones <= MAX_K, EG_ERR_UNSUPPORTED, "%s: bones=%d (1..%d)", who, bones, MAX_K);
    return check_rest(who, rest, bones);
}

extern "C" int eg_skeleton_levels(const int32_t* parents, const int32_t* children, const float* lengths, int32_t bones, const double* rest,
                                  int32_t* words) {
#pragma clang fp contract(off)                          // the rows are x / sqrt(x.x) in plain float64, every operation rounded once
    const char* who = "eg_skeleton_levels";
    int rc = check_table(who, parents, children, lengths, bones);
    if (rc != EG_OK) return rc;
    rc = check_rest(who, rest, bones);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(words, EG_ERR_BAD_ARG, "%s: null words", who);
    const int K = bones;
    int owner[MAX_K + 1], depth[MAX_K], count[MAX_K + 1] = {};
    for (int j = 0; j <= K; ++j) owner[j] = -1;
    int nlev = 0;
    int32_t* pb = words + lv_parents(K);
    for (int k = 0; k < K; ++k) {                       // topological order: the parent joint's bone, if any, came earlier
        pb[k] = owner[parents[k]];
        depth[k] = pb[k] < 0 ? 0 : depth[pb[k]] + 1;
        owner[children[k]] = k;
        ++count[depth[k]];
        nlev = depth[k] + 1 > nlev ? depth[k] + 1 : nlev;
    }
    words[0] = nlev;
    int at[LEVEL_SLOTS];
    for (int l = 0, s = 0; l < LEVEL_SLOTS; ++l) {
        words[LV_FIRST + l] = s;
        at[l] = s;
        if (l < nlev) s += count[l];
    }
    for (int k = 0; k < K; ++k) words[LV_ORDER + at[depth[k]]++] = k;                 // by depth, table order inside a level
    for (int k = 0; k < K; ++k) {
        const double* r = rest + 3 * k;
        const double nrm = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        for (int c = 0; c < 3; ++c) {
            const float v = (float)(r[c] / nrm);
            words[lv_rest(K) + 3 * k + c] = *reinterpret_cast<const int32_t*>(&v);
        }
    }
    return EG_OK;
}

extern "C" int eg_skeleton_rotations(const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                                     const float* lengths, int32_t bones, const double* rest, const void* d_levels, const int32_t* d_frames,
                                     int32_t draws, int32_t frame_unit, const float* d_mean, int32_t space, int32_t L, int32_t M,
                                     float* rotations, int64_t out_stride, void* stream) {
    const char* who = "eg_skeleton_rotations";
    int rc = common_checks(who, track, rotations, rows, T, parents, children, lengths, bones, d_levels, draws, frame_unit, d_mean);
    if (rc != EG_OK) return rc;
    rc = check_rest(who, rest, bones);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(space == EG_SKELETON_SPACE_LOCAL || space == EG_SKELETON_SPACE_GLOBAL, EG_ERR_BAD_ARG, "%s: space=%d (0: local, 1: global)", who, space);
    Args a = {track, static_cast<const int*>(d_levels), d_frames, d_mean, rotations, rows, T, bones, draws, frame_unit};
    rc = forward_args(who, a, L, M, out_stride, 4 * bones);
    if (rc != EG_OK) return rc;
    const bool native = a.L == 1 && a.M == 1;
    return launch(space == EG_SKELETON_SPACE_GLOBAL ? (native ? skeleton_rotations_kernel<true, true> : skeleton_rotations_kernel<false, true>)
                                                    : (native ? skeleton_rotations_kernel<true, false> : skeleton_rotations_kernel<false, false>),
                  a, RHEAD + round4(SLOTS * 3 * bones + 8) + bones * 4 * TF, stream, "skeleton_rotations");
}
